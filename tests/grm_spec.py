"""The numpy statement of grm / related_pairs (SnpArrays.grm's methods :GRM and :Robust) over an n x p float64 array of
genotypes -- allele counts or dosages -- with NaN for a missing one.  It is the yardstick of the device path.

C is the set of kept columns and m = |C|; mu_j and sinv_j are the handle's own (mu_sigma()), or those of mu_sigma(g) below.
    c_ij = g_ij - mu_j for an observed genotype, 0 for a missing one (imputed by the mean); a column without a finite mu
           (every genotype missing) is all zeros, never NaN * 0
    GRM:     Phi_ik = sum_{j in C} (c_ij sinv_j) (c_kj sinv_j) / (2 m)
    Robust:  Phi_ik = sum_{j in C} c_ij c_kj / (2 sum_{j in C, mu_j finite} mu_j (1 - mu_j / 2)), the divisor summed over
             ascending j
Any order of an m-term float64 sum is within m u S_ik of the exact value, u = 2^-53 and S = |X| |X|' (|C| |C|' for Robust),
and the entries carry at most two roundings each: bound() is 2 (m + 8) u S / div + 1e-300, elementwise."""
import numpy as np

from qc_spec import as_mask

U = 2.0 ** -53
METHODS = ("GRM", "Robust")


def genotypes(codes):
    """Allele counts with -1 for a missing genotype as float64 with NaN."""
    return np.where(codes < 0, np.nan, codes).astype(np.float64)


def mu_sigma(g):
    """mu_j = mean of the observed genotypes (NaN without any), sinv_j = 1 / sqrt(mu_j (1 - mu_j / 2)), 1 where that root
    is not positive: what the handles compute."""
    obs = ~np.isnan(g)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(obs, g, 0.0).sum(axis=0) / obs.sum(axis=0)
        s = np.sqrt(mu * (1.0 - mu / 2.0))
        sinv = np.where(s > 0.0, 1.0 / s, 1.0)
    return mu, sinv


def operand(g, mu, sinv, cols=None, method="GRM"):
    """(the n x m matrix whose product with its transpose is the numerator, the divisor)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}")
    keep = as_mask(cols, g.shape[1])
    g, mu, sinv = g[:, keep], mu[keep], sinv[keep]
    m = g.shape[1]
    if m == 0:
        raise ValueError("the selection of columns is empty")
    fin = np.isfinite(mu)
    c = np.where(np.isnan(g) | ~fin[None, :], 0.0, g - np.where(fin, mu, 0.0)[None, :])
    if method == "GRM":
        return c * sinv[None, :], 2.0 * m
    t = (mu * (1.0 - mu / 2.0))[fin]
    return c, 2.0 * (float(np.cumsum(t)[-1]) if t.size else 0.0)          # (cumsum: in ascending order)


def grm(g, mu, sinv, cols=None, method="GRM"):
    a, div = operand(g, mu, sinv, cols, method)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a @ a.T) / div


def bound(g, mu, sinv, cols=None, method="GRM"):
    a, div = operand(g, mu, sinv, cols, method)
    a = np.abs(a)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * (a.shape[1] + 8) * U * (a @ a.T) / div + 1e-300


def related_pairs(phi, threshold=0.125):
    """(i, k) with i < k and phi[i, k] > threshold, in the order (i, k)."""
    i, k = np.nonzero(np.triu(phi > threshold, 1))
    return i, k


def check(got, want, tol, what=""):
    """got against the spec's (want, tol), elementwise; where the spec has no finite number (a divisor of 0) got has the same."""
    nan = ~np.isfinite(want)
    assert got.shape == want.shape and np.array_equal(got[nan], want[nan], equal_nan=True), what
    err = np.abs(np.where(nan, 0.0, got - np.where(nan, 0.0, want)))
    bad = ~nan & ~(err <= np.where(nan, 0.0, tol))
    assert not bad.any(), (what, float(err[bad].max()), float(tol[bad].min()), np.argwhere(bad)[:4].tolist())


def assert_within(got, g, mu, sinv, cols, method, what=""):
    check(got, grm(g, mu, sinv, cols, method), bound(g, mu, sinv, cols, method), what)
