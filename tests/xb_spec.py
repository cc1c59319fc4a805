"""The dense forward product X B of the 2-bit matrix and the polygenic score, stated in numpy from a code matrix (n x p allele
counts, -1 = missing): what mih_snp_transpose / mih_xb_dense (csrc/transpose.hip, csrc/xb.hip) and SnpLinAlg.transpose / xb / score
are held to.

X is the matrix the SnpLinAlg presents under its flags.  With mu_j and sinv_j the f64 numbers of mu_sigma() below (what
mih_snp_mu_sigma returns: the handle forms them from the counts by the same correctly rounded steps), entry (i, j) is
    x_ij = (g_ij - [center] mu_j) [scale] sinv_j,    g_ij = the code, or, where it is missing, [impute] mu_j,
so that, with a_jt = ([scale] sinv_j) B_jt,
    (X B)_it = sum_j code_ij a_jt  +  [impute] sum_{j in miss(i)} mu_j a_jt  -  [center] sum_j mu_j a_jt          (code = 0 where missing)
-- three sums over f64 inputs, each of them a rational number.  exact() evaluates them without rounding, xb() in plain f64.
A SNP without an observed genotype has mu_j = NaN (0 / 0): every entry of X B is NaN when the call centres or imputes.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                       # unit roundoff of f64
COEF_CHUNK = 1024                    # kXbChunk of csrc/xb.hip: entries of a column of B per workgroup of k_xb_coef


def transpose_codes(codes):
    """The code matrix of the transposed genotypes: SNPs as rows, samples as columns."""
    return np.ascontiguousarray(np.asarray(codes).T)


def mu_sigma(codes):
    """mu_j = (n1 + 2 n2) / (n - nmiss) and sinv_j = 1 / sqrt(mu_j (1 - mu_j / 2)), 1 where that root is not positive (or NaN)."""
    n = codes.shape[0]
    n1, n2, nm = ((codes == v).sum(axis=0).astype(np.float64) for v in (1, 2, -1))
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (n1 + 2.0 * n2) / (float(n) - nm)
        s = np.sqrt(m * (1.0 - m / 2.0))
        sinv = np.where(s > 0.0, 1.0 / s, 1.0)
    return m, sinv


def standardized(codes, center, scale, impute):
    """The n x p matrix the SnpLinAlg presents, in f64: ((g - mu) sinv, one rounding per operation)."""
    mu, sinv = mu_sigma(codes)
    g = np.where(codes < 0, (mu if impute else np.zeros_like(mu))[None, :], codes.astype(np.float64))
    if center:
        g = g - mu[None, :]
    if scale:
        g = g * sinv[None, :]
    return g


def xb(codes, B, center, scale, impute):
    """X B in plain f64 (n, or n x t for a p x t B)."""
    with np.errstate(invalid="ignore"):
        return standardized(codes, center, scale, impute) @ np.asarray(B, dtype=np.float64)


def score(codes, weights, cols=None, average=False):
    """`plink --score`: sum_j w_j g_ij over raw allele counts, a missing genotype counting as the SNP's mean dosage mu_j (center 0,
    scale 0, impute 1).  cols: the SNPs the weights belong to (indices or a boolean mask; the others have weight 0); average: the
    sum divided by 2 x the number of scored SNPs."""
    p = codes.shape[1]
    w = np.zeros(p)
    if cols is None:
        w[:] = np.asarray(weights, dtype=np.float64)
        scored = p
    else:
        idx = np.flatnonzero(cols) if np.asarray(cols).dtype == np.bool_ else np.asarray(cols, dtype=np.int64)
        w[idx] = np.asarray(weights, dtype=np.float64)
        scored = idx.size
    s = xb(codes, w, False, False, True)
    return s / (2.0 * scored) if average else s


# ---- exact values ----------------------------------------------------------------------------------------------------------------
def exact_fraction(codes, B, center, scale, impute):
    """(X B)_it as Fractions, term by term in rational arithmetic (object array n x t; None where the value is NaN).  O(n p t)
    Fraction operations: for the small shapes of the CPU test."""
    codes = np.asarray(codes)
    B = np.asarray(B, dtype=np.float64).reshape(codes.shape[1], -1)
    n, p = codes.shape
    mu, sinv = mu_sigma(codes)
    out = np.empty((n, B.shape[1]), dtype=object)
    nan_all = (center or impute) and bool(np.isnan(mu).any())
    fmu = [None if math.isnan(v) else Fraction(float(v)) for v in mu]
    fs = [Fraction(float(v)) if scale else Fraction(1) for v in sinv]
    for t in range(B.shape[1]):
        a = [fs[j] * Fraction(float(B[j, t])) for j in range(p)]
        c = sum((fmu[j] * a[j] for j in range(p)), Fraction(0)) if center and not nan_all else Fraction(0)
        for i in range(n):
            if nan_all:
                out[i, t] = None
                continue
            v = Fraction(0)
            for j in range(p):
                g = int(codes[i, j])
                if g > 0:
                    v += g * a[j]
                elif g < 0 and impute:
                    v += fmu[j] * a[j]
            out[i, t] = v - c
    return out


def _two_prod(a, b):
    """a b = hi + lo exactly (Dekker; no overflow or underflow at the magnitudes of the tests)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _exact_dot(W, v):
    """W v without rounding: W an r x p matrix of small non-negative integers (codes, a 0 / 1 mask), v f64.  v is peeled into limbs
    of 30 bits below its largest exponent -- v = sum_l k_l 2^(E - 30 (l + 1)) with integers |k_l| < 2^30, every step exact in f64 --
    and each limb's dot product is taken in int64 (below 2^53 for p < 2^21).  A list of r Fractions."""
    W = np.ascontiguousarray(W, dtype=np.int64)
    total = [Fraction(0)] * W.shape[0]
    r = np.array(v, dtype=np.float64)
    if not r.any():
        return total
    assert np.isfinite(r).all() and W.shape[1] < 2 ** 21 and W.max(initial=0) <= 2
    E = int(np.frexp(np.abs(r).max())[1])                        # |v| < 2^E
    for level in range(1, 80):
        if not r.any():
            return total
        q = math.ldexp(1.0, E - 30 * level)
        k = np.trunc(r / q)                                      # (a division by a power of two: exact)
        r = r - k * q                                            # exact: the part of r below q
        dots = W @ k.astype(np.int64)
        fq = Fraction(q)
        total = [tv + int(d) * fq for tv, d in zip(total, dots)]
    raise AssertionError("more than 2400 binades in one vector")


def exact_parts(codes, B, scale):
    """The three sums of the module's header for a p x t B without rounding: every product sinv_j B_jt and mu_j (sinv_j B_jt) is
    split into f64 pieces that add up to it exactly (_two_prod), and each sum over SNPs is an exact integer dot product per piece
    (_exact_dot).  Returns (main (n x t), imputation (n x t), centring (t)) as object arrays of Fractions; mu = NaN counts as 0
    here (exact() answers NaN for it).  Computed once per (matrix, B, scale) and combined for every pair of the other two flags."""
    codes = np.asarray(codes)
    B = np.asarray(B, dtype=np.float64).reshape(codes.shape[1], -1)
    n, p = codes.shape
    mu, sinv = mu_sigma(codes)
    mu0 = np.where(np.isnan(mu), 0.0, mu)
    g = np.where(codes < 0, 0, codes).astype(np.int64)
    miss = (codes < 0).astype(np.int64)
    ones = np.ones((1, p), dtype=np.int64)
    main, imp = np.empty((n, B.shape[1]), dtype=object), np.empty((n, B.shape[1]), dtype=object)
    cen = np.empty(B.shape[1], dtype=object)
    for t in range(B.shape[1]):
        pieces = list(_two_prod(sinv, B[:, t])) if scale else [B[:, t].copy()]
        m = []                                                  # mu a in exact pieces
        for piece in pieces:
            m += list(_two_prod(mu0, piece))
        main[:, t] = [sum(vs, Fraction(0)) for vs in zip(*(_exact_dot(g, q) for q in pieces))]
        imp[:, t] = [sum(vs, Fraction(0)) for vs in zip(*(_exact_dot(miss, q) for q in m))]
        cen[t] = sum((_exact_dot(ones, q)[0] for q in m), Fraction(0))
    return main, imp, cen


def exact(codes, B, center, scale, impute, parts=None):
    """(X B)_it as an n x t object array of Fractions (None where NaN) from exact_parts (parts: those of this scale flag, if the
    caller has them), for shapes where exact_fraction would take minutes: the same rational numbers.  tests/test_xb_spec_cpu.py holds it against
    exact_fraction."""
    main, imp, cen = exact_parts(codes, B, scale) if parts is None else parts
    out = np.empty(main.shape, dtype=object)
    if (center or impute) and np.isnan(mu_sigma(np.asarray(codes))[0]).any():
        out[:] = None
        return out
    for t in range(main.shape[1]):
        for i in range(main.shape[0]):
            out[i, t] = main[i, t] + (imp[i, t] if impute else 0) - (cen[t] if center else 0)
    return out


# ---- the tolerance ---------------------------------------------------------------------------------------------------------------
def quantum(a_max, digits=None):
    """What one entry of a column of a = sinv B may be off in the pass's fixed point, as the header states it above
    mih_xtv_batched_fmt: the quantum is 2^-54 of the largest entry the fixed point carries, 2^-53 at worst (4910, the default of
    every fused context, and 428: ebits = 53); the 1316 format carries three more bits (ebits = 56): 2^-56 at worst."""
    if digits in (None, 0, 4910, 428):
        return a_max * 2.0 ** -53
    if digits == 1316:
        return a_max * 2.0 ** -56
    raise ValueError(f"no documented quantum for residual format {digits}")


def bound(codes, B, flags, digits=None):
    """The elementwise tolerance |device - exact| <= bound (n x t, f64) of SnpLinAlg.xb, assembled from what the device does
    (csrc/xb.hip), u = 2^-53, a_jt the f64 product sinv_j B_jt (B_jt itself without scale), ma_jt the f64 product mu_j a_jt:

    the pass over the row image (main term, documented above mih_xtv_batched_fmt)
      cnt_i q_t            every a_jt is rounded to the fixed point once, at most quantum(max_j |a_jt|) off, and enters row i code_ij
                           times: cnt_i = sum_j code_ij;
      64 u S_it            the f64 recombination, "64 ulp": at most 64 roundings (28 digit planes, 16 row slices, the scale, the side
                           channel's compensated sum), each relative to a partial sum of the terms code_ij a_jt, none of which
                           exceeds S_it = sum_j code_ij |a_jt| -- the ulp is taken of S, not of the result, which may have cancelled;
    the front end
      [scale] u (S_it + I_it + C_t)       a_jt is one rounding off sinv_j B_jt, and enters the three sums with the weights code_ij,
                           mu_j on the missing entries, mu_j: I_it = sum_{j in miss(i)} |ma_jt| (0 without impute), C_t = sum_j |ma_jt|
                           (0 without center);
      u (I_it + C_t)       ma_jt is one rounding off mu_j a_jt;
    the back end
      (k_i - 1) u I_it     the imputation chain: k_i - 1 additions of k_i = |miss(i)| terms in ascending order;
      D u C_t              c_t, the fixed tree: a term passes at most D = 3 + 8 + ceil(ceil(p / 1024) / 256) + 8 additions (four
                           entries a thread, a tree over 256 threads; the chunks' sums the same way);
      u (S_it + I_it)      the addition of the chain to the main term (where the sample has a missing entry);
      u (S_it + I_it + C_t)  the subtraction of c_t (with center).
    The sum is inflated by 1 + 2^-20 for the second-order terms and the bound's own f64 evaluation.  No constant is fitted.
    Every term is linear in |B[:, t]|: the bound of 2^e B[:, t] is 2^e times this one, exactly.  digits may be a tuple of
    formats: the list of their bounds (only the quantum differs)."""
    center, scale, impute = (bool(f) for f in flags)
    codes = np.asarray(codes)
    B = np.asarray(B, dtype=np.float64).reshape(codes.shape[1], -1)
    n, p = codes.shape
    mu, sinv = mu_sigma(codes)
    g = np.where(codes < 0, 0, codes).astype(np.float64)
    miss = (codes < 0).astype(np.float64)
    a = np.abs(sinv[:, None] * B) if scale else np.abs(B)
    with np.errstate(invalid="ignore"):
        ma = np.abs(mu[:, None] * a)
    ma = np.where(np.isnan(ma), 0.0, ma)
    cnt = g.sum(axis=1)[:, None]
    k = miss.sum(axis=1)[:, None]
    S = g @ a
    I = miss @ ma if impute else np.zeros_like(S)
    C = ma.sum(axis=0)[None, :] if center else np.zeros((1, B.shape[1]))
    D = 3 + 8 + -(-(-(-p // COEF_CHUNK)) // 256) + 8
    out = 64 * U * S
    if scale:
        out = out + U * (S + I + C)
    out = out + U * (I + C)
    if impute:
        out = out + np.maximum(k - 1, 0) * U * I + np.where(k > 0, U * (S + I), 0.0)
    if center:
        out = out + D * U * C + U * (S + I + C)
    amax = a.max(axis=0)

    def of(dg):
        q = np.array([quantum(v, dg) for v in amax])[None, :]
        return (cnt * q + out) * (1.0 + 2.0 ** -20)
    return [of(dg) for dg in digits] if isinstance(digits, (tuple, list)) else of(digits)
