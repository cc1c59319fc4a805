"""Helpers shared by the GPU test files (split out of test_gpu_parity.py in round 6)."""
import os

import numpy as np

from conftest import hash_folds


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) + 1e-300))

def _run_probe_snippet(snippet, out_file, extra_env=None, probes=True, timeout=900):
    """A python snippet in its own process, on the measurement build of the library (MENDELIHT_HIP_PROBES=1) or on the product."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "MENDELIHT_HIP_PROBES"}
    if probes:
        env["MENDELIHT_HIP_PROBES"] = "1"
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, "-c", snippet, root, str(out_file)], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out_file)

def _sim(oracle, ox, rng, k, scale=0.5):
    p = ox.p
    b = np.zeros(p)
    supp = rng.choice(p, k, replace=False)
    b[supp] = rng.standard_normal(k) * scale
    mask = np.zeros(p, np.uint8)
    mask[supp] = 1
    return ox.xv_masked(mask, b)

def _mv_problem(oracle, ox, rng, r, k, q=1):
    p, n = ox.p, ox.n
    B = np.zeros((r, p))
    for _ in range(k):
        B[rng.integers(r), rng.integers(p)] = rng.standard_normal() * 0.6
    XB = np.zeros((r, n))
    for i in range(r):
        mask = (B[i] != 0).astype(np.uint8)
        XB[i] = ox.xv_masked(mask, B[i])
    A = rng.standard_normal((r, r))
    L = np.linalg.cholesky(A @ A.T / r + np.eye(r) * 0.5)
    Z = np.vstack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    Cm = rng.standard_normal((r, q))
    Y = XB + Cm @ Z + L @ rng.standard_normal((r, n))
    return Y, Z

_BT_TIE = 1e-13      # orc_result.bt_cond below this: `old_logl > new_logl` compared two sums of n terms that agree to their rounding error

_NUDGES = [1.0 + e * 2.0 ** -51 for e in (2, 1, 3, 4, 6, 8)]      # a few ulps: one nudge can land on the same branch by luck (seed 2449)

def _unstable(a, b, rtol, atol=1e-10):
    """The oracle against ITSELF on covariates scaled by 1 + a few 2^-51 (a: the run on the original input, b: a nudged one, dicts
    of arrays / scalars): True when an ulp-sized change of the input moves the oracle's own answer by more than the tolerance.
    Such a trajectory amplifies rounding from step to step (seed 2121 of tools/fuzz_parity.py: the intercepts of a multivariate
    fit drift apart by x1.87 per iteration, 1e-15 -> 4e-7 over 40 steps; seed 2275: a Bernoulli fit that backtracks three
    times in most steps) -- no two floating-point implementations agree on it, the reference under another BLAS included,
    so the sweeps do not hold the GPU to it."""
    for key in a:
        va, vb = np.asarray(a[key], dtype=float), np.asarray(b[key], dtype=float)
        if va.shape != vb.shape or not np.allclose(va, vb, rtol=rtol, atol=atol):
            return True
    return False

def _rows_permuted(oracle, ox, perm):
    """The oracle's matrix with its rows in another order.  With y, z and every per-sample option permuted alike the PROBLEM is the same
    one -- same columns, same means and scales (integer counts), same optimum -- but every sum over the samples (X'r, the loglikelihood,
    the step size, debias!'s normal equations) adds its terms in another order: exactly the freedom another correct implementation
    of the reference has (a threaded BLAS, this library's tiles).  A trajectory the oracle does not reproduce under that is one
    nobody can be held to (the set-aside classes that were accepted by argument)."""
    keep, n = ox._keep, ox.n
    if keep.dtype != np.uint8:
        return oracle.Mat.from_dense(np.asarray(keep)[perm])
    code = np.stack([(keep >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(keep.shape[0], -1)[:, :n][:, perm]
    pad = np.zeros((keep.shape[0], keep.shape[1] * 4), np.uint8)
    pad[:, :n] = code
    return oracle.Mat.from_bed_columns(pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6), n)

def _row_orders(n, count=4):
    return [np.random.default_rng(7700 + t).permutation(n) for t in range(count)]

def _within_own_spread(o, own, got, tols, factor=4.0):
    """o: the oracle's answer, own: its answers to the same problem re-associated (ulp nudges of z, other row orders), got: the
    device's; dicts of arrays / scalars over the keys of tols = {key: (rtol, atol)}.  True when the device is within the tolerance
    PLUS factor x the oracle's own spread, entry by entry, and that spread is not nil: a trajectory the oracle reproduces to within
    the tolerance but not by much (seed 16276 of tools/fuzz_parity.py: an effect of 0.008 moves by 8e-7 from one row order to the
    next, the device's is 1.5e-6 away, the tolerance is 8e-7)."""
    any_spread = False
    for key, (rtol, atol) in tols.items():
        ref = np.asarray(o[key], dtype=float)
        spread = np.max([np.abs(np.asarray(v[key], dtype=float) - ref) for v in own], axis=0)
        any_spread |= bool(np.max(spread) > 0.0)
        if np.shape(got[key]) != ref.shape or not np.all(np.abs(np.asarray(got[key], dtype=float) - ref) <= rtol * np.abs(ref) + atol + factor * spread):
            return False
    return any_spread

def _exact_xtv(g, r):
    from fractions import Fraction
    rf = [Fraction(float(v)) for v in r]
    return [sum((int(gi) * ri for gi, ri in zip(g[j], rf) if gi), Fraction(0)) for j in range(g.shape[0])]

def _dosages(cols, n):
    p = cols.shape[0]
    bits = np.unpackbits(cols, axis=1, bitorder="little").reshape(p, -1, 2)[:, :n, :]
    code = bits[:, :, 0] + 2 * bits[:, :, 1]
    return np.select([code == 0, code == 2, code == 3], [0, 1, 2], default=0)

def _same_fit(a, b, what):
    assert a.iter == b.iter, (what, a.iter, b.iter)
    assert list(a.trace["backtracks"]) == list(b.trace["backtracks"]), what
    assert np.array_equal(np.flatnonzero(a.beta), np.flatnonzero(b.beta)), what
    # every sum of the resident chain is formed in the host-driven kernels' order, and the scalar log of the loglikelihood's closed
    # form is csrc/scalar_log.h's on both sides; only the Gamma family's lgamma still comes from another libm (device against
    # host): the last bit of a Gamma fit's trace may differ, every other trace is equal bit for bit
    np.testing.assert_allclose(a.trace["logl"], b.trace["logl"], rtol=4e-16, atol=0, err_msg=what)
    assert np.array_equal(a.trace["tol"], b.trace["tol"]), what
    assert np.array_equal(a.beta, b.beta) and np.array_equal(a.c, b.c), what
    assert np.array_equal(a.mu, b.mu), what
    assert a.choose_fired == b.choose_fired, what

def _config3_problem(mih, n, p, seed=2024):
    """BASELINE configs[3] in small: Bernoulli/Logit response with 10 true effects on a synthetic SnpArray, explicit hash folds."""
    x = mih.SnpLinAlg.synthetic(n, p, seed=seed)
    rng = np.random.default_rng(2025)
    supp = np.sort(rng.choice(p, 10, replace=False))
    eta = x.xv_sparse(supp, rng.standard_normal(10) * 0.5)
    yb = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float)
    return x, yb, hash_folds(n, 5)

def _config4_problem(x, rng, r, k, lo=0.15, hi=0.45):
    """r traits on matrix x with k planted effects spread over the traits (each trait its own columns), an intercept per trait and
    errors with an AR(1) covariance: returns Y (r x n), the planted B (r x p) as {trait: (columns, effects)} and Sigma."""
    n, p = x.n, x.p
    lin = rng.choice(r * p, k, replace=False)
    Sigma = 0.5 ** np.abs(np.subtract.outer(np.arange(r), np.arange(r)))        # AR(1), rho = 0.5
    L = np.linalg.cholesky(Sigma)
    Y = L @ rng.standard_normal((r, n))
    planted = {}
    for t in range(r):
        cols = np.unique(lin[lin % r == t] // r)
        eff = rng.choice([-1.0, 1.0], cols.size) * rng.uniform(lo, hi, cols.size)
        planted[t] = (cols, eff)
        Y[t] += x.xv_sparse(cols, eff) + 1.0 + 0.1 * t
    return Y, planted, Sigma


def peel_rule(r, ratio=64.0, max_rows=64):
    """The outlier guard of the fixed-point residual restated (csrc/peel.h): max|r| per strided 256-row block (block b: rows
    256 b + t + 16384 j), bq = the ceil(B/4)-th smallest of the B non-empty blocks' maxima; the guard fires iff max|r| > ratio * bq;
    then the rows with |r_i| > ratio * bq are peeled if there are at most max_rows of them.  Returns the peeled row indices."""
    r = np.asarray(r, dtype=np.float64)
    n = r.size
    nb = min(64, (n + 255) // 256)
    a = np.abs(r)
    bmax = np.zeros(nb)
    for b in range(nb):
        rows = np.concatenate([np.arange(lo, min(lo + 256, n)) for lo in range(256 * b, n, 16384)])
        bmax[b] = a[rows].max()
    bq = np.sort(bmax)[(nb + 3) // 4 - 1]
    with np.errstate(over="ignore"):
        tau = ratio * bq
    if not (bmax.max() > tau) or not np.isfinite(bmax.max()):
        return np.zeros(0, dtype=np.int64)
    rows = np.flatnonzero(a > tau)
    return rows if rows.size <= max_rows else np.zeros(0, dtype=np.int64)


def xv_documented_order(G, a, b, max_groups=16):
    """The summation order csrc/xv.hip documents for X beta over a support of the 2-bit matrix, restated: G (n x nnz) the stored
    dosages 0 / 1 / 2 of the support columns in LIST order (a missing entry is stored as 0), a_t = sinv_t v_t (or v_t) and
    b_t = -mu_t a_t (or 0.0) as doubles.  groups = min(nnz, 16), per = ceil(nnz / groups); group g covers the columns
    [g per, min((g + 1) per, nnz)); acc and bsum accumulate in column order, part_g = acc + bsum, out = ((0.0 + part_0) +
    part_1) + ... over all `groups` (an empty trailing group adds acc = bsum = +0.0).  g a is exact in f64 for g in {0, 1, 2}, so
    fma(g, a, acc) is acc + g * a with ONE rounding and numpy predicts the kernel's bits.  The fix-up of imputed entries is not
    part of it."""
    G = np.asarray(G)
    n, nnz = G.shape
    out = np.zeros(n)
    if nnz == 0:
        return out
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    groups = min(nnz, max_groups); per = -(-nnz // groups)
    for g in range(groups):
        acc = np.zeros(n); bsum = np.float64(0.0)
        for t in range(g * per, min((g + 1) * per, nnz)):
            acc = acc + G[:, t].astype(np.float64) * a[t]
            bsum = bsum + b[t]
        out = out + (acc + bsum)
    return out


def _signed_limbs(vals, bits=26):
    """Python integers as rows of signed `bits`-bit limbs (int64): v = sum_l limb[l] 2^(bits l)."""
    L = max(1, max((abs(v).bit_length() for v in vals), default=1) // bits + 1)
    out = np.zeros((len(vals), L), dtype=np.int64)
    mask = (1 << bits) - 1
    for t, v in enumerate(vals):
        s, w = (-1 if v < 0 else 1), abs(v)
        for l in range(L):
            out[t, l] = s * ((w >> (bits * l)) & mask)
    return out


def _int_matvec(M, vals, bits=26):
    """M (rows x k, small non-negative integers) times the Python integers vals, exactly: a list of Python integers per row.  The
    limb columns go through an int64 matrix product (|entries| <= 2 k 2^26), the limbs are joined in Python integers."""
    limbs = _signed_limbs(vals, bits)
    part = np.asarray(M, dtype=np.int64) @ limbs
    acc = np.zeros(part.shape[0], dtype=object)
    for l in range(limbs.shape[1] - 1, -1, -1):
        acc = acc * (1 << bits) + part[:, l].astype(object)
    return acc


def xv_exact_misses(got, G, miss, mu, sinv, val, center, scale, impute, rows, clamp20=False):
    """Rows (of `rows`) where got_i is farther from the exact X beta than the a-priori forward bound allows.

        exact_i = sum_t (g_it - mu_t) sinv_t v_t      in rational arithmetic over the doubles mu, sinv, v
                  (no mu term without center, sinv = 1 without scale; a missing entry counts as mu_t with impute, else as dosage 0)
        |got_i - exact_i| <= (nnz + 20) 2^-53 S_i,    S_i = sum_t (g_it + |mu_t|) |sinv_t v_t|

    -- a chain of nnz multiply-adds and at most 16 group additions (which also cover the centring and fix-up terms); nothing of
    it is measured.  Everything is a dyadic rational, so the comparison itself is done in integers: no rounding on the checking
    side.  clamp20: got is compared with clip(exact, -20, 20) (clipping moves two numbers no farther apart).
    G (n x nnz) stored dosages in list order (0 where missing), miss (n x nnz) bool.  Returns [(row, got, exact as float, bound as float)]."""
    from fractions import Fraction
    rows = np.asarray(rows, dtype=np.int64)
    nnz = G.shape[1]
    if nnz == 0:
        return [(int(i), float(got[i]), 0.0, 0.0) for i in rows if got[i] != 0.0]
    W = [(Fraction(float(s)) if scale else Fraction(1)) * Fraction(float(v)) for s, v in zip(sinv, val)]
    Cm = [Fraction(float(m_)) * w for m_, w in zip(mu, W)]
    D = max(max(f.denominator for f in W), max(f.denominator for f in Cm))           # powers of two: the largest is the common one
    Wn = [int(f * D) for f in W]; Cn = [int(f * D) for f in Cm]
    Gr, Mr = np.asarray(G)[rows], np.asarray(miss)[rows]
    N = _int_matvec(Gr, Wn)
    if center:
        N = N - sum(Cn)
    if impute and Mr.any():
        N = N + _int_matvec(Mr, Cn)
    S = _int_matvec(Gr, [abs(v) for v in Wn]) + sum(abs(v) for v in Cn)
    bad = []
    for r, i in enumerate(rows):
        num = int(N[r])
        if clamp20:
            num = max(-20 * D, min(20 * D, num))
        gp, gq = float(got[i]).as_integer_ratio()
        if (abs(gp * D - num * gq) << 53) > (nnz + 20) * int(S[r]) * gq:
            bad.append((int(i), float(got[i]), num / D, (nnz + 20) * 2.0 ** -53 * (int(S[r]) / D)))
    return bad



# ---- the 16-bit dosage matrix: the standardized matrix, an edge-case matrix, exact X'r and X beta, the counted error bounds ----
def standardized(num, den, mu, sinv):
    miss = num == 0xFFFF
    return np.where(miss, 0.0, (num.astype(np.float64) / den - mu) * sinv)


def edge_matrix(n, den, seed):
    """Columns with mu near 0 and 2 (0-5), monomorphic at 0, 1 and 2 (6-8), all missing (9), monomorphic at 2 with sparse missing
    entries (10), and ordinary fractional ones with 5 % missing (11-19).  Any n >= 1; the off-pole values go up to 2 den."""
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(3):                                  # mu near 0 / near 2: one or two entries off the pole
        c = np.zeros(n, np.int64); c[rng.choice(n, min(2, n), replace=False)] = rng.integers(1, 2 * den + 1, min(2, n)); cols.append(c)
        c = np.full(n, 2 * den, np.int64); c[rng.choice(n, min(2, n), replace=False)] = rng.integers(0, 2 * den + 1, min(2, n)); cols.append(c)
    cols += [np.zeros(n, np.int64), np.full(n, den, np.int64), np.full(n, 2 * den, np.int64), np.full(n, -1, np.int64)]
    c = np.full(n, 2 * den, np.int64); c[::97] = -1; cols.append(c)                    # monomorphic at 2 with missing entries
    for _ in range(9):
        c = rng.integers(0, 2 * den + 1, n); c[rng.random(n) < 0.05] = -1; cols.append(c)
    num = np.stack(cols, axis=1)
    return np.where(num < 0, 0xFFFF, num).astype(np.uint16)


def _dyadic(r):
    """The doubles r_i as integers A_i over one power of two D: r_i = A_i / D exactly."""
    ratios = [float(v).as_integer_ratio() for v in r]
    D = max(q for _, q in ratios)
    return np.array([a * (D // q) for a, q in ratios], dtype=object), D


def exact_xtv(num, den, mu, sinv, r):
    """sinv_j * sum_i (num_ij / den - mu_j) r_i over the non-missing i, exactly (mu_j, sinv_j the handle's own values)."""
    from fractions import Fraction
    A, D = _dyadic(r)
    out = []
    for j in range(num.shape[1]):
        ok = num[:, j] != 0xFFFF
        s_num = int(np.dot(num[ok, j].astype(object), A[ok])) if ok.any() else 0
        s_r = int(A[ok].sum()) if ok.any() else 0
        out.append(Fraction(float(sinv[j])) * (Fraction(s_num, den * D) - Fraction(float(mu[j])) * Fraction(s_r, D)))
    return out


def exact_xv(num, den, mu, sinv, idx, val):
    """sum_t x_{i, idx[t]} val_t with x_ij = (num_ij / den - mu_j) sinv_j (0 where missing), exactly, for every row i."""
    from fractions import Fraction
    n = num.shape[0]
    if len(idx) == 0:
        return [Fraction(0)] * n
    w = [Fraction(float(sinv[j])) * Fraction(float(v)) for j, v in zip(idx, val)]           # sinv_j val_t: dyadic rationals
    m = [Fraction(float(mu[j])) * den for j in idx]                                         # mu_j den: the mean numerator
    Dw = max(f.denominator for f in w); Dm = max(f.denominator for f in m)
    a = np.array([int(f * Dw) for f in w], dtype=object)
    b = np.array([int(f * Dm) for f in m], dtype=object)
    sub = num[:, idx]
    C = np.where(sub == 0xFFFF, 0, sub.astype(object) * Dm - b[None, :])                   # (num - mu den) Dm, 0 where missing
    tot = C.dot(a)
    return [Fraction(int(t), den * Dw * Dm) for t in tot]


def dosage_host_stats(num, den):
    """mun_j = fl(S / N) and sc_j = fl(sinv_j / den) as k_dosage_stats forms them (S, N exact integers in a double; every
    operation a correctly rounded IEEE one on both sides), from the numerators alone."""
    ok = num != 0xFFFF
    S = np.where(ok, num, 0).astype(np.int64).sum(axis=0).astype(np.float64)
    N = ok.sum(axis=0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(N > 0, S / (N * float(den)), 0.0)
        s = np.sqrt(m * (1.0 - m / 2.0))
        sinv = np.where(s > 0, 1.0 / s, 1.0)
        mun = np.where(N > 0, S / N, 0.0)
    return mun, sinv / float(den), m, sinv


def dosage_xtv_tol(num, den, R):
    """The a-priori error bound of k_xtv_dosage_lds per column and residual (p x m), counted from its source; u = 2^-53,
    steps = ceil(n / 1024), c_ij = num_ij - mun_j (0 where missing):

        tol_j = 2u [ (4 steps + 12) sc_j sum_i |c_ij| |r_i|  +  2 sc_j mun_j sum_{i not missing} |r_i| ]

    4 steps + 12: one rounding in num - mun; a row's product joins one of 4 chains per lane, and a chain takes 2 (loads u) x 2
    (pairs hh) = 4 FMAs per 1024-row step; 2 additions join the 4 chains, 6 the 64 lanes (wave_sum), one multiply by sc, and
    sc = fl(sinv / den) is one more rounding: 4 steps + 11 by the source, which the 4 steps + 12 this bound was set with covers.
    The second term: the reference centres by the handle's mu_j = fl(S / (N den)), the kernel by mun_j = fl(S / N): two independent
    roundings of the
    same mean, each worth u mun_j on every non-missing row.  The leading 2 covers the second-order terms."""
    n = num.shape[0]
    mun, sc, _, _ = dosage_host_stats(num, den)
    ok = num != 0xFFFF
    c = np.where(ok, np.abs(num.astype(np.float64) - mun[None, :]), 0.0)
    aR = np.abs(np.asarray(R, dtype=np.float64).reshape(n, -1))
    steps = (n + 1023) // 1024
    return 2.0 * 2.0 ** -53 * ((4 * steps + 12) * sc[:, None] * (c.T @ aR) + 2.0 * (sc * mun)[:, None] * (ok.astype(np.float64).T @ aR))


def dosage_xv_tol(num, den, idx, val, groups=16):
    """The a-priori error bound of k_xv_dosage + k_xv_reduce per row: an entry x_ij = fl(fl(num - mun_j) sc_j) carries three
    roundings relative to |c_ij| sc_j (the subtraction, sc_j = fl(sinv_j / den), the product) and the two roundings of the mean
    (2u mun_j sc_j, as in dosage_xtv_tol); a term passes at most per = ceil(nnz / G) FMAs of its group's chain and G additions of
    the reduction, G = min(nnz, groups):

        tol_i = 2u sum_t |val_t| sc_j [ (per + G + 3) |c_ij| + 2 mun_j ],   j = idx[t], over the non-missing (i, j)."""
    nnz = len(idx)
    if nnz == 0:
        return np.zeros(num.shape[0])
    G = min(nnz, groups); per = -(-nnz // G)
    mun, sc, _, _ = dosage_host_stats(num, den)
    sub = num[:, idx]
    ok = sub != 0xFFFF
    c = np.where(ok, np.abs(sub.astype(np.float64) - mun[idx][None, :]), 0.0)
    w = np.abs(np.asarray(val, dtype=np.float64)) * sc[idx]
    return 2.0 * 2.0 ** -53 * ((per + G + 3) * (c @ w) + 2.0 * (ok.astype(np.float64) @ (w * mun[idx])))


# ---- the residual front end of X'r over the 2-bit matrix at its edges: the scale rule restated, the inputs, exact values and bounds ----
XTV_EBITS = {None: 53, 0: 53, 4910: 53, 4908: 42, 1316: 56, 1308: 26, 428: 53}      # DigitMode::ebits of csrc/xtv.hip's format table


def peel_threshold(r, ratio=64.0):
    """(tau, max|r|) of peel_rule's guard: tau = ratio x the ceil(B/4)-th smallest block maximum.  The guard fires iff max|r| > tau."""
    a = np.abs(np.asarray(r, dtype=np.float64))
    n = a.size
    nb = min(64, (n + 255) // 256)
    bmax = np.array([max(a[lo:lo + 256].max() for lo in range(256 * b, n, 16384)) for b in range(nb)])
    with np.errstate(over="ignore"):
        return float(ratio * np.sort(bmax)[(nb + 3) // 4 - 1]), float(bmax.max())


def xtv_quantum(r, digits=None):
    """The scale rule of the fixed-point residual restated (k_r_stats and the stats hook of k_digits, csrc/xtv_digits.hip): the quantum
    2^-e every entry that stays in the fixed point is rounded to, e = ebits - ilogb(top) capped at 1000 (0 for top = 0), top = max|r|
    over the rows peel_rule leaves in."""
    import math
    a = np.abs(np.asarray(r, dtype=np.float64)).copy()
    a[peel_rule(r)] = 0.0
    top = float(a.max())
    if not (top > 0.0 and math.isfinite(top)):
        return 1.0
    return math.ldexp(1.0, -min(XTV_EBITS[digits] - (math.frexp(top)[1] - 1), 1000))


def _codes(cols, n):
    """PLINK codes (p x n) of packed columns; _pack is the way back."""
    return np.stack([(cols >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(cols.shape[0], -1)[:, :n]


def _pack(code):
    p, n = code.shape
    pad = np.zeros((p, (n + 3) // 4 * 4), np.uint8)
    pad[:, :n] = code
    return (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)


class EdgeCase:
    """One residual of the edge suite: r, the rows the guard is MEANT to peel (ascending), and what the result is held to:
    "bound" (the derived bound), "bound_or_nan" (that, or NaN in every column) or "nan" (NaN in every column)."""
    def __init__(self, name, r, rows=(), expect="bound", fires=None):
        self.name, self.r, self.expect, self.fires = name, np.ascontiguousarray(r, dtype=np.float64), expect, fires
        self.rows = np.array(sorted(int(i) for i in rows), dtype=np.int64)


_EDGE_GROUPS = ("ragged", "zero_blocks", "limit", "where", "company", "scale", "huge")
_EDGE_P = {"ragged": 37, "zero_blocks": 41, "limit": 48, "where": 70, "company": 37, "scale": 33, "huge": 35}


def xtv_edge_problem(group, n):
    """THE inputs of tests/test_gpu_xtv_residual_edges.py and of its CPU companion (which shows that every residual is what its name
    says): (cols, cases) -- the packed PLINK columns of a p x n matrix (p = 33 .. 70: a ragged column group) and a list of EdgeCase.
    Deterministic in (group, n).  Block b of the guard holds rows 256 b + t + 16384 k; nb = min(64, ceil(n / 256)) blocks, the guard's
    quartile is the ceil(nb / 4)-th smallest block maximum.

      ragged       a: Gaussian with the last row 2^-20; b: Gaussian; c: every entry +-1; d: Gaussian clipped to 2.5 with ten rows at +-3
                   and the last row 2.75 / 64 -- where the last block is that single row and the quartile is the smallest maximum
                   (n = 257, 513, 769) tau = 2.75 and exactly the ten rows are peeled, anywhere else nothing is
      zero_blocks  z1 / z2: one / two whole blocks (and a single-row last block) zero, the rest Gaussian: tau = 0, more than 64 rows
                   above it; nz64 / nz10 / nz1: only 64 / 10 / 1 non-zero rows: tau = 0 and every one of them is peeled
      limit        lim64 / lim65: 64 / 65 rows 2^30 x the rest; tie: max|r| = 64 = 64 x the quartile exactly; tie_up: one ulp more
      where        one row 1e9 x the rest: the last row, row 0, a row on which a column has a missing genotype (2 % missing)
      company      23 residuals of the kinds above and plain Gaussians of several scales, one n
      scale        max|r| = 2^k and the double below it, positive and negative, k = -1022, -600, 0, 1, 600; only denormal entries
      huge         max|r| = 9.9e299, 1e300, 1e305, 2^1022 with every partial sum finite; two entries of 1.5e308 (sum r overflows)"""
    assert group in _EDGE_GROUPS
    rng = np.random.default_rng([20260 + _EDGE_GROUPS.index(group), n])
    p = _EDGE_P[group]
    nb = min(64, (n + 255) // 256)
    clean = (nb + 3) // 4                                  # this many blocks must stay ordinary for the quartile to be ordinary
    single_last = n < 16384 and n % 256 == 1 and n > 1
    maf = rng.uniform(0.05, 0.5, p)
    code = np.array([0, 2, 3], dtype=np.uint8)[rng.binomial(2, maf[:, None], size=(p, n))]
    if group in ("where", "company"):
        code[rng.random((p, n)) < 0.02] = 1
    cases = []

    def ragged(tag=""):
        a = rng.standard_normal(n); a[n - 1] = 2.0 ** -20
        b = rng.standard_normal(n)
        c = rng.choice([-1.0, 1.0], n)
        d = np.clip(rng.standard_normal(n), -2.5, 2.5)
        ten = np.sort(rng.choice(n - 1, min(10, n - 1), replace=False))
        d[ten] = 3.0 * rng.choice([-1.0, 1.0], ten.size)
        d[n - 1] = 2.75 / 64
        d_fires = single_last and nb <= 4
        return [EdgeCase(tag + "a", a, fires=bool(single_last and nb <= 4)), EdgeCase(tag + "b", b), EdgeCase(tag + "c", c, fires=False),
                EdgeCase(tag + "d", d, rows=ten if d_fires else (), fires=d_fires)]

    def zero_blocks(tag=""):
        assert single_last and nb >= 4
        out = []
        for name, blocks in (("z1", (1,)), ("z2", (0, 2))):
            r = rng.standard_normal(n)
            for b in blocks:
                r[256 * b:256 * (b + 1)] = 0.0
            r[n - 1] = 0.0                                  # the single-row last block: a whole block too
            out.append(EdgeCase(tag + name, r, fires=True))
        for cnt in (64, 10, 1):
            r = np.zeros(n)
            rows = np.sort(rng.choice(256 * (nb - clean), cnt, replace=False))      # the last `clean` blocks stay zero: tau = 0
            r[rows] = 1.0 if cnt == 1 else rng.standard_normal(cnt) + np.where(rng.random(cnt) < 0.5, -0.1, 0.1)
            assert np.count_nonzero(r) == cnt
            out.append(EdgeCase(f"{tag}nz{cnt}", r, rows=rows, fires=True))
        return out

    def limit(tag=""):
        base = rng.standard_normal(n)
        cand = np.flatnonzero(np.abs(base) > 0.05)
        cand = cand[cand >= 256 * clean]                    # the first `clean` blocks keep ordinary maxima
        rows = np.sort(rng.choice(cand, 65, replace=False))
        r64, r65 = base.copy(), base.copy()
        r64[rows[:64]] *= 2.0 ** 30
        r65[rows] *= 2.0 ** 30
        tie = np.clip(rng.standard_normal(n) / 8, -0.99, 0.99)
        tie[3:256 * nb:256] = rng.choice([-1.0, 1.0], len(tie[3:256 * nb:256]))       # every full block's maximum is exactly 1
        if n % 256 and n - 256 * (nb - 1) <= 3:
            tie[n - 1] = 1.0
        at = int(256 * clean + 77)
        up = tie.copy()
        tie[at], up[at] = -64.0, -np.nextafter(64.0, np.inf)
        return [EdgeCase(tag + "lim64", r64, rows=rows[:64], fires=True), EdgeCase(tag + "lim65", r65, fires=True),
                EdgeCase(tag + "tie", tie, fires=False), EdgeCase(tag + "tie_up", up, rows=[at], fires=True)], rows

    def where(tag=""):
        miss_rows = np.flatnonzero((code == 1).any(axis=0))
        mrow = int(miss_rows[miss_rows >= 300][0])
        out = []
        for name, row, val in (("last", n - 1, 1e9), ("first", 0, -3e8), ("missing", mrow, 2e9)):
            r = rng.standard_normal(n); r[row] = val
            out.append(EdgeCase(tag + name, r, rows=[row], fires=True))
        return out

    if group == "ragged":
        cases = ragged()
    elif group == "zero_blocks":
        cases = zero_blocks()
    elif group == "limit":
        cases, rows = limit()
        code[:8, rows] = 0                                  # columns 0 .. 7 carry none of the planted rows
    elif group == "where":
        cases = where()
    elif group == "company":
        lim, rows = limit("limit.")
        special = ragged("ragged.") + zero_blocks("zero.") + lim + where("where.")[:2]
        plain = [EdgeCase(f"gauss{t}", rng.standard_normal(n) * 10.0 ** s) for t, s in enumerate((0, -3, 5, 0, 100, -100, 1, 0))]
        assert len(special) == 15 and len(plain) == 8
        cases = [None] * 23
        for t, c in enumerate(special + plain):
            cases[(7 * t) % 23] = c                         # peeled and plain residuals interleaved over the two passes
    elif group == "scale":
        assert nb == 3 and single_last
        for k in (-1022, -600, 0, 1, 600):
            for vname, v in (("pow2", 2.0 ** k), ("below", float(np.nextafter(2.0 ** k, 0.0)))):
                for sign in (1.0, -1.0):
                    r = np.ldexp(np.clip(rng.standard_normal(n) / 4, -0.9, 0.9), k)
                    if sign > 0:
                        r[n - 1] = v                        # the single-row block holds the maximum: every block maximum >= max / 64
                    else:
                        r[100], r[n - 1] = -v, np.ldexp(0.5, k)
                    cases.append(EdgeCase(f"{vname}_k{k}_{'pos' if sign > 0 else 'neg'}", r, fires=False))
        r = rng.integers(-2 ** 20, 2 ** 20, n).astype(np.float64) * 2.0 ** -1074
        r[n - 1] = 2.0 ** 21 * 2.0 ** -1074
        cases.append(EdgeCase("denormal_only", r, fires=False))
    else:
        assert nb == 3 and single_last
        for name, T in (("9.9e299", 9.9e299), ("1e300", 1e300), ("1e305", 1e305)):
            r = T * np.clip(rng.standard_normal(n) / 4, -0.9, 0.9); r[n - 1] = T        # sum |r| < 513 x 0.9e305: no partial sum overflows
            cases.append(EdgeCase("max_" + name, r, expect="bound_or_nan", fires=False))
        r = 1e305 * np.clip(rng.standard_normal(n) / 4, -0.9, 0.9); r[100], r[n - 1] = -1e305, 0.5e305
        cases.append(EdgeCase("max_1e305_neg", r, expect="bound_or_nan", fires=False))
        T = 2.0 ** 1022                                                                   # the rest at 2^-10 T: sum |r| < 2 T < 2^1024
        r = np.ldexp(np.clip(rng.standard_normal(n) / 4, -0.9, 0.9), 1012); r[n - 1], r[5], r[300] = T, T / 32, -T / 32
        cases.append(EdgeCase("max_2p1022", r, expect="bound_or_nan", fires=False))       # (every block maximum >= T / 32: tau = 2 T)
        r = np.ldexp(np.clip(rng.standard_normal(n) / 4, -0.9, 0.9), 1012); r[100], r[n - 1] = T, np.ldexp(0.5, 1012)
        cases.append(EdgeCase("max_2p1022_outlier", r, rows=[100], expect="bound_or_nan", fires=True))
        r = rng.standard_normal(n); r[7] = r[300] = 1.5e308; r[n - 1] = 1.0             # (tau = 64: the two rows and no other)
        cases.append(EdgeCase("sum_overflows", r, rows=[7, 300], expect="nan", fires=True))
        code[:, [100, n - 1]] = np.minimum(code[:, [100, n - 1]], 2)      # dosage <= 1 on the rows of 2^1022: the exact X'r stays below 2^1024
    return _pack(code), cases


def xtv_edge_exact(cols, n, case, digits=None):
    """Exact X'r of the raw dosages (a missing entry counts as 0) against residual case.r, and the derived bounds, per column, as
    Fractions: (exact, B, ulp_sum) with
        B_j = (q / 2) sum_i g_ij [row i not peeled] + 8 x 2^-53 sum_i g_ij |r_i|,   q = xtv_quantum(r, digits),  ulp_sum_j = 2^-53 sum_i g_ij |r_i|
    -- the rounding of every entry of the fixed point to its quantum, and the f64 recombination at the 8 ulp-sums numpy's own sum is
    granted.  The sums are taken in integers (r_i = A_i / D with one power of two D)."""
    from fractions import Fraction
    g = _dosages(cols, n)
    A, D = _dyadic(case.r)
    N = _int_matvec(g, [int(v) for v in A])
    S = _int_matvec(g, [abs(int(v)) for v in A])
    inside = np.ones(n, dtype=np.int64)
    inside[case.rows] = 0
    cnt = g.astype(np.int64) @ inside
    q = Fraction(xtv_quantum(case.r, digits))
    exact = [Fraction(int(v), D) for v in N]
    ulp = [Fraction(int(v), D) / 2 ** 53 for v in S]
    return exact, [q / 2 * int(c) + 8 * u for c, u in zip(cnt, ulp)], ulp


# ---- the matrix side of X'r over the 2-bit matrix: the row slices and the pass plan restated, inputs, exact values, counted bounds ----
# DigitMode of csrc/xtv.hip's format table: (base, digits, residuals per operand, digit columns per residual)
XTV_MODES = {None: (49, 10, 3, 10), 0: (49, 10, 3, 10), 4910: (49, 10, 3, 10), 4908: (49, 8, 4, 8), 1316: (13, 16, 2, 16),
             1308: (13, 8, 4, 8), 428: (4, 28, 1, 32)}
XTV_KERNELS = tuple(f"k_xtv_dma16<{nr},2,8,{3 if nr == 6 else 4}{h}>" for nr in range(1, 7) for h in ("", ",half")) + \
    ("k_xtv_dma<1,2,4,8,fp4>", "k_xtv_mfma_lds<2,4,1,4,fp4>", "k_xtv_mfma_lds<3,2,2,8,fp4>", "k_xtv_mfma_lds<4,2,2,8,fp4>")


def xtv_slices(n, p):
    """auto_splits + row_slice of csrc/xtv.hip / xtv_kernels.h restated for n < 100000 rows: the number of 128-row blocks every row
    slice walks, one entry per slice (0: an empty trailing slice -- its workgroups run one masked-out step).  nbp = ceil(n / 128)
    blocks; the slice count s doubles while s < 16, ceil(ceil(p / 32) / 16) s < 2048 and nbp // (2 s) >= 8, and never exceeds nbp;
    a slice holds bps = ceil(nbp / s) blocks, the last ones what is left."""
    assert 1 <= n < 100000
    nbp = -(-n // 128)
    groups = (-(-p // 32) + 15) // 16
    s = 1
    while s < 16 and groups * s < 2048 and nbp // (2 * s) >= 8:
        s *= 2
    s = min(s, nbp)
    bps = -(-nbp // s)
    return [max(0, min(bps, nbp - k * bps)) for k in range(s)]


def xtv_plan(digits, m, max_flat_passes=16):
    """plan_passes + dispatch_xtv of csrc/xtv.hip restated at the release defaults (max_nr = 4, max_ops = 6, half = true): the passes
    that score m residuals in format `digits`, as [(residuals, operands, half, kernel name)] -- the name is the string dispatch_xtv
    leaves in the pass record.  The ten-digit format packs its digit columns flat (19 residuals in six operands) while that takes at
    most 16 passes (m <= 304), and goes back to three residuals per operand beyond."""
    base, ndig, per_op, slots = XTV_MODES[digits]
    lay16 = base == 49

    def name(nr, half):
        if lay16:
            return f"k_xtv_dma16<{nr},2,8,{3 if nr == 6 else 4}{',half' if half else ''}>"
        return {1: "k_xtv_dma<1,2,4,8,fp4>", 2: "k_xtv_mfma_lds<2,4,1,4,fp4>", 3: "k_xtv_mfma_lds<3,2,2,8,fp4>",
                4: "k_xtv_mfma_lds<4,2,2,8,fp4>"}[nr]
    out = []
    if lay16 and slots * per_op < 32:
        cap = (6 * 32) // slots
        npass = -(-m // cap)
        if npass <= max_flat_passes:
            for q in range(npass):
                cnt = m // npass + (1 if q < m % npass else 0)
                nr = (cnt * slots + 31) // 32
                half = cnt * slots - 32 * (nr - 1) <= 16
                out.append((cnt, nr, half, name(nr, half)))
            return out
    nops = -(-m // per_op)
    t = 0
    while t < nops:
        rem = nops - t
        if lay16:
            np_ = -(-rem // 6)
            nr = -(-rem // np_)
        else:
            nr = 4 if (rem >= 4 and rem != 5) else 3 if rem in (3, 5) else 2 if rem >= 2 else 1
        u1 = min((t + nr) * per_op, m)
        half = lay16 and (u1 - (t + nr - 1) * per_op) * slots <= 16
        out.append((u1 - t * per_op, nr, half, name(nr, half)))
        t += nr
    return out


def xtv_recombine_count(digits, splits):
    """C of the matrix-side bound: how many ulp-sums u sum_i g_ij |r_i| (u = 2^-53) the f64 recombination of the exact digit sums can
    cost, COUNTED from csrc/xtv_kernels.h (digit_weights, digit_sum / xtv_epilogue / xtv_epilogue16_flat, xtv_finalize_col).

    The f32 accumulators are exact: S_t = sum_i g_ij d_it per digit plane t and slice, R_i = sum_t d_it b^t the integer residual.
    Signed digits magnify: with |d| <= 2 (b - 1) / 3 in all three systems (32 / 48, 8 / 12, 2 / 3) the digits below the leading one
    T_i add up to at most (2/3) b^T_i, so |R_i| >= b^T_i / 3 and sum_t |d_it| b^t <= (5/3) b^T_i <= K |R_i| with K = 5.
      products  x_t = fl(S_t w_t): one rounding of a term of size <= sum_i g_ij |d_it| b^t  -> K ulp-sums over all t.  Base 4: w_t is a
                power of two, no rounding (0).  Base 13 with 16 digits: w_15 = 4 x 13^15 > 2^53 is itself rounded (2 K); every other
                weight (16 x 49^9, 4 x 13^7) is an integer below 2^53 times a power of two.
      additions ten columns: the chain sum = ((0 + x_0) + x_1) + ... + x_9, nine roundings.  The partial sum after digit k is
                sum_i g_ij (R_i mod-reduced to its digits <= k): |R_i| exactly for k >= T_i, at most (2/3) b^(k+1) <= 2 |R_i| b^(k+1-T_i)
                below.  Worst T_i = 2: 8 + 2 + 2 / 49 -> 10 ulp-sums (rounded down by less than the slack below).
                8 / 16 / 32 columns: the xor tree, log2(slots) levels; a level adds partial sums of arbitrary digit subsets, each
                bounded by the magnified size -> K log2(slots).
      scale     x 2^-e: exact.
      slices    dot = ((0 + p_0) + p_1) + ... : splits - 1 roundings of at most the whole sum (an empty slice adds +0 exactly).
      peeled    the compensated sum of the side channel: one rounding of the result and its own second-order term -> 2.
      slack     1: second-order terms (C u << 1) and sum g |R| 2^-e against sum g |r| (a relative 2^-54 per row).
    4910: 5 + 10 + splits + 2 = splits + 17;  4908: 5 + 15 + splits + 2;  1316: 10 + 20 + splits + 2;  1308: 5 + 15 + splits + 2;
    428: 0 + 25 + splits + 2.  (The 8 of xtv_edge_exact was set on the measured side of this count; it does not survive it.)"""
    base, ndig, per_op, slots = XTV_MODES[digits]
    K = 5
    products = 0 if base == 4 else 2 * K if (base, ndig) == (13, 16) else K
    additions = 10 if slots == 10 else K * {8: 3, 16: 4, 32: 5}[slots]
    return products + additions + (splits - 1) + 2 + 1


def xtv_matrix_cols(n, p, miss=0.02, seed=0, last_row_missing=False):
    """Packed PLINK columns (p x ceil(n / 4)) of the matrix-side tests: random genotypes with allele frequencies spread over
    0.02 .. 0.5 and a share `miss` of missing codes; where p >= 9 the first eight columns are structured -- 0: all 0, 1: all 2,
    2: a single 2 in row 0, 3: a single 1 in row n - 1, 4: non-zero only in the last (ragged) 128-row block, 5: non-zero only in rows
    63, 64, 127, 128 (where they exist), 6: non-zero only in the last row of each row slice and the first of the next, 7: every
    entry missing.  last_row_missing (p >= 10): column 8 has its only missing entry in row n - 1."""
    rng = np.random.default_rng([20270, n, p, int(round(miss * 1000)), seed])
    maf = rng.uniform(0.02, 0.5, p)
    code = np.array([0, 2, 3], dtype=np.uint8)[rng.binomial(2, maf[:, None], size=(p, n))]
    code[rng.random((p, n)) < miss] = 1
    if p >= 9:
        full = np.array([0, 2, 3], dtype=np.uint8)[rng.integers(1, 3, size=(8, n))]        # dosages 1 and 2 everywhere
        code[:8] = 0
        code[1] = 3
        code[2, 0] = 3
        code[3, n - 1] = 2
        lo = 128 * ((n - 1) // 128)
        code[4, lo:] = full[4, lo:]
        rows = [i for i in (63, 64, 127, 128) if i < n]
        code[5, rows] = full[5, rows]
        bps = max(xtv_slices(n, p))
        edge = [i for s in range(1, len(xtv_slices(n, p))) for i in (128 * bps * s - 1, 128 * bps * s) if i < n]
        code[6, edge] = full[6, edge]
        code[7] = 1
    if last_row_missing:
        assert p >= 10
        code[8][code[8] == 1] = 0
        code[8, n - 1] = 1
    return _pack(code)


def xtv_matrix_residuals(n, p, count=19):
    """The residuals of the matrix-side tests for an n x p matrix, as EdgeCase (rows = what peel_rule peels: small n makes the guard
    fire on ordinary residuals, and a unit vector rides the side channel as soon as n > 256 gives the guard a second block): unit vectors c e_i on rows 0, n - 1, 63, 64, 127,
    128 and the slice boundaries 128 bps s - 1, 128 bps s (first, middle and last boundary), the constant 1, and Gaussian columns with
    per-column scale exp(U(-3, 3)) -- dealt out so that every prefix of the list mixes the kinds: positions 0, 3, 5, 7, ... are
    Gaussian, 1 is the constant, 2, 4, 6, ... the unit vectors while they last.  Deterministic in (n, p, count's prefix)."""
    rng = np.random.default_rng([20271, n, p])
    sl = xtv_slices(n, p)
    bps = max(sl)
    bnd = sorted({s for s in (1, len(sl) // 2, len(sl) - 1) if 1 <= s < len(sl)})
    rows = [0, n - 1, 63, 64, 127, 128] + [i for s in bnd for i in (128 * bps * s - 1, 128 * bps * s)]
    rows = [i for k, i in enumerate(rows) if 0 <= i < n and i not in rows[:k]]
    out = []
    while len(out) < count:
        t = len(out)
        if t == 1:
            kind, r = "one", np.ones(n)
        elif t >= 2 and t % 2 == 0 and rows:
            i = rows.pop(0)
            kind, r = f"unit{i}", np.zeros(n)
            r[i] = float(np.exp(rng.uniform(-3, 3)) * rng.choice([-1.0, 1.0]))
        else:
            kind, r = f"gauss{t}", rng.standard_normal(n) * np.exp(rng.uniform(-3, 3))
        out.append(EdgeCase(kind, r, rows=peel_rule(r)))
    return out


def xtv_matrix_exact(cols, n, case, splits):
    """Exact X'r of the raw dosages against case.r (xtv_edge_exact, computed once) and, for every format, the bound
        B_j = (q / 2) sum_i g_ij [row i not peeled] + C x 2^-53 sum_i g_ij |r_i|,  q = xtv_quantum(r, format), C = xtv_recombine_count(format, splits):
    (exact, {format: bounds}, ulp_sum), Fractions per column."""
    from fractions import Fraction
    exact, b8, ulp = xtv_edge_exact(cols, n, case, 428)
    q53 = Fraction(xtv_quantum(case.r, 428))
    cnt = [(b - 8 * u) / (q53 / 2) for b, u in zip(b8, ulp)]                      # sum_i g_ij [row i not peeled], an integer
    assert all(c.denominator == 1 for c in cnt)
    bounds = {}
    for dg in (None, 4908, 1316, 1308, 428):
        q, C = Fraction(xtv_quantum(case.r, dg)), xtv_recombine_count(dg, splits)
        bounds[dg] = [q / 2 * c + C * u for c, u in zip(cnt, ulp)]
    return exact, bounds, ulp


def xtv_std_exact(cols, n, case, mu, sinv, center, scale, impute, raw, w_stats=None):
    """The exact value of the standardized X'r and its counted bound per column, from `raw` = xtv_matrix_exact(cols, n, case, splits):
        exact_j = sinv_j (sum_i g_ij r_i + [impute] mu_j sum_{i missing in j} r_i - [center] mu_j sum_i r_i)
    in rationals over the handle's own doubles mu_j, sinv_j (mu_sigma(); sinv_j = 1 without scale); a missing entry is stored as
    dosage 0.  Returns (exact, {format: bounds}); exact_j is None where the reference itself has no value: a column with every entry
    missing has mu = 0 / 0 = NaN, and with centring or imputation that NaN reaches the result (as in the reference's mean over no
    observation) -- the result must then be NaN.

    bound_j = |sinv_j| (B_j + u [ (k_j - 1) M_j + (w + 70) S_j + 6 (D_j + M_j + S_j) ]),  u = 2^-53, counted from xtv_finalize_col and k_r_stats:
      D_j = sum_i g_ij |r_i|;  M_j = [impute] |mu_j| sum_{i missing in j} |r_i|;  S_j = [center] |mu_j| sum_i |r_i|;
      (k_j - 1) M_j   the fix-up `ms += ru[miss_row[t]]` over the k_j missing rows: a plain chain, k_j - 1 roundings (0 + x is exact);
      (w + 70) S_j    sum_r of k_r_stats: the thread's walk over w = ceil(n / 16384) rows (w - 1 roundings), 8 tree levels, the chain over
                      64 block partials (63): w + 70;
      6 (D + M + S)   dot += mu ms (product, sum), dot -= mu sum_r (product, difference), dot *= sinv: 5 roundings of at most the
                      whole magnitude, and 1 for the second-order terms."""
    from fractions import Fraction
    exact_raw, bounds_raw, ulp = raw
    p = cols.shape[0]
    missing = (_codes(cols, n) == 1).astype(np.int64)
    A, D = _dyadic(case.r)
    Ai = [int(v) for v in A]
    absA = [abs(v) for v in Ai]
    msum = _int_matvec(missing, Ai); mabs = _int_matvec(missing, absA)
    kmiss = missing.sum(axis=1)
    sum_r, sum_abs = Fraction(sum(Ai), D), Fraction(sum(absA), D)
    w = -(-n // 16384)
    u = Fraction(1, 2 ** 53)
    exact, bounds = [], {dg: [] for dg in bounds_raw}
    for j in range(p):
        nan = bool(np.isnan(mu[j])) and (center or (impute and kmiss[j] > 0))
        m = Fraction(0) if np.isnan(mu[j]) else Fraction(float(mu[j]))
        si = Fraction(float(sinv[j])) if scale else Fraction(1)
        Mj = abs(m) * Fraction(int(mabs[j]), D) if impute else Fraction(0)
        Sj = abs(m) * sum_abs if center else Fraction(0)
        Dj = ulp[j] * 2 ** 53
        val = exact_raw[j] + (m * Fraction(int(msum[j]), D) if impute else 0) - (m * sum_r if center else 0)
        exact.append(None if nan else si * val)
        tail = u * (max(int(kmiss[j]) - 1, 0) * Mj + (w + 70) * Sj + 6 * (Dj + Mj + Sj))
        for dg in bounds:
            bounds[dg].append(abs(si) * (bounds_raw[dg][j] + tail))
    return exact, bounds


def snp_host_stats(cols, n):
    """mu_j and sinv_j as k_col_stats (csrc/snp.hip) forms them from the genotype counts: every operation a correctly rounded IEEE
    one on both sides.  A column with every entry missing: mu = 0 / 0 = NaN, sinv = 1."""
    code = _codes(cols, n)
    n1, n2, nm = (code == 2).sum(axis=1).astype(np.float64), (code == 3).sum(axis=1).astype(np.float64), (code == 1).sum(axis=1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (n1 + 2.0 * n2) / (float(n) - nm)
        s = np.sqrt(m * (1.0 - m / 2.0))
        sinv = np.where(s > 0.0, 1.0 / s, 1.0)
    return m, sinv


# the cases of tests/test_gpu_xtv_matrix_edges.py (and of its CPU companion, which shows that the inputs are what their names say)
XTV_ROW_N = (1, 3, 64, 127, 128, 129, 255, 384, 385, 512, 513, 640, 1024, 1025, 1152, 1920, 2048, 2049, 4095, 4225, 8321, 16400, 28800, 28801)
XTV_RUNS = ((None, 1), (None, 19), (428, 1), (1316, 4), (1316, 6), (1316, 8), (4908, 5))        # (format, residuals in the call)
XTV_COL_N = (385, 2049)
XTV_COL_P = (1, 31, 32, 33, 64, 65, 255, 256, 257, 511, 512, 513, 545, 1025)
XTV_PLAN_SHAPES = ((385, 70), (2049, 65))
XTV_PLAN_M = {None: list(range(1, 20)) + [20, 38, 39, 304, 305, 307], 4908: [1, 3, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25],
              1316: list(range(1, 15)) + [18], 428: list(range(1, 10)), 1308: [1, 4, 5, 16, 17]}
XTV_FLAGS = ((1, 1, 1), (1, 1, 0), (0, 0, 1), (1, 0, 1))
XTV_FLAG_SHAPES = ((129, 33), (2049, 65), (16400, 70))
XTV_FLAG_MISS = (0.02, 0.3)
XTV_FLAG_RUNS = ((None, 3), (428, 1))


def xtv_run_calls(m, flags=False):
    """The residuals (positions in xtv_matrix_residuals' list) of the calls a run of m residuals makes: the first m in one call; a run
    of one makes three calls -- a Gaussian, the constant 1 and the unit vector on row n - 1 (position 4).  flags: the standardized
    runs take the Gaussians and the constant (positions 0, 1, 3)."""
    if flags:
        return [[0, 1, 3]] if m == 3 else [[0], [1], [3]]
    return [[0], [1], [4]] if m == 1 else [list(range(m))]


class XtvMatrixProblem:
    """One matrix of the matrix-side tests with its residuals; exact values and bounds are computed once per residual."""
    def __init__(self, n, p, miss=0.02, count=19, last_row_missing=False):
        self.n, self.p, self.miss = n, p, miss
        self.cols = xtv_matrix_cols(n, p, miss, last_row_missing=last_row_missing)
        self.cases = xtv_matrix_residuals(n, p, count)
        self.slices = xtv_slices(n, p)
        self.R = np.asfortranarray(np.stack([c.r for c in self.cases], axis=1))
        self._raw, self._std = {}, {}

    def raw(self, t):
        if t not in self._raw:
            self._raw[t] = xtv_matrix_exact(self.cols, self.n, self.cases[t], len(self.slices))
        return self._raw[t]

    def std(self, t, mu, sinv, flags):
        if (t, flags) not in self._std:
            self._std[(t, flags)] = xtv_std_exact(self.cols, self.n, self.cases[t], mu, sinv, *flags, self.raw(t))
        return self._std[(t, flags)]


_XTV_PROBLEMS = {}


def xtv_matrix_problem(n, p, miss=0.02, count=19, last_row_missing=False):
    key = (n, p, miss, count, last_row_missing)
    if key not in _XTV_PROBLEMS:
        _XTV_PROBLEMS[key] = XtvMatrixProblem(*key)
    return _XTV_PROBLEMS[key]


# ---- project_k! at its buffer edges: the constants read from the sources, the list rules and the 22-bit prefix restated, the inputs ----
_SELECT_PATTERNS = {
    "topk.hip": {
        "finish_cap": r"constexpr int kFinishCap = (\d+);",
        "finish_bin": r"constexpr int kFinishBin = (\d+);",
        "expect_pad": r"w\.expect = max_keep \+ (\d+);",
        "cap_pad": r"w\.cap = max_keep \+ (\d+);",
        "hist_blocks": r"gridh = \(int\)std::min<int64_t>\(\(len \+ 255\) / 256, (\d+)\)",
        "sweep_blocks": r"gridh = [^;]*?, grid = \(int\)std::min<int64_t>\(\(len \+ 255\) / 256, (\d+)\);",
        "radix_blocks": r"int grid = \(int\)std::min<int64_t>\(\(len \+ 255\) / 256, (\d+)\);\s*// <= 512 blocks",
    },
    "resident.inc": {
        "collect_slots": r"constexpr int kResCollectSlots = (\d+);",
        "collect_blocks": r"constexpr int kResCollectBlocks = (\d+);",
        "grad_blocks": r"constexpr int kResGradBlocks = (\d+);",
        "res_hist_blocks": r"constexpr int kResHistBlocks = (\d+);",
        "max_in_bin": r"constexpr int kResMaxInBin = (\d+);",
        "max_list": r"constexpr int kResMaxList = (\d+);",
        "big_list": r"constexpr int kResBigList = (\d+);",
        "spread_strides": r"const bool spread = len < (\d+) \* stride;",
        "support_list": r"__shared__ int64_t lst_idx\[(\d+)\];",
        "support_scan": r"if \(nl <= (\d+)\) \{ for \(int e = 0; e < nl; \+\+e\)",
    },
    "iht_var.hip": {         # a FIT sizes its stand-alone select with kcap, not with k: topk_work_init(topk, kcap)
        "fit_kcap_floor": r"int64_t kcap = std::max<int64_t>\(std::max<int64_t>\(J, 1\) \* k \+ q, (\d+)\) \+ \d+;",
        "fit_kcap_pad": r"int64_t kcap = std::max<int64_t>\(std::max<int64_t>\(J, 1\) \* k \+ q, \d+\) \+ (\d+);",
        "fit_topk_by_kcap": r"MIH_TRY\(topk_work_init\(topk, kcap\)\);()",
    },
}
_SELECT_CONSTANTS = {}


def select_constants():
    """The sizes the select's cases are built around, read from csrc/topk.hip and csrc/resident.inc (the cases follow the code); a
    pattern that no longer matches exactly once is an AssertionError naming it."""
    if not _SELECT_CONSTANTS:
        _SELECT_CONSTANTS.update(_constants_from_sources(_SELECT_PATTERNS))
    return dict(_SELECT_CONSTANTS)


def _constants_from_sources(patterns):
    """{name: int} of {file under csrc/: {name: pattern with one group}}; every pattern must match its file exactly once."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mendeliht.jl_amd", "csrc")
    out = {}
    for fname, pats in patterns.items():
        with open(os.path.join(root, fname)) as f:
            text = f.read()
        for name, pat in pats.items():
            found = re.findall(pat, text)
            assert len(found) == 1, f"{fname}: the pattern of {name} ({pat!r}) matches {len(found)} times, not once"
            out[name] = int(found[0] or 1)
    return out


def res_list_of(j, length, mode):
    """Which of the per-block candidate lists of the resident select entry j of a vector of `length` = p + q entries lands in.
    mode "direct": the gather of k_res_grad<true> -- block b owns the contiguous range [b chunk, (b + 1) chunk), chunk =
    ceil(length / blocks); mode "collect": k_res_collect -- a vector shorter than 4 strides (stride = 256 blocks) is dealt out
    entry by entry, j mod blocks; a longer one in runs of 256, (j // 256) mod blocks."""
    C = select_constants()
    assert C["collect_blocks"] == C["grad_blocks"]
    B = C["collect_blocks"]
    j = np.asarray(j, dtype=np.int64)
    if mode == "direct":
        return j // (-(-int(length) // B))
    assert mode == "collect"
    return j % B if length < C["spread_strides"] * B * 256 else (j // 256) % B


def abs_key(x):
    """The IEEE-754 bit pattern of |x| (monotone in |x|; -0.0 -> 0)."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)


def prefix22(x):
    """Exponent and the top 11 mantissa bits of |x|: what two 11-bit histogram sweeps pin the threshold down to."""
    return abs_key(x) >> np.uint64(41)


def fit_select_caps(k, q, J=1):
    """(expect, cap) of the stand-alone select INSIDE a fit (the host-driven step, the replay of a step the device handed back):
    IhtVar sizes it with kcap = max(J k + q, 64) + 1024, so the landing buffer holds kcap + 64 pairs and the gather buffer
    kcap + 1024 -- not k + 64 and k + 1024 as in mih.project_k."""
    C = select_constants()
    kcap = max(max(J, 1) * k + q, C["fit_kcap_floor"]) + C["fit_kcap_pad"]
    return kcap + C["expect_pad"], kcap + C["cap_pad"]


def tied_fit_route(copies, k=2, q=1):
    """The way the stand-alone select takes inside the tied fits (k = 2, the intercept kept: K = 3) when every projection ties
    copies + 1 entries at the threshold, above them only the intercept's +Inf: gathered = copies + 2 = survivors.  "host": within
    the fit's gather buffer but more sharers than kFinishBin -- nth_element on the host, with the second copy when the landing
    buffer is exceeded; "radix": beyond the gather buffer -- the 8 x 8-bit select, and compact_device grows its buffer."""
    C = select_constants()
    expect, cap = fit_select_caps(k, q)
    tied, gathered = copies + 1, copies + 2
    assert tied > C["finish_bin"]
    return dict(route="radix" if gathered > cap else "host", fetch=gathered > expect, grow=gathered > cap, cap=cap, expect=expect)


def select_counts(v, k, radix8=False):
    """What the stand-alone select meets on vector v at sparsity k (csrc/topk.hip restated in counts): the entries above the
    22-bit prefix of the k-th largest magnitude (A), the non-zero entries sharing it (S), the gathered count A + S (zeros are
    not gathered), the survivors (|x| >= the k-th largest, ties kept, zeros excluded), and the way they take:
      route  "device": gathered <= min(cap, kFinishCap) and S <= kFinishBin -- k_topk_finish; "host": gathered <= cap otherwise
             -- nth_element on the host; "radix": gathered > cap = k + 1024 (or the switch MENDELIHT_TOPK_RADIX8) -- 8 x 8 bits
      fetch  the landing buffer of k + 64 pairs (kFinishCap at most for the device finish) does not hold what comes home (the
             survivors; the candidates for the host finish): a second copy fetches the rest
      grow   radix only: more survivors than cap -- compact_device grows its buffer and runs again."""
    C = select_constants()
    v = np.ascontiguousarray(v, dtype=np.float64)
    keys = abs_key(v)
    nz = v != 0.0
    kth = np.partition(keys, keys.size - k)[keys.size - k]
    pre = kth >> np.uint64(41)
    top = keys >> np.uint64(41)
    A = int(np.count_nonzero(top > pre))
    S = int(np.count_nonzero((top == pre) & nz))
    surv = int(np.count_nonzero((keys >= kth) & nz))
    cap, expect = k + C["cap_pad"], k + C["expect_pad"]
    gathered = A + S
    if radix8 or gathered > cap:
        route, fetch, grow = "radix", surv > min(expect, cap), surv > cap
    elif gathered <= C["finish_cap"] and S <= C["finish_bin"]:
        route, fetch, grow = "device", surv > min(expect, cap, C["finish_cap"]), False
    else:
        route, fetch, grow = "host", gathered > min(expect, cap), False
    return dict(A=A, S=S, gathered=gathered, survivors=surv, rem=k - A, route=route, fetch=fetch, grow=grow, cap=cap, expect=expect)


def sweep_handover(length):
    """(last index the 4-way unrolled loop of k_hist11 reads, first index its tail reads) for a vector of `length`; None where a
    part is empty.  blocks = min(ceil(length / 256), 512), stride = 256 blocks; thread g runs the unrolled body while
    i + 3 stride < length from i = g in steps of 4 stride, then the tail in steps of stride."""
    blocks = min(-(-length // 256), select_constants()["hist_blocks"])
    stride = 256 * blocks
    i = np.arange(length, dtype=np.int64)
    g = i % stride
    left = length - 1 - g - 3 * stride
    n_unr = np.where(left >= 0, left // (4 * stride) + 1, 0)
    unrolled = (i // stride) < 4 * n_unr
    return (int(i[unrolled].max()) if unrolled.any() else None, int(i[~unrolled].min()) if (~unrolled).any() else None)


class ProjectCase:
    """One vector of the stand-alone select's edge cases: v, k and `want`, the entries of select_counts(v, k) its name promises."""
    def __init__(self, name, v, k, **want):
        self.name, self.v, self.k, self.want = name, np.ascontiguousarray(v, dtype=np.float64), int(k), want


_PROJECT_CASES = []
PROJECT_LENGTHS = (255, 256, 257, 512 * 256 - 1, 512 * 256, 512 * 256 + 1, 4 * 512 * 256 - 1, 4 * 512 * 256, 4 * 512 * 256 + 1)


def project_cases():
    """THE inputs of the stand-alone half of tests/test_gpu_select_edges.py (and of its CPU companion, which shows that every vector
    sits where its name says).  Sharers of one 22-bit prefix are 1.0 + j 2^-52: distinct keys under the prefix of 1.0; entries
    above them lie in [2, 1000), noise below in (0, 0.9); signs are mixed and the positions shuffled.  No NaN anywhere."""
    if _PROJECT_CASES:
        return list(_PROJECT_CASES)
    C = select_constants()
    FB, FC, EXP, CAP = C["finish_bin"], C["finish_cap"], C["expect_pad"], C["cap_pad"]
    u = 2.0 ** -52
    out = []

    def build(tag, above, sharers, noise):
        rng = np.random.default_rng([20280, *[ord(c) for c in tag]])
        big = rng.uniform(2.0, 1000.0, above)
        low = rng.uniform(1e-3, 0.9, noise)
        v = np.concatenate([big, np.asarray(sharers, dtype=np.float64), low])
        v *= rng.choice([-1.0, 1.0], v.size)
        return rng.permutation(v)

    # the sharers of the threshold's prefix against kFinishBin; k at the largest sharer, in their middle, at the smallest
    for S in (FB - 1, FB, FB + 1):
        for where, rank in (("largest", 1), ("middle", S // 2), ("smallest", S)):
            v = build(f"sharers{S}{where}", 10, 1.0 + u * np.arange(S), 3000 - 10 - S)
            out.append(ProjectCase(f"sharers S={S} k at the {where}", v, 10 + rank, A=10, S=S, gathered=10 + S, survivors=10 + rank,
                                   rem=rank, route="device" if S <= FB else "host", fetch=S > FB and S > rank + EXP))
    # the gathered candidates against kFinishCap, few sharers, cap = k + 1024 far away
    for G in (FC - 1, FC, FC + 1):
        k, S = FC - 46, G - (FC - 56)
        v = build(f"candidates{G}", G - S, 1.0 + u * np.arange(S), 6000 - G)
        out.append(ProjectCase(f"candidates A+S={G}", v, k, A=G - S, S=S, gathered=G, survivors=k, rem=10,
                               route="device" if G <= FC else "host", fetch=G > k + EXP))
    # t copies of the k-th magnitude: k - 1 + t survivors against the landing buffer of k + 64 pairs.  device: the ties are the
    # only sharers; host: kFinishBin - 24 more sharers above them push the pool beyond kFinishBin, so the candidates come home
    for t in (EXP, EXP + 1, EXP + 2):
        v = build(f"ties_dev{t}", 49, np.full(t, 1.0), 3000 - 49 - t)
        out.append(ProjectCase(f"threshold ties t={t}, device finish", v, 50, A=49, S=t, gathered=49 + t, survivors=49 + t, rem=1,
                               route="device", fetch=t > EXP + 1))
        more = FB - 24
        v = build(f"ties_host{t}", 10, np.concatenate([1.0 + u * np.arange(1, more + 1), np.full(t, 1.0)]), 3000 - 10 - more - t)
        k = 10 + more + 1
        out.append(ProjectCase(f"threshold ties t={t}, host finish", v, k, A=10, S=more + t, gathered=k - 1 + t, survivors=k - 1 + t,
                               rem=more + 1, route="host", fetch=t > EXP + 1))
    # t copies against the gather buffer cap = k + 1024: beyond it the radix select runs and compact_device grows its buffer
    for t in (CAP, CAP + 1, CAP + 2):
        v = build(f"ties_cap{t}", 2, np.full(t, 1.0), 3000 - 2 - t)
        over = 2 + t > 3 + CAP
        out.append(ProjectCase(f"gather ties t={t}", v, 3, A=2, S=t, gathered=2 + t, survivors=2 + t, rem=1,
                               route="radix" if over else "device" if t <= FB else "host", fetch=True, grow=over))
    # degenerate inputs
    rng = np.random.default_rng(20281)
    for nnz in (99, 1, 0):
        v = np.zeros(3000)
        v[1::2] = -0.0
        v[rng.choice(3000, nnz, replace=False)] = rng.standard_normal(nnz) + 3.0
        out.append(ProjectCase(f"{nnz} non-zeros, k=100", v, 100, survivors=nnz, gathered=nnz, A=nnz, S=0, route="device"))
    v = rng.standard_normal(3000)
    out.append(ProjectCase("k = len", v, 3000, survivors=3000, gathered=3000, route="device"))
    out.append(ProjectCase("len = 1", np.array([-0.75]), 1, survivors=1, gathered=1, A=0, S=1, route="device"))
    out.append(ProjectCase("len = 1, zero", np.array([-0.0]), 1, survivors=0, gathered=0))
    eq = 2.5 * rng.choice([-1.0, 1.0], 3000)
    out.append(ProjectCase("all equal, k=7", eq, 7, A=0, S=3000, survivors=3000, route="radix", fetch=True, grow=True))
    out.append(ProjectCase("all equal, k=len", eq, 3000, A=0, S=3000, survivors=3000, route="host", fetch=False))
    for bits, route in ((52, "device"), (30, "radix")):      # exponent bin 0 throughout; below 2^-1044 all 3000 share ONE 22-bit prefix
        den = rng.integers(1, 2 ** bits, 3000).astype(np.float64) * rng.choice([-1.0, 1.0], 3000) * 2.0 ** -1074
        assert int(prefix22(den).max()) < 2048
        out.append(ProjectCase(f"denormals only, below 2^{bits - 1074}", den, 50, route=route, grow=False, **(dict(S=3000) if bits == 30 else {})))
    inf = rng.standard_normal(3000) * 1e300
    inf[rng.choice(3000, 40, replace=False)] = np.repeat([np.inf, -np.inf], 20)
    out.append(ProjectCase("40 infinities, k=25", inf, 25, A=0, S=40, survivors=40, route="device", fetch=False))
    big = rng.standard_normal(3000) * 1e300
    pos = rng.choice(3000, 20, replace=False)
    big[pos[:10]] = np.repeat([np.inf, -np.inf], 5)
    big[pos[10:]] = np.finfo(np.float64).max * np.repeat([1.0, -1.0], 5)
    for k, surv in ((10, 10), (11, 20), (15, 20), (20, 20), (21, 21)):
        out.append(ProjectCase(f"largest finite next to infinities, k={k}", big, k, survivors=surv, route="device"))
    # lengths around the sweeps' geometry; the k-th and the (k + 1)-th largest (3 + 4 ulp and 3: one prefix, so the exact finish
    # tells them apart) at the ends of the vector and on either side of the unrolled loop's hand-over to its tail
    for L in PROJECT_LENGTHS:
        last_unrolled, first_tail = sweep_handover(L)
        spots = [(0, L - 1), (L - 1, 0)]
        if last_unrolled is not None and first_tail is not None:
            spots += [(last_unrolled, first_tail), (first_tail, last_unrolled)]
        else:
            spots += [(L // 2, L // 2 + 1), (L // 2 + 1, L // 2)]
        base = np.random.default_rng([20282, L]).uniform(-0.9, 0.9, L)
        for a, b in spots:
            k = 37
            v = base.copy()
            free = np.setdiff1d(np.array([1, L // 3, L // 2 - 1, L - 2] + list(range(2, 200, 6))), [a, b])[:k - 1]
            v[free] = np.linspace(4.0, 8.0, k - 1) * np.where(np.arange(k - 1) % 2, -1.0, 1.0)
            v[a], v[b] = -(3.0 + 4 * 2.0 ** -51), 3.0
            out.append(ProjectCase(f"len={L}, k-th at {a}, next at {b}", v, k, A=k - 1, S=2, gathered=k + 1, survivors=k, rem=1, route="device"))
    _PROJECT_CASES.extend(out)
    return list(out)


# ---- the resident select inside fits: problems whose supports fill or overflow its lists ----
_SELECT_BEDS = {}
SELECT_FIT_N = 2000
SELECT_LAYOUTS = {                       # name: (p, planted columns, k, max_iter)
    "A": (41 * 512, tuple(5 + 512 * m for m in range(40)), 45, 8),
    "B": (51200, tuple(range(10000, 10070)), 80, 8),
    "B_exact64": (51200, tuple(range(10000, 10064)), 80, 8),
    "B_exact65": (51200, tuple(range(10000, 10065)), 80, 8),
}


def planted_response(cols, n, planted, rng):
    """y = X_S (+-1) + 0.5 + N(0, 1) over the standardized dosages of the planted columns (no missing entries)."""
    g = _dosages(cols[np.asarray(planted)], n).astype(np.float64)
    xs = (g - g.mean(axis=1, keepdims=True)) / g.std(axis=1, keepdims=True)
    return rng.choice([-1.0, 1.0], len(planted)) @ xs + 0.5 + rng.standard_normal(n)


def select_fit_problem(layout):
    """(cols, y, planted, k, max_iter) of layouts A and B (SELECT_LAYOUTS): make_bed(default_rng(7), 2000, p, maf_lo=0.2), no
    covariates beyond the intercept, so the projection selects among p + 1 entries.
      A        40 effects at 5 + 512 m: j mod 512 = 5 for all -- ONE list of k_res_collect's spread rule takes 40 > 32 entries;
               the contiguous ranges of the direct gather (42 entries) hold one each
      B        70 effects at 10000 .. 10069: one contiguous range (9999 .. 10099) holds them all -- the direct gather's list
               overflows and k_res_grad's support list (64) with it, so the binary-search branch runs; j mod 512 are distinct
      B_exact  64 / 65 effects there: the last linear scan, the first binary search."""
    from conftest import make_bed
    p, planted, k, max_iter = SELECT_LAYOUTS[layout]
    n = SELECT_FIT_N
    if p not in _SELECT_BEDS:
        _SELECT_BEDS[p] = make_bed(np.random.default_rng(7), n, p, maf_lo=0.2)
    cols = _SELECT_BEDS[p]
    y = planted_response(cols, n, planted, np.random.default_rng([7, len(planted)]))
    return cols, y, np.asarray(planted), k, max_iter


def select_tied_copies(copies):
    """The positions tied_case copies SNP 300 to: `copies` consecutive positions from 400."""
    return tuple(range(400, 400 + copies))


def tied_copy_counts():
    """The massive-tie fits: 2047 copies (2048 tied entries fill the resident pool exactly), 2100 (they overflow it), and as many
    copies as the FIT's gather buffer holds pairs (fit_select_caps: 2112), so that the tied entries alone exceed it and the
    host-driven replay runs the radix select inside a fit."""
    return (2047, 2100, fit_select_caps(2, 1)[1])


def clear_cut_backtracks(traces):
    """How many leading entries the backtrack traces of the oracle on the input as given and under the nudges have in common: the
    part of the trace that is not decided between loglikelihoods equal to rounding."""
    traces = [list(map(int, t)) for t in traces]
    n = 0
    while all(len(t) > n for t in traces) and len({t[n] for t in traces}) == 1:
        n += 1
    return n


TINY_N, TINY_SEED, TINY_MAX_ITER = 64, 7, 8
TINY_COMBOS = tuple((p, q, k) for p in (1, 5, 511, 512, 513) for q in (1, 2) for k in sorted({1, p // 2, p} - {0}))


def tiny_problem(p, q):
    """(cols, y, z) of the tiny fits: 64 rows, min(3, p) planted effects, an intercept and (q = 2) one Gaussian covariate."""
    from conftest import make_bed
    rng = np.random.default_rng([TINY_SEED, p, q])
    cols = make_bed(rng, TINY_N, p, maf_lo=0.2)
    planted = np.sort(rng.choice(p, min(3, p), replace=False))
    y = planted_response(cols, TINY_N, planted, rng)
    z = np.column_stack([np.ones(TINY_N)] + [rng.standard_normal(TINY_N) for _ in range(q - 1)])
    return cols, y, z


def oracle_wavers(oracle, ox, y, z, tol=1e-5, **kw):
    """True when the oracle's own fit moves by more than `tol` under the ulp-sized nudges of its covariates (_unstable)."""
    pick = lambda d, g=1.0: dict(iter=d["iter"], beta=d["beta"], c=d["c"] * g, logl=d["logl"], bt=np.asarray(d["bt_trace"], dtype=float))
    z = np.ones((len(y), 1)) if z is None else z
    o = oracle.fit_iht(ox, y, z, **kw)
    return any(_unstable(pick(o), pick(oracle.fit_iht(ox, y, z * g, **kw), g), tol) for g in _NUDGES)


# combinations of TINY_COMBOS whose oracle trajectory moves under the nudges (tests/test_select_edges_cpu.py asserts the list): a
# one-SNP model with the intercept alone is solved by the first exact line search, and every later backtracking decision compares
# loglikelihoods that are equal to rounding
TINY_DROPPED = ((1, 1, 1), (5, 1, 1), (511, 1, 1), (512, 1, 1))

SELECT_C_N, SELECT_C_RUN, SELECT_C_WEIGHT = 400, 256 * 1000, 100.0      # layout C: rows, first column of the 40-column run, prior weight on it


def select_layout_c(at_boundary, polymorphic=None):
    """(p, planted) of layout C: 40 adjacent columns at the start of one 256-aligned run, p + 1 = 4 x 512 x 256 - 1 (k_res_collect
    deals the vector out entry by entry: 40 lists) or 4 x 512 x 256 (runs of 256: ONE list).  polymorphic (a flag per column of the
    matrix at hand: enough minor alleles to carry an effect): the first such run from column SELECT_C_RUN on whose 40 columns all
    have the flag."""
    C = select_constants()
    length = C["spread_strides"] * C["collect_blocks"] * 256 - (0 if at_boundary else 1)
    start = SELECT_C_RUN
    if polymorphic is not None:
        ok = np.asarray(polymorphic, dtype=bool)
        start = next(s for s in range(SELECT_C_RUN, length - 1 - 256, 256) if ok[s:s + 40].all())
    return length - 1, start + np.arange(40)


def model_size_cases(q=3):
    """(name, k, zkeep, where) of the model-size edges with q covariates: K = k + zkeepn, K + 64 against kResMaxList (the select in
    LDS / in scratch memory) and kResBigList (resident at all).  where: "lds", "scratch" or "host"."""
    C = select_constants()
    out = []
    for zkeep in (None, [1, 0, 1]):
        zn = q if zkeep is None else sum(zkeep)
        out.append((f"last LDS select, zkeepn={zn}", C["max_list"] - 64 - zn, zkeep, "lds"))
        out.append((f"first scratch select, zkeepn={zn}", C["max_list"] - 64 - zn + 1, zkeep, "scratch"))
    out.append(("last resident model", C["big_list"] - 64 - q, None, "scratch"))
    out.append(("first model beyond the scratch lists", C["big_list"] - 64 - q + 1, None, "host"))
    return out


# ---- the GLM refit of debias! on its own (csrc/debias.hip through mih_probe_debias_glm): problems, the panel rebuilt on the host,
# ---- the exact Gram with its counted bound, the closed forms in numpy and in mpmath ----
DEBIAS_DIST = {"normal": 0, "bernoulli": 1, "poisson": 2, "negbin": 3, "gamma": 4, "invgauss": 5}
DEBIAS_LINK = {"identity": 0, "logit": 1, "log": 2, "probit": 3, "cloglog": 4, "cauchit": 5, "inverse": 6, "invsquare": 7, "sqrt": 8}
DEBIAS_FORMS = (("normal", "identity", 1.0), ("normal", "log", 1.0), ("bernoulli", "logit", 1.0), ("bernoulli", "cloglog", 1.0),
                ("bernoulli", "cauchit", 1.0), ("poisson", "log", 1.0), ("poisson", "sqrt", 1.0), ("negbin", "log", 4.0), ("negbin", "log", 0.5),
                ("gamma", "log", 1.0), ("gamma", "inverse", 1.0), ("invgauss", "log", 1.0), ("invgauss", "invsquare", 1.0))
DEBIAS_SHAPES = ((257, 17), (1000, 48), (4097, 33))
DEBIAS_KS = (1, 15, 16, 17, 31, 32, 33, 48)
DEBIAS_NS = (17, 63, 64, 65, 1000, 4095, 4096, 4097, 4161)
DEBIAS_FLAGS = ((1, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0))
DEBIAS_P = 83                                   # columns of the 2-bit matrices: two full 32-column groups and a ragged one of 19
_STORED = np.array([0, 0, 1, 2], dtype=np.int64)          # PLINK code -> stored dosage (a missing entry is stored as 0)


def debias_gamma(n):
    """The relative error allowed to an entry of the Gram of k_db_gram / k_db_gram_reduce, in units of sum_i |P_ia w_i P_ib|, COUNTED
    from the kernels: a row slice holds per = ceil(n / 64) rows, each one fma step of the chain (the padding rows of a chunk add
    +0.0 exactly); 64 additions join the slices; the product P_ia w_i is rounded once, and one more for the second-order terms."""
    from fractions import Fraction
    return Fraction(-(-n // 64) + 64 + 2, 2 ** 53)


def debias_support(p, k, rng, ordered=True):
    """k columns of 0 .. p-1 that hold column 0, column p - 1 (in the ragged last 32-column group), a run of adjacent columns across
    the 32-column boundary (30 .. 33) and random others; ascending, or (ordered=False) in a random order."""
    must = [0, p - 1, 31, 32, 30, 33][:k] if k > 1 else [int(rng.integers(2)) * (p - 1)]
    rest = [int(j) for j in rng.permutation(p) if j not in must]
    idx = np.array(must + rest[:k - len(must)], dtype=np.int64)
    return np.sort(idx) if ordered else idx[rng.permutation(k)]


def debias_codes(rng, n, p, miss=0.02):
    """PLINK codes (p x n) with allele frequencies 0.15 .. 0.5 and a share `miss` of missing entries."""
    maf = rng.uniform(0.15, 0.5, p)
    code = np.array([0, 2, 3], dtype=np.uint8)[rng.binomial(2, maf[:, None], size=(p, n))]
    if miss > 0:
        code[rng.random((p, n)) < miss] = 1
    return code


def debias_panel_snp(code, idx, mu, sinv, center, scale, impute):
    """The n x k panel k_db_cols_snp + k_db_cols_missing decode from the 2-bit matrix, rebuilt from the PLINK codes (p x n) and the
    handle's own mu and sinv: ((double)g - cm) * s for a stored entry, ((impute ? mu : 0) - cm) * s for a missing one, cm = center ?
    mu : 0, s = scale ? sinv : 1 -- one subtraction and one multiplication, each rounded once on both sides."""
    c = np.asarray(code)[np.asarray(idx)]
    s = np.asarray(sinv, dtype=np.float64)[idx] if scale else np.ones(len(idx))
    cm = np.asarray(mu, dtype=np.float64)[idx] if center else np.zeros(len(idx))
    fill = ((np.asarray(mu, dtype=np.float64)[idx] if impute else np.zeros(len(idx))) - cm) * s
    P = (_STORED[c].astype(np.float64) - cm[:, None]) * s[:, None]
    return np.ascontiguousarray(np.where(c == 1, fill[:, None], P).T)


def debias_panel_dosage(num, den, idx):
    """dosage_x of csrc/common.h on the columns idx: ((double)num - mun_j) * sc_j, 0.0 for a missing entry (dosage_host_stats)."""
    mun, sc, _, _ = dosage_host_stats(num, den)
    sub = num[:, idx]
    return np.where(sub == 0xFFFF, 0.0, (sub.astype(np.float64) - mun[idx][None, :]) * sc[idx][None, :])


def _col_ints(A):
    """The doubles A (n x m) as Python integers over one power of two per column: A[i, c] = I[i, c] * 2 ** e[c], exactly."""
    A = np.asarray(A, dtype=np.float64)
    assert np.isfinite(A).all()
    mant, ex = np.frexp(A)
    M = np.ldexp(mant, 53).astype(np.int64)
    ex = ex.astype(np.int64) - 53
    nz = A != 0.0
    e = np.where(nz, ex, np.iinfo(np.int64).max).min(axis=0)
    e = np.where(nz.any(axis=0), e, 0)
    shift = np.where(nz, ex - e[None, :], 0)
    return M.astype(object) << shift.astype(object), [int(v) for v in e]


def _abs_limbs(I, bits=18):
    """|I| (an object array of Python integers) as float64 arrays of `bits`-bit limbs, least significant first, and the signs."""
    sign = np.where(I < 0, -1.0, 1.0)
    W = np.abs(I)
    top = max(int(v).bit_length() for v in W.ravel())
    mask = (1 << bits) - 1
    return [((W >> (bits * l)) & mask).astype(np.float64) for l in range(max(1, -(-top // bits)))], sign


def debias_gram_exact(P, w, bits=18):
    """sum_i P_ia w_i P_ib and sum_i |P_ia w_i P_ib| for every (a, b), exactly, as Fractions (two m x m object arrays).  Every
    double is an integer over a power of two; the integers are cut into 18-bit limbs and the limb matrices multiplied in float64,
    where every product (< 2^36) and every sum over n < 2^16 rows is exact; the limbs are joined in Python integers."""
    from fractions import Fraction
    P = np.asarray(P, dtype=np.float64)
    n, m = P.shape
    assert n < 2 ** 16
    I, e = _col_ints(P)
    Wi, ew = _col_ints(np.asarray(w, dtype=np.float64).reshape(n, 1))
    Q = I * Wi
    la, sa = _abs_limbs(I, bits)
    lq, sq = _abs_limbs(Q, bits)
    N = np.zeros((m, m), dtype=object); S = np.zeros((m, m), dtype=object)
    for x, ax in enumerate(la):
        for y, qy in enumerate(lq):
            sh = bits * (x + y)
            N = N + ((ax * sa).T @ (qy * sq)).astype(np.int64).astype(object) * (1 << sh)
            S = S + (ax.T @ qy).astype(np.int64).astype(object) * (1 << sh)
    two = Fraction(2)
    scale = np.array([[two ** (e[a] + e[b] + ew[0]) for b in range(m)] for a in range(m)], dtype=object)
    return N * scale, S * scale


def debias_gram_misses(G, P, w, n, exact=None):
    """Entries of the upper triangle of G (m x m doubles, column-major in a flat array or G[a, b]) farther from the exact Gram of
    the panel P (n x m) under the weights w than debias_gamma(n) * sum_i |P_ia w_i P_ib|.  Returns (misses, worst): misses =
    [(a, b, got, exact as float, bound as float)], worst = the largest error in units of its bound."""
    from fractions import Fraction
    m = P.shape[1]
    G = np.asarray(G, dtype=np.float64).reshape(m, m, order="F")
    E, S = exact if exact is not None else debias_gram_exact(P, w)
    gam = debias_gamma(n)
    bad, worst = [], 0.0
    for a in range(m):
        for b in range(a, m):
            if not np.isfinite(G[a, b]):
                bad.append((a, b, float(G[a, b]), float(E[a, b]), float(gam * S[a, b]))); worst = np.inf
                continue
            err, bound = abs(Fraction(float(G[a, b])) - E[a, b]), gam * S[a, b]
            if err > bound:
                bad.append((a, b, float(G[a, b]), float(E[a, b]), float(bound)))
            if err:
                worst = max(worst, float(err / bound) if bound else np.inf)
    return bad, worst


def debias_gram_restated(P, w):
    """The summation order of k_db_gram / k_db_gram_reduce in plain float64 (a multiply and an add where the kernel has one fma):
    64 row slices of per = ceil(n / 64) rows, each a chain over its rows, joined in slice order.  m x m (the kernel forms the upper
    tiles only)."""
    n, m = P.shape
    per = -(-n // 64)
    Pw = P * np.asarray(w, dtype=np.float64)[:, None]
    G = np.zeros((m, m))
    for s in range(64):
        acc = np.zeros((m, m))
        for i in range(s * per, min((s + 1) * per, n)):
            acc = acc + np.multiply.outer(Pw[i], P[i])
        G = G + acc
    return G


def debias_forms_f64(dist, link, nb_r, y):
    """(w0, t0): the working weight and the working response eta + wrkresid of GLM.jl at eta0 = linkfun(mustart(y)), by the closed
    forms of csrc/fit_common.h (d_mustart, d_linkfun, d_linkinv, d_mueta, d_glmvar) in numpy float64, every intermediate rounded as
    there."""
    y = np.asarray(y, dtype=np.float64)
    pi = 3.141592653589793
    with np.errstate(all="ignore"):
        mu0 = {"bernoulli": (y + 0.5) / 2.0, "poisson": y + 0.1, "negbin": y + np.where(y == 0.0, 1.0 / 6.0, 0.0),
               "gamma": np.where(y == 0.0, 0.1, y)}.get(dist, y)
        eta = {"logit": lambda m: np.log(m / (1.0 - m)), "log": np.log, "cloglog": lambda m: np.log(-np.log1p(-m)),
               "cauchit": lambda m: np.tan(pi * (m - 0.5)), "inverse": lambda m: 1.0 / m, "invsquare": lambda m: 1.0 / (m * m),
               "sqrt": np.sqrt, "identity": lambda m: m}[link](mu0)
        if link == "logit":
            e = np.exp(-np.abs(eta)); f = 1.0 + e
            mu, me = 1.0 / (1.0 + np.exp(-eta)), e / (f * f)
        elif link == "log":
            mu, me = np.exp(eta), np.exp(eta)
        elif link == "cloglog":
            mu, me = -np.expm1(-np.exp(eta)), np.exp(eta) * np.exp(-np.exp(eta))
        elif link == "cauchit":
            mu, me = 0.5 + np.arctan(eta) / pi, 1.0 / (pi * (1.0 + eta * eta))
        elif link == "inverse":
            mu, me = 1.0 / eta, -1.0 / (eta * eta)
        elif link == "invsquare":
            mu = 1.0 / np.sqrt(eta); me = -mu * mu * mu / 2.0
        elif link == "sqrt":
            mu, me = eta * eta, 2.0 * eta
        else:
            mu, me = eta, np.ones_like(eta)
        var = {"bernoulli": mu * (1.0 - mu), "poisson": mu, "negbin": mu * (1.0 + mu / nb_r), "gamma": mu * mu,
               "invgauss": mu * mu * mu}.get(dist, np.ones_like(mu))
        return me * me / var, eta + (y - mu) / me


def _mp_forms():
    """GLM.jl's closed forms in mpmath: mustart(dist, y), linkfun / linkinv / mueta(link, .), glmvar(dist, mu, r)."""
    import mpmath as mp
    half = mp.mpf(1) / 2
    mustart = {"bernoulli": lambda y: (y + half) / 2, "poisson": lambda y: y + mp.mpf(1) / 10,
               "negbin": lambda y: y + (mp.mpf(1) / 6 if y == 0 else 0), "gamma": lambda y: mp.mpf(1) / 10 if y == 0 else y}
    linkfun = {"identity": lambda m: m, "logit": lambda m: mp.log(m / (1 - m)), "log": mp.log, "cloglog": lambda m: mp.log(-mp.log(1 - m)),
               "cauchit": lambda m: mp.tan(mp.pi * (m - half)), "inverse": lambda m: 1 / m, "invsquare": lambda m: 1 / (m * m), "sqrt": mp.sqrt}
    linkinv = {"identity": lambda e: e, "logit": lambda e: 1 / (1 + mp.exp(-e)), "log": mp.exp, "cloglog": lambda e: 1 - mp.exp(-mp.exp(e)),
               "cauchit": lambda e: half + mp.atan(e) / mp.pi, "inverse": lambda e: 1 / e, "invsquare": lambda e: 1 / mp.sqrt(e),
               "sqrt": lambda e: e * e, "probit": lambda e: mp.ncdf(e)}
    mueta = {"identity": lambda e: mp.mpf(1), "logit": lambda e: mp.exp(-e) / (1 + mp.exp(-e)) ** 2, "log": mp.exp,
             "cloglog": lambda e: mp.exp(e) * mp.exp(-mp.exp(e)), "cauchit": lambda e: 1 / (mp.pi * (1 + e * e)),
             "inverse": lambda e: -1 / (e * e), "invsquare": lambda e: -1 / (2 * e * mp.sqrt(e)), "sqrt": lambda e: 2 * e,
             "probit": lambda e: mp.npdf(e)}
    glmvar = {"normal": lambda m, r: mp.mpf(1), "bernoulli": lambda m, r: m * (1 - m), "poisson": lambda m, r: m,
              "negbin": lambda m, r: m * (1 + m / r), "gamma": lambda m, r: m * m, "invgauss": lambda m, r: m * m * m}
    return mustart, linkfun, linkinv, mueta, glmvar


def debias_forms_mp(dist, link, nb_r, y, dps=50):
    """(w0, t0) of debias_forms_f64 as lists of mpmath numbers at `dps` digits: GLM.jl's formulas evaluated literally --
    mu0 = mustart(y), eta0 = linkfun(mu0), mu = linkinv(eta0), w = mueta(eta0)^2 / var(mu), t = eta0 + (y - mu) / mueta(eta0)."""
    import mpmath as mp
    mustart, linkfun, linkinv, mueta, glmvar = _mp_forms()
    W, T = [], []
    with mp.workdps(dps):
        r = mp.mpf(float(nb_r))
        for v in np.asarray(y, dtype=np.float64):
            yy = mp.mpf(float(v))
            eta = linkfun[link](mustart.get(dist, lambda t: t)(yy))
            mu, me = linkinv[link](eta), mueta[link](eta)
            W.append(me * me / glmvar[dist](mu, r)); T.append(eta + (yy - mu) / me)
    return W, T


def debias_form_errors(got, exact):
    """Per entry of got (doubles) against exact (mpmath numbers): (relative error, error in ulps of the exact value, the ulp) as
    float arrays; an exact zero has relative error 0 when got is 0 and inf otherwise."""
    import mpmath as mp
    rel_, ulps, ulp = np.zeros(len(exact)), np.zeros(len(exact)), np.zeros(len(exact))
    with mp.workdps(50):
        for i, (g, x) in enumerate(zip(np.asarray(got, dtype=np.float64), exact)):
            ulp[i] = float(np.spacing(abs(float(x))))
            if not np.isfinite(g):
                rel_[i] = ulps[i] = np.inf
                continue
            d = abs(mp.mpf(float(g)) - x)
            rel_[i] = float(d / abs(x)) if x != 0 else (0.0 if d == 0 else np.inf)
            ulps[i] = float(d / mp.mpf(ulp[i]))
    return rel_, ulps, ulp


def debias_refit_problem(dist, link, nb_r, n, k, attempt=0):
    """One refit of tests/test_gpu_debias_refit.py (d): PLINK codes (DEBIAS_P x n, 2 % missing), the flags (center, scale, impute),
    the ascending support of k columns and y.  Links that need eta in their domain without an intercept (log, inverse,
    inverse-square, sqrt) get an uncentred matrix and positive planted coefficients with a mean linear predictor near 1.2; the
    others a centred, scaled matrix and Gaussian coefficients with sd(eta) = 1.  Deterministic in its arguments; `attempt` is the
    re-draw counter of DEBIAS_REDRAWS."""
    f = DEBIAS_FORMS.index((dist, link, nb_r))
    rng = np.random.default_rng([20280, f, n, k, attempt])
    code = debias_codes(rng, n, DEBIAS_P)
    idx = debias_support(DEBIAS_P, k, rng)
    positive = link in ("log", "inverse", "invsquare", "sqrt")
    csi = ((0, 0, 1), (0, 1, 0))[(f + k) % 2] if positive else (1, 1, 1)
    mu, sinv = snp_host_stats(_pack(code), n)
    X = debias_panel_snp(code, idx, mu, sinv, *csi)
    if positive:
        eta = X @ (rng.uniform(0.02, 0.12, k) / X.mean() * (17.0 / k))
    else:
        eta = X @ (rng.standard_normal(k) / np.sqrt(k))
    mean = {"identity": lambda e: e, "log": np.exp, "logit": lambda e: 1 / (1 + np.exp(-e)), "cloglog": lambda e: -np.expm1(-np.exp(e)),
            "cauchit": lambda e: 0.5 + np.arctan(e) / np.pi, "inverse": lambda e: 1 / e, "invsquare": lambda e: 1 / np.sqrt(e),
            "sqrt": lambda e: e * e}[link](eta)
    if dist == "normal":
        y = eta + rng.standard_normal(n) if link == "identity" else mean * (1.0 + 0.1 * np.clip(rng.standard_normal(n), -3, 3))
    elif dist == "bernoulli":
        y = (rng.random(n) < mean).astype(np.float64)
    elif dist == "poisson":
        y = rng.poisson(mean).astype(np.float64)
    elif dist == "negbin":
        y = rng.negative_binomial(nb_r, nb_r / (mean + nb_r)).astype(np.float64)
    elif dist == "gamma":
        y = rng.gamma(5.0, mean / 5.0)
    else:
        y = rng.wald(mean, 25.0)
    return code, csi, idx, np.ascontiguousarray(y, dtype=np.float64)


# (dist, link, nb_r, n, k) -> attempt: cases whose first draw the oracle does not fit, or not reproducibly under another row order
# (tests/test_debias_refit_cpu.py asserts the condition for the draws listed here and for attempt 0 everywhere else)
DEBIAS_REDRAWS = {}


def debias_refit_cases():
    """Every (dist, link, nb_r, n, k, attempt) of (d): DEBIAS_FORMS x DEBIAS_SHAPES."""
    return [(d, l, r, n, k, DEBIAS_REDRAWS.get((d, l, r, n, k), 0)) for d, l, r in DEBIAS_FORMS for n, k in DEBIAS_SHAPES]


def debias_oracle_beta(oracle, code, csi, idx, y, dist, link, nb_r, perm=None):
    """oracle.debias_glm on the problem (rows in the order perm), the k coefficients in the order of the ascending idx."""
    n = code.shape[1]
    if perm is not None:
        code, y = code[:, perm], y[perm]
    ox = oracle.Mat.from_bed_columns(_pack(code), n, center=csi[0], scale=csi[1], impute=csi[2])
    mask = np.zeros(code.shape[0], np.uint8); mask[idx] = 1
    return oracle.debias_glm(ox, mask, y, dist, link, nb_r)[np.sort(idx)]


def debias_gram_jobs():
    """The jobs of (a): (kind, n, k, flags or None, seed) with kind "snp", "f64", "f32" or "dosage" -- every k at n = 4097, every n
    at k = 17, the corners of the cross product, the flags dealt round; n < k (the not-positive-definite error) on a matrix of
    whole numbers, (0, 0, 1) without a missing entry, where the oracle forms the same Gram bit for bit; a job that succeeds follows
    each of them."""
    pairs = [(4097, k) for k in DEBIAS_KS] + [(n, 17) for n in DEBIAS_NS if n != 4097]
    pairs += [(17, 1), (17, 15), (17, 16), (63, 15), (64, 16), (64, 1), (65, 32), (1000, 31), (1000, 48), (4095, 1), (4095, 33), (4096, 16), (4096, 48),
              (4161, 33), (4161, 48), (4161, 1)]
    jobs = [("snp", n, k, DEBIAS_FLAGS[t % 4], t) for t, (n, k) in enumerate(pairs)]
    jobs += [("snp", 17, 33, (0, 0, 1), 100), ("snp", 63, 17, (1, 1, 1), 102), ("snp", 17, 48, (0, 0, 1), 101), ("snp", 4161, 17, (1, 0, 0), 103)]
    for t, kind in enumerate(("f64", "f32", "dosage")):
        jobs += [(kind, 65, 17, None, 200 + t), (kind, 1000, 33, None, 210 + t), (kind, 4097, 17, None, 220 + t)]
    return jobs


def debias_gram_problem(kind, n, k, flags, seed):
    """The input of one job of debias_gram_jobs: (data, idx, y) -- data the PLINK codes (DEBIAS_P x n), an n x 40 float matrix, or
    (num, den) of an n x 40 dosage matrix with 3 % missing; idx in a random order; y Gaussian."""
    rng = np.random.default_rng([20281, seed, n, k])
    if kind == "snp":
        data = debias_codes(rng, n, DEBIAS_P, miss=0.0 if n < k else 0.02)
        p = DEBIAS_P
    elif kind == "dosage":
        den, p = 255, 40
        num = (rng.binomial(2, rng.uniform(0.15, 0.5, p), (n, p)) * den + rng.integers(-25, 26, (n, p))).clip(0, 2 * den)
        num[rng.random((n, p)) < 0.03] = 0xFFFF
        data = (num.astype(np.uint16), den)
    else:
        p = 40
        data = rng.standard_normal((n, p)) * np.exp(rng.uniform(-2, 2, p))
        data = np.asfortranarray(data.astype(np.float32) if kind == "f32" else data)
    return data, debias_support(p, k, rng, ordered=False), rng.standard_normal(n) * 2.0 + 0.5


# ---- project_group_sparse! at its edges (csrc/group.hip): the radix sorts' constants read from the source, the inputs, a fit ----
_GROUP_PATTERNS = {
    "group.hip": {
        "items": r"constexpr int kRsItems = (\d+), kRsTile = \d+ \* kRsItems;",
        "round": r"constexpr int kRsItems = \d+, kRsTile = (\d+) \* kRsItems;",
        "scan_chunk": r"for \(int64_t base = 0; base < count; base \+= (\d+)\) \{",
        "scan_threads": r"hipLaunchKernelGGL\(k_rs_scan, dim3\(1\), dim3\((\d+)\), 0, s, hist, \(int64_t\)\d+ \* nblk\);",
        "digits": r"hipLaunchKernelGGL\(k_rs_scan, dim3\(1\), dim3\(\d+\), 0, s, hist, \(int64_t\)(\d+) \* nblk\);",
        "key_bits": r"radix_sort_pairs<uint64_t>\(key\.p, key2\.p, idx\.p, perm\.p, len, (\d+), 1, hist\.p, s\);",
        "label_bits": r"radix_sort_pairs<uint32_t>\(lab\.p, lab2\.p, member\.p, member2\.p, len, (\d+), 0, hist\.p, s\);",
        "norm_bits": r"radix_sort_pairs<uint64_t>\(nkey\.p, nkey2\.p, gid\.p, gid2\.p, G, (\d+), 1, hist\.p, s\);",
    },
}
_GROUP_CONSTANTS = {}


def group_constants():
    """The sizes of csrc/group.hip's radix sort the group cases are built around, read from the source as select_constants() reads
    the select's: items (keys a thread owns), round (keys a block takes a round), tile = round x items (keys a block owns),
    scan_chunk (histogram entries k_rs_scan takes at a time), digits (histogram entries a block contributes), the bits of the
    three sorts.  A pattern that no longer matches exactly once is an AssertionError naming it."""
    if not _GROUP_CONSTANTS:
        _GROUP_CONSTANTS.update(_constants_from_sources(_GROUP_PATTERNS))
        _GROUP_CONSTANTS["tile"] = _GROUP_CONSTANTS["round"] * _GROUP_CONSTANTS["items"]
    return dict(_GROUP_CONSTANTS)


def group_lengths():
    T = group_constants()["tile"]
    return (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T, 2 * T + 1, 4 * T, 4 * T + 1, 5 * T + 1)


GROUP_LABELS_BYTE2 = (1, 2, 255, 256, 257, 65535, 65536, 65537)       # and G - 1, G
GROUP_G_BYTE2, GROUP_G_BYTE3 = 70001, 2 ** 24 + 3
GROUP_VALUE_KINDS = ("equal", "zeros", "extremes", "onebyte", "normal")
_GROUP_COMBOS = ((1, 1, 3), (3, 2, 1), (300, 150, 3), (3, 2, "vec"), (300, 150, "vec"))       # (G, J, k)
_GROUP_CASES, _GROUP_KNOWN = [], {}


def group_values(kind, rng, n):
    """n values of one kind: "equal" -- one |y|, random signs (index order alone decides); "zeros" -- 0.0, -0.0, +-1; "extremes" --
    denormals, the smallest normal, 1e-200, 1e308, +-Inf; "onebyte" -- |y| with the bit pattern 1 << j, j uniform in 0 .. 62 (two
    keys differ in ONE byte or in two: every pass of the key sort is the only one that orders some pair); "normal" -- N(0, 1)."""
    sign = rng.choice([-1.0, 1.0], n)
    if kind == "equal":
        return 1.5 * sign
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0]), n)
    if kind == "extremes":
        return rng.choice(np.array([5e-324, -1e-323, 2.2250738585072014e-308, 1e-200, 1e308, np.inf, -np.inf]), n)
    if kind == "onebyte":
        v = (np.uint64(1) << rng.integers(0, 63, n).astype(np.uint64)).view(np.float64).copy()
        v[np.isnan(v)] = 1.0
        return v * sign
    assert kind == "normal"
    return rng.standard_normal(n)


def group_edge_cases():
    """THE inputs of tests/test_gpu_group_edges.py and of its CPU companion tests/test_group_spec_cpu.py (which shows that every
    case has the property its name promises): a list of (name, y, group, J, k), k an int or an int64 vector.  No NaN anywhere.
    T = tile; the lengths 1 .. 5 T + 1 of group_lengths(): a partial wave, a partial round, a last tile of one key, a histogram of
    exactly one scan chunk (4 T) and the first whose carry matters (4 T + 1)."""
    if _GROUP_CASES:
        return list(_GROUP_CASES)
    T = group_constants()["tile"]
    L = group_lengths()
    out, names = [], set()

    def rng_of(tag):
        return np.random.default_rng([20290, *[ord(c) for c in tag]])

    def add(name, y, group, J, k):
        assert name not in names, name
        names.add(name)
        y = np.ascontiguousarray(y, dtype=np.float64)
        group = np.ascontiguousarray(group, dtype=np.int64)
        assert y.ndim == 1 and y.shape == group.shape and not np.isnan(y).any()
        out.append((name, y, group, int(J), int(k) if np.ndim(k) == 0 else np.ascontiguousarray(k, dtype=np.int64)))

    def kvec(rng, G, group):
        k = rng.integers(0, 4, G)
        k[int(group[0]) - 1] = 0                            # a 0 at a populated label
        if group.size > 1 and group[-1] != group[0]:
            k[int(group[-1]) - 1] = 3
        return k

    # (a) the value kinds across the lengths: every length for the stability kind and the control, every combination of (G, J, k)
    # from the first tile edge on for the stability kind, two of them (dealt round) elsewhere
    per_kind = {"equal": L, "normal": L,
                "zeros": (1, 2, 65, 257, T, T + 1, 2 * T + 1, 4 * T + 1),
                "extremes": (2, 64, 256, T - 1, T + 1, 4 * T + 1),
                "onebyte": (255, 257, T, T + 1, 2 * T, 4 * T + 1, 5 * T + 1)}
    for kind in GROUP_VALUE_KINDS:
        for t, n in enumerate(per_kind[kind]):
            every = kind == "equal" and n >= T - 1
            for c in range(len(_GROUP_COMBOS)) if every else ((2 * t) % 5, (2 * t + 1) % 5):
                G, J, k = _GROUP_COMBOS[c]
                rng = rng_of(f"{kind}{n}c{c}")
                group = rng.integers(1, G + 1, n)
                add(f"{kind} len={n} G={G} J={J} k={k}", group_values(kind, rng, n), group, J, kvec(rng, G, group) if k == "vec" else k)
    # a kept -0.0 stays -0.0: everything kept
    for n in (257, T + 1):
        rng = rng_of(f"keepall{n}")
        add(f"zeros len={n} everything kept", group_values("zeros", rng, n), rng.integers(1, 4, n), 3, 2 ** 62)

    # (b) label layouts
    for n in (300, 2 * T + 1):
        rng = rng_of(f"layout{n}")
        y = rng.standard_normal(n)
        add(f"one group len={n}", y, np.ones(n), 1, 3)
        for J in (1, 299, 300):
            add(f"every entry labelled 300 len={n} J={J}", y, np.full(n, 300), J, 3)
        add(f"labels 1 and 300 only len={n}", y, rng.choice([1, 300], n), 2, 3)
        add(f"labels 1 and 300 only len={n} vector k", y, rng.choice([1, 300], n), 2, np.r_[2, rng.integers(0, 4, 298), 3])
        mid = rng.choice(np.r_[1:101, 201:301], n)
        add(f"labels 101..200 empty len={n} J=150", y, mid, 150, 1)
        add(f"labels 101..200 empty len={n} J=250 vector k", y, mid, 250, kvec(rng, 300, mid))
    for tag, G in (("byte 2", GROUP_G_BYTE2), ("byte 3", GROUP_G_BYTE3)):
        rng = rng_of(tag)
        pool = np.array(GROUP_LABELS_BYTE2 + ((2 ** 24, 2 ** 24 + 1) if G == GROUP_G_BYTE3 else ()) + (G - 1, G))
        group = np.r_[pool, rng.choice(pool, 300 - pool.size)][rng.permutation(300)]
        y = rng.standard_normal(300)
        if G == GROUP_G_BYTE3:
            add(f"label {tag}: G={G} len=300 J=5 k=3", y, group, 5, 3)
            continue
        for J in (1, 5, G):
            add(f"label {tag}: G={G} len=300 J={J} k=3", y, group, J, 3)
        add(f"label {tag}: G={G} len=300 J=6 vector k", y, group, 6, kvec(rng, G, group))
        add(f"label {tag}: G={G} len=300 equal |y| J=4 k=2", group_values("equal", rng, 300), group, 4, 2)

    # (c) degenerate J and k
    for n, G in ((257, 3), (T + 1, 300)):
        rng = rng_of(f"degenerate{n}")
        y = rng.standard_normal(n)
        group = rng.integers(1, G + 1, n)
        group[:2] = (1, G)
        for J in (0, 1, G, G + 3, 2 ** 40):
            add(f"J={J} len={n} G={G} k=3", y, group, J, 3)
        for k in (0, 1, 3, 2 ** 62):
            add(f"k={k} len={n} G={G} J=2", y, group, 2, k)
        kv = kvec(rng, G, group)
        add(f"vector k with a 0 at a populated label len={n} G={G}", y, group, G, kv)
        big = kv.copy()
        big[G - 1] = 2 ** 62
        add(f"vector k with 2^62 inside len={n} G={G}", y, group, max(G - 1, 1), big)
        add(f"vector k longer than G len={n} G={G}", y, group, 2, np.r_[kv, rng.integers(0, 4, 7)])
        add(f"vector k all 0 len={n} G={G}", y, group, 2, np.zeros(G, dtype=np.int64))

    # (d) ties with a known answer
    big = 2.0 ** 27                                          # big^2 = 2^54, where an ulp is 4: adding 1.0 nine times, one at a time, changes nothing
    ones = np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, -1.0, 1.0])
    y = np.r_[0.5, ones[:4], -big, -0.25, ones[4:], big, 0.5]
    for lone, many in ((1, 2), (2, 1)):
        group = np.r_[3, [many] * 4, many, 3, [many] * 5, lone, 3]
        want = np.where(group == min(lone, many), y, 0.0)
        name = f"tie across the cut by the sequential sum, the lone entry is group {lone}"
        add(name, y, group, 1, 10)
        _GROUP_KNOWN[name] = want
    y = np.array([6.0, 3.0, 0.5, -5.0, 1.0, -4.0, 0.25, 0.125])
    group = np.array([1, 2, 3, 5, 1, 2, 3, 3])
    for J, alive in ((2, (1, 2)), (3, (1, 2, 5))):
        name = f"3^2 + 4^2 against 5^2 across the cut J={J}"
        add(name, y, group, J, 2)
        _GROUP_KNOWN[name] = np.where(np.isin(group, alive), y, 0.0)      # norms 37, 25, 0.3125, 0 (label 4 is absent), 25
    y = np.array([-0.0, 1.0, 3.0, 0.0, -2.0, -0.0, -0.0, -0.0])
    group = np.array([5, 2, 9, 5, 2, 5, 9, 10])
    k = np.full(10, 2)
    k[8] = 0
    k[4] = 3
    for J, alive in ((4, (2,)), (5, (2, 5)), (8, (2, 5)), (10, (2, 5, 10))):      # the ranking: 2, then the zero norms by label: 1, 3, 4, 5, 6, 7, 8, 9, 10
        name = f"J beyond the non-empty groups: zero norms rank by label J={J}"
        add(name, y, group, J, k)
        _GROUP_KNOWN[name] = np.where(np.isin(group, alive), y, 0.0)
    _GROUP_CASES.extend(out)
    return list(out)


def group_known_answers():
    """{name: the projection written down by hand} of the tie cases of group_edge_cases()."""
    group_edge_cases()
    return dict(_GROUP_KNOWN)


GROUP_FIT_N, GROUP_FIT_P, GROUP_FIT_G, GROUP_FIT_SEED = 301, 4101, 41, 613
GROUP_FIT_CAUSAL = (5, 22, 41)
_GROUP_FIT = {}


def group_fit_problem():
    """The fit of tests/test_gpu_group_edges.py: 301 x 4101 genotypes (make_bed, seed 613, maf >= 0.05) -- the projection sorts
    4101 keys: two full tiles and a third -- with interleaved labels 1 + (7 j mod 41), label 13 relabelled 14 (absent), two causal
    SNPs in each of the groups 5, 22 and 41 with effects +-U(0.6, 0.9), an intercept and one Gaussian covariate.  Returns
    dict(cols, z, group, causal, y={"normal": ..., "bernoulli": ...}, settings=[(k, J), ...])."""
    if _GROUP_FIT:
        return dict(_GROUP_FIT)
    from conftest import make_bed
    n, p, G = GROUP_FIT_N, GROUP_FIT_P, GROUP_FIT_G
    rng = np.random.default_rng(GROUP_FIT_SEED)
    cols = make_bed(rng, n, p, maf_lo=0.05)
    group = 1 + (np.arange(p) * 7 % G)
    group[group == 13] = 14
    causal = np.sort(np.concatenate([rng.choice(np.flatnonzero(group == g), 2, replace=False) for g in GROUP_FIT_CAUSAL]))
    beta = np.zeros(p)
    beta[causal] = rng.choice([-1.0, 1.0], causal.size) * rng.uniform(0.6, 0.9, causal.size)
    g = _dosages(cols[causal], n).astype(np.float64)
    eta = beta[causal] @ ((g - g.mean(axis=1, keepdims=True)) / g.std(axis=1, keepdims=True))
    z = np.column_stack([np.ones(n), rng.standard_normal(n)])
    y_normal = eta + 0.7 + 0.4 * z[:, 1] + rng.standard_normal(n)
    y_bern = (rng.random(n) < 1.0 / (1.0 + np.exp(-(1.5 * eta + 0.2)))).astype(np.float64)
    kv = np.ones(G, dtype=np.int64)
    kv[np.array(GROUP_FIT_CAUSAL) - 1] = 2
    kv[13 - 1] = 0
    _GROUP_FIT.update(cols=cols, z=z, group=group, causal=causal, y={"normal": y_normal, "bernoulli": y_bern}, settings=[(2, 3), (kv, 4)])
    return dict(_GROUP_FIT)
