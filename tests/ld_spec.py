"""The numpy statement of ld / ld_pairs / ld_prune (csrc/ld.hip: mih_ld_band, mih_ld_pairs, mih_ld_prune) over an n x p array
of allele counts with -1 for a missing genotype.  It is the yardstick of the device path.

For columns j, k: g_ij in {0, 1, 2} an observed genotype, miss(j) the missing rows of column j, m_j = |miss(j)|, n_j = n - m_j,
s_j = sum of the observed g_ij, mu_j = s_j / n_j (one float64 division of integers), t_ij = g_ij where observed, 0 where missing.
    D_jk = sum_i t_ij t_ik        A_jk = sum_{i in miss(j)} t_ik        M_jk = |miss(j) & miss(k)|          (integers)
    C_jk = D_jk - mu_j (s_k - A_jk) - mu_k (s_j - A_kj) + mu_j mu_k (n - m_j - m_k + M_jk)
    C_jj = D_jj - s_j^2 / n_j
    r_jk = C_jk / sqrt(C_jj C_kk)
the float operations in exactly this order, each rounded by itself: r is the correlation of the mean-imputed columns (g - mu
where observed, 0 where missing -- the c_ij of grm_spec).  A column is degenerate when n_j = 0 or n_j D_jj = s_j^2 in integers
(monomorphic among its observed genotypes): r = 0 with every column.  The band holds the pairs j < k with k - j < w,
w = min(window, p): r[j, d - 1] = r_{j, j + d}, NaN where j + d >= p (the integers are 0 there)."""
import numpy as np

import qc_spec as Q

U = 2.0 ** -53
ROUNDINGS = 8


def column_stats(codes):
    """(s, m, D_jj) as int64 vectors."""
    t = np.where(codes < 0, 0, codes)                              # (summed as int64 whatever the codes' own type)
    return t.sum(axis=0, dtype=np.int64), (codes < 0).sum(axis=0, dtype=np.int64), (t * t).sum(axis=0, dtype=np.int64)


def degenerate(codes):
    return degenerate_of(codes.shape[0], *column_stats(codes))


def degenerate_of(n, s, m, d):
    nj = n - m
    return (nj == 0) | (nj * d == s * s)


def clamp(window, p):
    if window < 2:
        raise ValueError("window must be at least 2")
    return min(int(window), p)


def band_index(p, w):
    """(j, k, valid) of shape (p, w - 1): k = j + d, valid where k < p (k is clipped to p - 1 elsewhere)."""
    j = np.repeat(np.arange(p)[:, None], w - 1, axis=1)
    k = j + np.arange(1, w)[None, :]
    valid = k < p
    return j, np.where(valid, k, p - 1), valid


def stats(codes, window):
    """(stats (p, w - 1, 4) int64: D_jk, A_jk, A_kj, M_jk by their definitions, 0 where j + d >= p; diag (p,) int64: D_jj)."""
    n, p = codes.shape
    w = clamp(window, p)
    t = np.where(codes < 0, 0, codes).astype(np.int64)
    miss = (codes < 0).astype(np.int64)
    D, A, M = t.T @ t, miss.T @ t, miss.T @ miss                   # A[j, k] = sum_{i in miss(j)} t_ik
    j, k, valid = band_index(p, w)
    out = np.stack([D[j, k], A[j, k], A[k, j], M[j, k]], axis=2)
    out[~valid] = 0
    return out, np.diag(D).copy()


def _terms(codes, st, window):
    """The pieces of the formula over the band, in float64: everything r() and bound() share.  codes: the n x p array, or
    (n, s, m, D_jj) -- the column statistics are all the formula needs beside the band's integers."""
    if isinstance(codes, tuple):
        n, s, m, d = codes
    else:
        n, (s, m, d) = codes.shape[0], column_stats(codes)
    p = s.size
    w = clamp(window, p)
    j, k, valid = band_index(p, w)
    nj = (n - m).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = s.astype(np.float64) / nj
        sq = (s * s).astype(np.float64) / nj
    cdiag = d.astype(np.float64) - sq
    D, Ajk, Akj, M = (st[:, :, q] for q in range(4))
    t1 = mu[j] * (s[k] - Ajk).astype(np.float64)
    t2 = mu[k] * (s[j] - Akj).astype(np.float64)
    t3 = (mu[j] * mu[k]) * (n - m[j] - m[k] + M).astype(np.float64)
    return dict(j=j, k=k, valid=valid, D=D.astype(np.float64), t1=t1, t2=t2, t3=t3, cdiag=cdiag, tdiag=d.astype(np.float64) + sq,
                deg=degenerate_of(n, s, m, d))


def r(codes, window, st=None):
    """The band of r, (p, w - 1) float64 (codes as in _terms; st is required with column statistics)."""
    if st is None:
        st = stats(codes, window)[0]
    q = _terms(codes, st, window)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = ((q["D"] - q["t1"]) - q["t2"]) + q["t3"]
        out = c / np.sqrt(q["cdiag"][q["j"]] * q["cdiag"][q["k"]])
    out[q["deg"][q["j"]] | q["deg"][q["k"]]] = 0.0
    out[~q["valid"]] = np.nan
    return out


def bound(codes, window, st=None):
    """|r_device - r_spec| <= bound, elementwise (0 where r is 0 by degeneracy, NaN places excluded by check()).

    Roundings of the spec's expression, u = 2^-53: mu_j and mu_k one division each; t1 = mu_j * int and t2 = mu_k * int two
    each (the mean's and the product's); t3 = (mu_j mu_k) * int four (two means, two products); then the three additions
    ((D - t1) - t2) + t3, each within u of a partial sum that T_jk = |D| + |t1| + |t2| + |t3| bounds.  To first order
    |dC_jk| <= (2 |t1| + 2 |t2| + 4 |t3| + 3 T) u <= 7 u T_jk; C_jj = D_jj - s_j^2 / n_j has two (the division, the
    subtraction), T_jj = D_jj + s_j^2 / n_j.  c = ROUNDINGS = 8 covers both with room for the second-order terms.  Then
        |dr| <= c u T_jk / sqrt(C_jj C_kk) + |r| c u (T_jj / C_jj + T_kk / C_kk) + 4 u |r|
    (the product, the root and the quotient are one rounding each; the root halves what it is given), doubled because the
    numpy side rounds too."""
    if st is None:
        st = stats(codes, window)[0]
    q = _terms(codes, st, window)
    rr = np.abs(r(codes, window, st))
    T = np.abs(q["D"]) + np.abs(q["t1"]) + np.abs(q["t2"]) + np.abs(q["t3"])
    cj, ck, tj, tk = q["cdiag"][q["j"]], q["cdiag"][q["k"]], q["tdiag"][q["j"]], q["tdiag"][q["k"]]
    with np.errstate(invalid="ignore", divide="ignore"):
        b = ROUNDINGS * U * T / np.sqrt(cj * ck) + rr * ROUNDINGS * U * (tj / cj + tk / ck) + 4.0 * U * rr
    b[q["deg"][q["j"]] | q["deg"][q["k"]]] = 0.0
    b[~q["valid"]] = 0.0
    return 2.0 * b


def check(got, want, tol, what=""):
    """got against the spec's (want, tol), elementwise, with NaN in the same places."""
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    err = np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want))
    bad = ~nan & ~(err <= tol)
    assert not bad.any(), (what, float(err[bad].max()), float(tol[bad].min()), np.argwhere(bad)[:4].tolist())


def brute_r(codes, window):
    """The correlation of the mean-imputed columns, computed as such: the check of the formula."""
    n, p = codes.shape
    w = clamp(window, p)
    obs = codes >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(obs, codes, 0).sum(axis=0) / obs.sum(axis=0)
    c = np.where(obs, codes - np.where(np.isfinite(mu), mu, 0.0)[None, :], 0.0)
    cov = c.T @ c
    with np.errstate(invalid="ignore", divide="ignore"):
        full = cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    deg = degenerate(codes)
    full[deg, :] = 0.0
    full[:, deg] = 0.0
    j, k, valid = band_index(p, w)
    out = full[j, k]
    out[~valid] = np.nan
    return out


def pairs(rband, threshold):
    """(j, k) of the band entries with r r > threshold (strictly; a NaN is no pair), in the order (j, k)."""
    with np.errstate(invalid="ignore"):
        j, d = np.nonzero(rband * rband > threshold)
    return j.astype(np.int64), (j + d + 1).astype(np.int64)


def maf(codes):
    return Q.maf(Q.counts(codes)[0])


def prune(codes, window, step, threshold, rband=None):
    """The greedy pass of `plink --indep-pairwise window step threshold` over the band of r: a boolean mask of the kept columns.
    Degenerate columns are dropped first.  For s = 0, step, 2 step, ... < p the window is the columns [s, min(s + w, p)); inside
    it i ascends over the kept columns and j over the kept columns above i; where r_ij^2 > threshold and maf(i) < maf(j), i is
    dropped and the inner loop left, otherwise j is dropped (a tie keeps the earlier column).  One pass per window suffices:
    drops never make a compared pair comparable again."""
    n, p = codes.shape
    if step < 1:
        raise ValueError("step must be at least 1")
    w = clamp(window, p)
    if rband is None:
        rband = r(codes, window)
    r2 = rband * rband
    f = maf(codes)
    keep = ~degenerate(codes)
    for s in range(0, p, step):
        e = min(s + w, p)
        for i in range(s, e):
            if not keep[i]:
                continue
            for j in range(i + 1, e):
                if keep[j] and r2[i, j - i - 1] > threshold:
                    if f[i] < f[j]:
                        keep[i] = False
                        break
                    keep[j] = False
    return keep


# ---- the inputs of the device tests ------------------------------------------------------------------------------------------------
EDGE_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 385)
EDGE_P = (1, 2, 31, 32, 33, 64, 65, 97, 150)
EDGE_W = (2, 3, 32, 33, 34, 65, "p", "p+10")
THRESHOLDS = (0.1999, 0.4999)
PAIR_WINDOWS = (2, 33, "p")
PRUNE_SHAPES = ((2, 1), (33, 5), (50, 5), ("p", "p"), (64, 64))
MARGIN = 1e-9


def planted(n, p, seed, missing=0.03):
    """Planted LD: columns come in runs of 1-6, each column of a run the previous one with 5-60 % of its genotypes redrawn; a
    share `missing` of the genotypes is missing; where p >= 31 a monomorphic-0 and a monomorphic-2 column and (unless missing
    is 0) an all-missing one."""
    rng = np.random.default_rng(seed)
    codes = np.empty((n, p), dtype=np.int64)
    j = 0
    while j < p:
        run, f = int(rng.integers(1, 7)), rng.uniform(0.1, 0.5)
        col = rng.binomial(2, f, n)
        for t in range(run):
            if j >= p:
                break
            if t > 0:
                redraw = rng.random(n) < rng.uniform(0.05, 0.6)
                col = np.where(redraw, rng.binomial(2, f, n), col)
            codes[:, j] = col
            j += 1
    if missing > 0:
        codes[rng.random((n, p)) < missing] = -1
    if p >= 31:
        codes[:, 3], codes[:, 17] = 0, 2
        if missing > 0:
            codes[:, p - 2] = -1
    return codes


def window_of(w, p):
    """(a window must be at least 2: "p" of a single column is 2, which is clamped to p again)"""
    return max(p, 2) if w == "p" else p + 10 if w == "p+10" else int(w)


def edge_cases():
    """(n, p, window, missing share, seed): every (p, window) of EDGE_P x EDGE_W, the n cycling through EDGE_N with a stride
    that meets every n six times, and twelve more that combine several row slices (n >= 257) with several panels (p >= 65).
    A quarter of the cases has no missing genotype at all (the one-product kernel), chosen so that it meets every window and
    every p: window index w_i of column count index p_i where (3 p_i + w_i) % 4 == 3."""
    out = []
    for pi, p in enumerate(EDGE_P):
        for wi, w in enumerate(EDGE_W):
            t = len(EDGE_W) * pi + wi
            n = EDGE_N[(5 * t + t // len(EDGE_N)) % len(EDGE_N)]
            out.append((n, p, window_of(w, p), 0.0 if (3 * pi + wi) % 4 == 3 else 0.03, 7000 + t))
    t = 0
    for p in (65, 97, 150):
        for n in (257, 385):
            for w in (34, 65):
                out.append((n, p, w, 0.0 if t % 4 == 1 else 0.03, 7100 + t))
                t += 1
    return out


def list_cases():
    """The inputs of the pair-list and pruning tests: (n, p, missing share, seed)."""
    return [(129, 150, 0.03, 11), (385, 97, 0.0, 12), (15, 65, 0.03, 13), (16, 64, 0.03, 14), (257, 33, 0.03, 15)]


def min_margin(codes, window, threshold):
    """min over the band of |r^2 - threshold| (inf for an empty band)."""
    rb = r(codes, window)
    v = np.abs(rb * rb - threshold)[~np.isnan(rb)]
    return float(v.min()) if v.size else np.inf
