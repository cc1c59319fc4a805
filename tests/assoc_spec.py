"""The numpy statement of the marginal association scan (csrc/assoc.hip: mih_assoc_score; score_test and assoc of the matrix
classes).  It is the yardstick of the device path.

x_ij is the entry of the matrix as mih_xtv multiplies it.  For a 2-bit matrix with mean mu_j = (n1 + 2 n2) / n_obs and
sinv_j = 1 / sqrt(mu_j (1 - mu_j / 2)) (1 where that is not positive) and the handle's flags (center, scale, impute):
    x(g) = (g - [center] mu_j) * ([scale] sinv_j, else 1),   a missing entry: g = [impute] mu_j, else 0.
Inputs: A (n x t) score residuals, w (n) working weights >= 0 (None: ones), Z (n x c) covariates.  Per column j and trait s
    U_js = sum_i x_ij A_is,      b_j = sum_i x_ij (w_i Z_i.)  (c-vector; w_i Z_ik is one product),      Q_j = sum_i x_ij^2 w_i
    G = Z'WZ = L L' (unpivoted Cholesky),   V_j = Q_j - |L^-1 b_j|^2
    z_js = U_js / sqrt(V_j),   beta_js = U_js / V_j,   se_j = 1 / sqrt(V_j),   neglog10p_js = -log10 erfc(|z_js| / sqrt 2).
The per-column finish has a FIXED floating-point order, every operation rounded by itself (finish()):
    u_k = sum_{l <= k} Linv[k, l] b_l, l ascending from 0.0;   r2 = sum_k u_k u_k, k ascending from 0.0;   V = Q - r2;
    z = U / sqrt(V);  beta = U / V;  se = 1.0 / sqrt(V).
Q of a 2-bit column is its four class sums, from the left:  Q = x(0)^2 W0 + x(1)^2 W1 + x(2)^2 W2 + x(miss)^2 Wm, x^2 = x * x,
W1 / W2 the weight of the rows with dosage 1 / 2, Wm of the missing rows, W0 of the rows with dosage 0 (the device forms it as
sum w - W1 - W2 - Wm in exact integers of the fixed-point weights).

Degenerate columns have NaN in z, beta, se and neglog10p: a 2-bit column without an observed genotype or monomorphic among its
observed ones (integers), and any column with V <= 0.

With an intercept in span(Z) and impute = True the statistics do not depend on center / scale: centring subtracts a multiple of
the intercept, which the projection removes, and scaling multiplies U by s and V by s^2, so z is unchanged (beta and se scale by
1 / s).  tests/test_assoc_spec_cpu.py shows it.

U and b are evaluated here in extended precision (numpy longdouble) and rounded once, so that the spec's own error in them is
far below the device bound; Q's class sums with math.fsum (correctly rounded)."""
import math

import numpy as np

U = 2.0 ** -53
EBITS = 53                         # kAssocEbits of csrc/assoc.hip: max w * 2^e < 2^54
SLICE_ROWS_LIMIT = 21845 * 128     # kAssocSliceBp tiles: floor(2^24 / 6) rows rounded down to whole tiles


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
def host_stats(codes):
    """mu_j and sinv_j of an n x p array of allele counts (-1 missing), as the 2-bit handle forms them from the counts."""
    n = codes.shape[0]
    n1, n2, nm = ((codes == v).sum(axis=0).astype(np.float64) for v in (1, 2, -1))
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (n1 + 2.0 * n2) / (float(n) - nm)
        s = np.sqrt(m * (1.0 - m / 2.0))
        sinv = np.where(s > 0.0, 1.0 / s, 1.0)
    return m, sinv


def class_values(mu, sinv, flags):
    """(4, p): x(0), x(1), x(2), x(miss) in the device's operation order."""
    center, scale, impute = flags
    cm = mu if center else np.zeros_like(mu)
    s = sinv if scale else np.ones_like(mu)
    gm = mu if impute else np.zeros_like(mu)
    with np.errstate(invalid="ignore"):
        return np.stack([(0.0 - cm) * s, (1.0 - cm) * s, (2.0 - cm) * s, (gm - cm) * s])


def xtilde(codes, flags, stats=None):
    """The n x p matrix mih_xtv multiplies."""
    mu, sinv = host_stats(codes) if stats is None else stats
    xv = class_values(mu, sinv, flags)
    cls = np.where(codes < 0, 3, codes)
    return np.take_along_axis(xv, cls, axis=0)


def degenerate(codes):
    n0, n1, n2 = ((codes == v).sum(axis=0) for v in (0, 1, 2))
    nobs = n0 + n1 + n2
    return (nobs == 0) | (n0 == nobs) | (n1 == nobs) | (n2 == nobs)


# ---- the weights' fixed point -----------------------------------------------------------------------------------------------------
def quantum(w):
    """q = 2^-e, e = 53 - ilogb(max w) capped at 1000 (1.0 for all-zero weights): every weight is rounded to a multiple of q."""
    top = float(np.max(w))
    if not top > 0.0:
        return 1.0
    return math.ldexp(1.0, -min(EBITS - (math.frexp(top)[1] - 1), 1000))


def quantised(w):
    """(R, q): R_i = rint(w_i / q) as Python integers."""
    q = quantum(w)
    return [int(np.rint(v / q)) for v in np.asarray(w, dtype=np.float64)], q


def class_sums(codes, w):
    """(4, p) float64: W0, W1, W2, Wm of the TRUE weights, each sum correctly rounded (math.fsum).  w None: the counts."""
    n, p = codes.shape
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    out = np.empty((4, p))
    for k, v in enumerate((0, 1, 2, -1)):
        for j in range(p):
            out[k, j] = math.fsum(w[codes[:, j] == v])
    return out


def class_sums_quantised(codes, w):
    """(4, p) of Fractions: the exact class sums of the quantised weights q R_i -- what the device's W are ONE rounding away from."""
    from fractions import Fraction
    R, q = quantised(w)
    R = np.array(R, dtype=object)
    fq = Fraction(q)
    return [[fq * int(sum(R[codes[:, j] == v])) for j in range(codes.shape[1])] for v in (0, 1, 2, -1)]


# ---- the statistic ----------------------------------------------------------------------------------------------------------------
def null_factor(Z, w):
    """(G, Linv): G = Z'WZ, Linv the inverse of its unpivoted Cholesky factor (lower triangular)."""
    Z = np.asarray(Z, dtype=np.float64)
    w = np.ones(Z.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    G = Z.T @ (w[:, None] * Z)
    L = np.linalg.cholesky(G)                      # raises LinAlgError when G is not positive definite
    Linv = np.linalg.solve(L, np.eye(L.shape[0]))
    return G, np.tril(Linv)


def linear_terms(X, A, w, Z):
    """(U p x t, b p x c), extended precision rounded once."""
    w = np.ones(X.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    R = np.concatenate([np.asarray(A, dtype=np.float64).reshape(X.shape[0], -1), w[:, None] * np.asarray(Z, dtype=np.float64)], axis=1)
    with np.errstate(invalid="ignore"):
        S = (X.astype(np.longdouble).T @ R.astype(np.longdouble)).astype(np.float64)
    t = R.shape[1] - np.asarray(Z).shape[1]
    return S[:, :t], S[:, t:]


def q_snp(codes, w, flags, stats=None, W=None):
    mu, sinv = host_stats(codes) if stats is None else stats
    xv = class_values(mu, sinv, flags)
    W = class_sums(codes, w) if W is None else W
    with np.errstate(invalid="ignore"):
        q = (xv[0] * xv[0]) * W[0]
        q = q + (xv[1] * xv[1]) * W[1]
        q = q + (xv[2] * xv[2]) * W[2]
        q = q + (xv[3] * xv[3]) * W[3]
    return q


def q_dense(X, w):
    w = np.ones(X.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    XL = X.astype(np.longdouble)
    return ((XL * XL).T @ w.astype(np.longdouble)).astype(np.float64)


def finish(Um, b, Q, Linv, deg):
    """(z, beta, se, V) in the fixed order of the module docstring."""
    p, c = b.shape
    r2 = np.zeros(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(c):
            u = np.zeros(p)
            for l in range(k + 1):
                u = u + Linv[k, l] * b[:, l]
            r2 = r2 + u * u
        V = Q - r2
        V = np.where(deg | ~(V > 0.0), np.nan, V)
        rt = np.sqrt(V)
        z = Um / rt[:, None]
        beta = Um / V[:, None]
        se = 1.0 / rt
    return z, beta, se, V


def neglog10p(z):
    """-log10 of the two-sided normal tail, from scipy's log_ndtr (finite where p underflows)."""
    from scipy.special import log_ndtr
    return -(math.log(2.0) + log_ndtr(-np.abs(z))) / math.log(10.0)


def score(codes, flags, A, w, Z):
    """The whole statement for a 2-bit matrix: dict of z, beta (p x t), se, V, Q (p), U, b, G, Linv, deg, X."""
    stats = host_stats(codes)
    X = xtilde(codes, flags, stats)
    Um, b = linear_terms(X, A, w, Z)
    G, Linv = null_factor(Z, w)
    deg = degenerate(codes)
    Q = q_snp(codes, w, flags, stats)
    z, beta, se, V = finish(Um, b, Q, Linv, deg)
    return dict(z=z, beta=beta, se=se, V=V, Q=Q, U=Um, b=b, G=G, Linv=Linv, deg=deg, X=X, stats=stats)


def score_dense(X, A, w, Z):
    """The statement for a dense or dosage matrix X (the entries mih_xtv multiplies): only V <= 0 is degenerate."""
    Um, b = linear_terms(X, A, w, Z)
    G, Linv = null_factor(Z, w)
    Q = q_dense(X, w)
    deg = np.zeros(X.shape[1], dtype=bool)
    z, beta, se, V = finish(Um, b, Q, Linv, deg)
    return dict(z=z, beta=beta, se=se, V=V, Q=Q, U=Um, b=b, G=G, Linv=Linv, deg=deg, X=X)


def brute(X, A, w, Z):
    """The brute-force statement: residualise every column on Z under W, then V = x_perp' W x_perp and U = x_perp' A."""
    n = X.shape[0]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64).reshape(n, -1)
    sw = np.sqrt(w)
    coef = np.linalg.lstsq(Z * sw[:, None], X * sw[:, None], rcond=None)[0]
    Xp = X - Z @ coef
    V = np.einsum("ij,i,ij->j", Xp, w, Xp)
    Um = Xp.T @ A
    return Um / np.sqrt(V)[:, None], Um / V[:, None], 1.0 / np.sqrt(V), V


# ---- the bound --------------------------------------------------------------------------------------------------------------------
def _xtv_bound_snp(codes, flags, stats, R):
    """|X'r_device - X'r| per column and residual (p x m) for a 2-bit handle: the bound tests/test_gpu_xtv_residual_edges.py holds
    X'r to (gpu_helpers.xtv_edge_exact / xtv_matrix_exact / xtv_std_exact), restated in floats for the fused default format:
        |sinv_j| ( (q / 2) sum_i g_ij [row i not peeled, r_i != 0] + C u D_j + u [ (k_j - 1) M_j + (ceil(n / 16384) + 70) S_j + 6 (D_j + M_j + S_j) ] )
    (a residual that is exactly 0 has the fixed-point value 0: no quantisation error; a train mask that leaves few rows has every
    non-zero row peeled, and the term vanishes), q = xtv_quantum(r), C = xtv_recombine_count(None, 16) (the largest slice count), D_j = sum_i g_ij |r_i|, M_j = [impute] |mu_j|
    sum_{i missing} |r_i|, S_j = [center] |mu_j| sum_i |r_i|, k_j the column's missing entries."""
    import gpu_helpers as H
    center, scale, impute = flags
    mu, sinv = stats
    n, p = codes.shape
    g = np.where(codes < 0, 0, codes).astype(np.float64)
    miss = (codes < 0).astype(np.float64)
    kj = miss.sum(axis=0)
    C = H.xtv_recombine_count(None, 16)
    out = np.empty((p, R.shape[1]))
    amu = np.abs(np.nan_to_num(mu))
    si = np.abs(sinv) if scale else np.ones(p)
    for v in range(R.shape[1]):
        r = R[:, v]
        q = H.xtv_quantum(r, None)
        inside = np.ones(n)
        inside[H.peel_rule(r)] = 0.0
        inside[r == 0.0] = 0.0
        ar = np.abs(r)
        D = g.T @ ar
        M = amu * (miss.T @ ar) if impute else np.zeros(p)
        S = amu * ar.sum() if center else np.zeros(p)
        out[:, v] = si * (q / 2 * (g.T @ inside) + C * U * D + U * (np.maximum(kj - 1, 0) * M + (-(-n // 16384) + 70) * S + 6 * (D + M + S)))
    return out * (1.0 + 1e-9)          # (the float restatement of a rational bound)


def _xtv_bound_dense(X, R):
    """Plain f64 dot products of length n in any order: |error| <= (n + 8) u sum_i |x_i r_i| (the classical bound; the device sums
    per thread and then over a tree, which is shorter)."""
    n = X.shape[0]
    return (n + 8) * U * (np.abs(X).T @ np.abs(R))


def bound(sp, codes, flags, A, w, Z):
    """(dz, dbeta (p x t), dse (p)): |device - spec| <= these on the non-degenerate columns.  codes None: a dense / dosage matrix sp["X"].

    U and b: the X'r bound of the residual-edge tests (above), dU (p x t) and db (p x c).
    Q, 2-bit: the device's class sums are the exact sums of the quantised weights rounded once, the spec's the exact sums of the
        true weights rounded once, so |dW_k| <= (q / 2) count_k + 2 u W_k and, with the four products, three additions and the
        squares of the expression, dQ <= sum_k x_k^2 |dW_k| + 8 u sum_k x_k^2 W_k.  Unit weights: q = 0.
    Q, dense: dQ <= (n + 8) u Q (all terms are positive).
    r2 = |L^-1 b|^2: with lmin, lmax the extreme eigenvalues of G and kappa = lmax / lmin,
        d r2 <= 2 sqrt(r2) |db|_2 / sqrt(lmin) + |db|_2^2 / lmin          (the error of b through L^-1, |L^-1|_2 = lmin^-1/2)
              + 2 kappa eps_G r2,   eps_G = u c (n + 8 c + 16)            (G summed in another order on the two sides, each entry within
                                                                           (n + 2) u sqrt(G_kk G_ll); Cholesky, inverse and the products
                                                                           8 c u more: a relative perturbation of G, magnified by kappa)
              + 2 (c + 2) u r2                                            (the two chains of the fixed order)
    V = Q - r2: dV <= dQ + d r2 + u (Q + r2).  With x = dV / V <= 1/2 ((1 - x)^-1/2 - 1 <= x, (1 - x)^-1 - 1 <= 2 x):
        dz <= dU / sqrt(V) + |z| dV / V + 3 u |z|,   dbeta <= dU / V + 2 |beta| dV / V + 2 u |beta|,   dse <= se dV / V + 3 u se
    (inf where dV > V / 2: the inputs keep V / Q >= 1e-3 and kappa <= 100, so this does not happen).  Doubled for numpy's own rounding."""
    X = sp["X"]
    n, p = X.shape
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64).reshape(n, -1)
    Z = np.asarray(Z, dtype=np.float64)
    t, c = A.shape[1], Z.shape[1]
    R = np.concatenate([A, wv[:, None] * Z], axis=1)
    if codes is None:
        dS = _xtv_bound_dense(X, R)
        dQ = (n + 8) * U * sp["Q"]
    else:
        dS = _xtv_bound_snp(codes, flags, sp["stats"], R)
        xv = class_values(*sp["stats"], flags)
        W = class_sums(codes, w)
        q = 0.0 if w is None else quantum(wv)
        cnt = np.stack([(codes == v).sum(axis=0) for v in (0, 1, 2, -1)]).astype(np.float64)
        x2 = xv * xv
        with np.errstate(invalid="ignore"):
            dQ = (x2 * (q / 2 * cnt + 2 * U * W)).sum(axis=0) + 8 * U * (x2 * W).sum(axis=0)
    dU, db = dS[:, :t], dS[:, t:]
    ev = np.linalg.eigvalsh(sp["G"])
    lmin, lmax = float(ev[0]), float(ev[-1])
    kappa = lmax / lmin
    r2 = sp["Q"] - sp["V"]
    nb = np.sqrt((db * db).sum(axis=1))
    eps_g = U * c * (n + 8 * c + 16)
    with np.errstate(invalid="ignore", divide="ignore"):
        dr2 = 2 * np.sqrt(np.abs(r2)) * nb / math.sqrt(lmin) + nb * nb / lmin + 2 * kappa * eps_g * np.abs(r2) + 2 * (c + 2) * U * np.abs(r2)
        dV = dQ + dr2 + U * (sp["Q"] + np.abs(r2))
        x = dV / sp["V"]
        x = np.where(x <= 0.5, x, np.inf)
        rt = np.sqrt(sp["V"])
        dz = dU / rt[:, None] + np.abs(sp["z"]) * x[:, None] + 3 * U * np.abs(sp["z"])
        dbeta = dU / sp["V"][:, None] + 2 * np.abs(sp["beta"]) * x[:, None] + 2 * U * np.abs(sp["beta"])
        dse = sp["se"] * x + 3 * U * sp["se"]
    return 2 * dz, 2 * dbeta, 2 * dse


def check(got, want, tol, what=""):
    """got against the spec's (want, tol), elementwise, with NaN in the same places; returns max err / bound."""
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), (what, "NaN places differ", np.argwhere(np.isnan(got) != nan)[:4].tolist())
    err = np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want))
    bad = ~nan & ~(err <= tol)
    assert not bad.any(), (what, float(err[bad].max()), float(tol[bad].min()), np.argwhere(bad)[:4].tolist())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(nan | (err == 0.0), 0.0, err / tol)
    return float(ratio.max()) if ratio.size else 0.0


# ---- the inputs of the edge tests ----------------------------------------------------------------------------------------------------
EDGE_N = (15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 385)
EDGE_P = (1, 31, 32, 33, 64, 65, 97, 150)
EDGE_TC = ((1, 1), (1, 2), (3, 5), (1, 18), (1, 19), (2, 18))       # the fused pass holds 19 residuals: 19 / 20 is its edge
EDGE_MISSING = (0.0, 0.03)
EDGE_FLAGS = ((1, 1, 1), (1, 1, 0), (0, 0, 1), (1, 0, 1))           # test_gpu_xtv_residual_edges.FLAGS
EDGE_WEIGHTS = ("none", "ones", "logistic", "zeros", "outlier")
MIN_V_OVER_Q = 1e-3
MAX_KAPPA = 100.0


def edge_cases():
    """(n, p, t, c, missing share, flags, weights, seed): every (n, p) once; the other factors cycle with strides that meet every
    value of each many times and every (t, c) with every weight kind.  c <= n / 3 always: a (t, c) that does not fit the n takes
    the next that does.  The outlier weight (one entry 10^6 x the rest) goes with c = 1 and flags that centre and impute, its row
    missing in every column: the row then carries x = 0, otherwise Q_j is that one row and V_j / Q_j ~ 1e-6 whatever the data
    (and for c >= 2 the same row makes kappa(G) ~ 1e6 / n)."""
    out = []
    t = 0
    for ni, n in enumerate(EDGE_N):
        for pi, p in enumerate(EDGE_P):
            wk = EDGE_WEIGHTS[t % 5]
            tc = t // 5
            while True:
                tt, cc = EDGE_TC[tc % 6]
                if 3 * cc <= n:
                    break
                tc += 1
            flags = EDGE_FLAGS[(t // 3) % 4]
            missing = EDGE_MISSING[(t + t // 10) % 2]
            if wk == "outlier":
                tt, cc = 1, 1
                flags = EDGE_FLAGS[0] if flags[0] == 0 or flags[2] == 0 else flags
            out.append((n, p, tt, cc, missing, flags, wk, 9000 + t))
            t += 1
    return out


def edge_inputs(case):
    """codes (n x p), A (n x t), w (n or None), Z (n x c) of an edge case.  Z: an intercept and orthonormalised Gaussian columns
    scaled to sqrt(n), so that kappa(Z'WZ) stays near the spread of the weights.  A: random residuals made orthogonal to Z, as
    those of a fitted null model are (U = x'A = x_perp'A then).  Columns: binomial genotypes with allele
    frequencies 0.1 .. 0.5; where p >= 31 a monomorphic-0, a monomorphic-2 and an all-missing column.  A non-degenerate column
    whose V / Q the spec puts below 10 MIN_V_OVER_Q (its variation sits in rows of weight zero, or Z explains it) is redrawn."""
    n, p, t, c, missing, flags, wk, seed = case
    rng = np.random.default_rng(seed)
    Zr = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1)
    Qf, Rf = np.linalg.qr(Zr)
    Z = Qf * np.sign(np.diag(Rf))[None, :] * math.sqrt(n)
    Z[:, 0] = 1.0
    eta = 0.8 * rng.standard_normal(n)
    mu = 1.0 / (1.0 + np.exp(-eta))
    row0 = int(rng.integers(0, n))
    if wk in ("none", "ones"):
        w = None if wk == "none" else np.ones(n)
        A = rng.standard_normal((n, t)) * np.exp(rng.uniform(-2, 2, t))[None, :]
    else:
        w = mu * (1.0 - mu)
        if wk == "zeros":
            w[rng.random(n) < 0.2] = 0.0
            w[row0] = 0.0
        elif wk == "outlier":
            w = w * 0 + rng.uniform(0.5, 1.5, n)
            w[row0] = 1e6 * float(np.median(w))
        A = (rng.random((n, t)) < mu[:, None]).astype(np.float64) - mu[:, None]
        A[w == 0.0] = 0.0
    wz = Z if w is None else w[:, None] * Z                # a score residual of a fitted null model: Z'A = 0
    A = A - wz @ np.linalg.solve(Z.T @ wz, Z.T @ A)

    def draw():
        col = rng.binomial(2, rng.uniform(0.1, 0.5), n).astype(np.int64)
        if missing > 0:
            col[rng.random(n) < missing] = -1
        if wk == "outlier":
            col[row0] = -1
        return col
    codes = np.stack([draw() for _ in range(p)], axis=1)
    if p >= 31:
        codes[:, 3], codes[:, 17], codes[:, p - 2] = 0, 2, -1
        if wk == "outlier":
            codes[row0, 3] = codes[row0, 17] = -1
    G, Linv = null_factor(Z, w)
    for j in range(p):
        for _ in range(50):
            cj = codes[:, j:j + 1]
            if degenerate(cj)[0]:
                break
            X = xtilde(cj, flags)
            Um, b = linear_terms(X, A, w, Z)
            Q = q_snp(cj, w, flags)
            V = finish(Um, b, Q, Linv, np.zeros(1, dtype=bool))[3]
            if V[0] / Q[0] >= 10 * MIN_V_OVER_Q:
                break
            codes[:, j] = draw()
        else:
            raise AssertionError(("no column with enough variation", case, j))
    return codes, A, w, Z
