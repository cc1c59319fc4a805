"""The numpy statement of the set-based tests on top of the marginal association scan (csrc/assoc_sets.hip: mih_assoc_sets; set_test
and assoc_sets of the matrix classes).  It is the yardstick of the device path and builds on tests/assoc_spec.py, whose U, b, Q, V,
z, Linv and degenerate-column rule it takes as they are (one trait).

A set is a list of entries (column, omega >= 0), columns strictly ascending, at most 128.  Its MEMBERS are the entries whose
column is not degenerate (V is a number) and whose omega > 0, in entry order; m is their count.  Over the members:
    C_jk = sum_i w_i x~_ij x~_ik  (j > k),  x~ the entry as mih_xtv multiplies it (assoc_spec.xtilde)
    u_j  = Linv b_j               (u_jl = sum_{q <= l} Linv[l, q] b_jq, q ascending from 0.0 -- the scan's own)
    K_jk = C_jk - sum_l u_jl u_kl (l ascending from 0.0, every operation rounded by itself),   K_jj = V_j,   K mirrored
    M_jk = (omega_j K_jk) omega_k for j >= k, mirrored
Burden:  a_j = omega_j U_j;  T = sum_j a_j;  rs_j = sum_k M_jk (k ascending);  S = sum_j rs_j (j ascending);
    burden_z = T / sqrt(S), NaN where S <= 0;  neglog10p_burden the two-sided normal tail.
SKAT:    Q = sum_j a_j a_j;  lambda the eigenvalues of M, descending, every lambda_i <= 0 set to 0;  the p-value is
    P(sum lambda_i chi2_1 > Q) by the saddlepoint approximation of Kuonen (1999),
        K(t) = -1/2 sum log1p(-2 lambda_i t),  K' = sum lambda_i / (1 - 2 lambda_i t),  K'' = 2 sum (lambda_i / (1 - 2 lambda_i t))^2,
        t_hat: K'(t_hat) = Q on t < 1 / (2 lambda_1),  w = sign(t_hat) sqrt(2 (t_hat Q - K)),  v = t_hat sqrt(K''),  r = w + log(v / w) / w,
        the tail log Phi(-r).
Everything is evaluated in units of 1 / (2 lambda_1) (root(), finish()):  s = 2 lambda_1 t,  mu_i = lambda_i / lambda_1,  q = Q / lambda_1,
    g(s) = sum mu_i / (1 - mu_i s),  g2(s) = sum (mu_i / (1 - mu_i s))^2,  w^2 = s q + sum log1p(-mu_i s),  v = s sqrt(g2 / 2).
The root of f = g - q:  s = 0, lo missing, hi = 1 (the pole).  Repeat: evaluate g, g2 (one evaluation); |f| <= 2^-40 q: converged,
s_hat = s - f / g2 (one more Newton step) -- stop; 128 evaluations made: not converged -- stop; f < 0: lo = s, else hi = s;
sn = s - f / g2; if not lo < sn < hi: f < 0: sn = (s + hi) / 2; f > 0: sn = (lo + s) / 2 if lo exists, else 2 s if s < 0, else -1; s = sn.

States, decided in this order:  0 -- m = 0, or lambda_1 not > 0 and finite: NaN.  2 -- rank one, m = 1 or lambda_2 <= 2^-40 lambda_1:
the exact chi2_1 tail of Q / lambda_1 as the two-sided normal tail of sqrt(Q) / sqrt(lambda_1) (sqrt(U U) = |U| exactly: a one-variant
set with omega = 1 has the scan's p).  4 -- Q <= 0: 0.  5 -- not converged: the one-sided tail of the moment-matched normal
z = (Q - sum lambda) / sqrt(2 sum lambda^2).  3 -- near the mean, w^2 < 2^-40: the limit of r as w -> 0, kappa_3 / 6 with the
skewness kappa_3 = 8 sum lambda^3 / (2 sum lambda^2)^(3/2) (expand K to third order: w = t sqrt(k2) (1 + k3 t / (3 k2)),
v = t sqrt(k2) (1 + k3 t / (2 k2)), so log(v / w) / w -> k3 / (6 k2^(3/2)): the tail at the mean of a right-skewed law is below 1/2).
1 -- the saddlepoint value.  A set without members has T = S = Q = 0.

C is evaluated here in numpy longdouble and rounded once; the eigenvalues with numpy.linalg.eigvalsh."""
import math

import numpy as np

import assoc_spec as S

LD = np.longdouble
U = 2.0 ** -53
TOL_F = 2.0 ** -40
RANK_ONE = 2.0 ** -40
NEAR_MEAN = 2.0 ** -40
MAX_EVALS = 128
MAX_SET = 128
CHUNK = 32                  # kSetChunk of csrc/assoc_sets.hip: the rows of a decode chunk
LN10 = math.log(10.0)
# The spec's own relative error in log p (SKAT, state 1) against the same formula in 50-digit mpmath with mpmath.eigsy of the
# spec's M, measured on ALL inputs of tests/test_gpu_assoc_sets.py (132 sets in state 1; tests/test_sets_spec_cpu.py measures it
# again on a share of them, the worst among them, and holds it to this figure).  The worst is the 17-variant set of the n = 257
# case, whose Q sits 0.013 standard deviations from the mean: w^2 = s q + sum log1p(-mu_i s) cancels there (w^2 ~ 1e-4 from terms
# ~ 1e-2), and log(v / w) / w divides what is left by w.  Everywhere else the figure is below 1e-14.
SPEC_ERR = 7.3e-12
# The saddlepoint approximation against the exact mixture tail: the worst |delta neglog10p| tests/test_sets_spec_cpu.py measured
# (50 points: spectra of 1 .. 30 equal pairs in closed form at Q from one standard deviation below the mean to 20 above, generic
# spectra of 3 .. 5 eigenvalues by Imhof's integral); the test holds the spec to twice this.
APPROX_ERR = 0.0212


# ---- the covariance ------------------------------------------------------------------------------------------------------------------
def u_of(b, Linv):
    """u = Linv b per row of b (p x c) in the fixed order of the scan's finish."""
    p, c = b.shape
    u = np.zeros((p, c))
    for k in range(c):
        a = np.zeros(p)
        for l in range(k + 1):
            a = a + Linv[k, l] * b[:, l]
        u[:, k] = a
    return u


def members(sp, cols, omega):
    """The positions within the set of its members."""
    cols, omega = np.asarray(cols, dtype=np.int64), np.asarray(omega, dtype=np.float64)
    return np.flatnonzero(~np.isnan(sp["V"][cols]) & (omega > 0))


def cov_members(sp, w, cols, u=None):
    """K (m x m) over the member columns cols."""
    X = sp["X"][:, cols]
    n = X.shape[0]
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    C = ((X.astype(LD) * wv.astype(LD)[:, None]).T @ X.astype(LD)).astype(np.float64)
    u = u_of(sp["b"], sp["Linv"]) if u is None else u
    uu = u[cols]
    dot = np.zeros((len(cols), len(cols)))
    for l in range(uu.shape[1]):
        dot = dot + uu[:, l][:, None] * uu[:, l][None, :]
    K = C - dot
    K = np.tril(K, -1)
    K = K + K.T
    K[np.diag_indices_from(K)] = sp["V"][cols]
    return K


def m_of(K, om):
    """M_jk = (omega_j K_jk) omega_k for j >= k, mirrored."""
    M = np.tril((om[:, None] * K) * om[None, :])
    return M + np.tril(M, -1).T


# ---- the tails -----------------------------------------------------------------------------------------------------------------------
def log_phi_neg(r):
    from scipy.special import log_ndtr
    return float(log_ndtr(-r))


def evaluate(lam, s):
    l1 = lam[0]
    g = g2 = 0.0
    for v in lam:
        mu = v / l1
        d = mu / (1.0 - mu * s)
        g = g + d
        g2 = g2 + d * d
    return g, g2


def root(lam, q):
    """(s_hat, converged, evaluations)."""
    s, lo, hi, n = 0.0, -math.inf, 1.0, 0
    tol = TOL_F * q
    while True:
        g, g2 = evaluate(lam, s)
        n += 1
        f = g - q
        if abs(f) <= tol:
            return s - f / g2, True, n
        if n == MAX_EVALS:
            return math.nan, False, n
        if f < 0:
            lo = s
        else:
            hi = s
        sn = s - f / g2
        if not (lo < sn < hi):
            if f < 0:
                sn = (s + hi) / 2
            else:
                sn = (lo + s) / 2 if math.isfinite(lo) else (2 * s if s < 0 else -1.0)
        s = sn


def skat_tail(lam, Q):
    """dict of state, neglog10p, t_hat, evals, w2 for eigenvalues lam (descending, clamped) and Q."""
    lam = [float(v) for v in lam]
    out = dict(state=0, neglog10p=math.nan, t_hat=math.nan, evals=0, w2=math.nan)
    m = len(lam)
    if m < 1 or not (lam[0] > 0.0) or not math.isfinite(lam[0]):
        return out
    l1 = lam[0]
    if m == 1 or lam[1] <= RANK_ONE * l1:
        out.update(state=2, neglog10p=float(S.neglog10p(np.float64(math.sqrt(Q) / math.sqrt(l1)))))
        return out
    if not Q > 0.0:
        out.update(state=4, neglog10p=0.0)
        return out
    q = Q / l1
    sh, conv, n = root(lam, q)
    out["evals"] = n
    s1 = s2 = s3 = 0.0
    for v in lam:
        mu = v / l1
        s1, s2, s3 = s1 + mu, s2 + mu * mu, s3 + (mu * mu) * mu
    if not conv:
        out.update(state=5, neglog10p=-log_phi_neg((q - s1) / math.sqrt(2.0 * s2)) / LN10)
        return out
    out["t_hat"] = sh / (2.0 * l1)
    g, g2 = evaluate(lam, sh)
    lg = 0.0
    for v in lam:
        lg = lg + math.log1p(-(v / l1) * sh)
    w2 = sh * q + lg
    out["w2"] = w2
    if not w2 >= NEAR_MEAN:
        out.update(state=3, neglog10p=-log_phi_neg((8.0 * s3 / (2.0 * s2) ** 1.5) / 6.0) / LN10)
        return out
    w = math.copysign(math.sqrt(w2), sh)
    v = sh * math.sqrt(g2 / 2.0)
    r = w + math.log(v / w) / w
    out.update(state=1, neglog10p=-log_phi_neg(r) / LN10, r=r)
    return out


def eigenvalues(M):
    lam = np.linalg.eigvalsh(M)[::-1].copy() if M.size else np.zeros(0)
    lam[lam <= 0.0] = 0.0
    return lam


# ---- the whole statement ---------------------------------------------------------------------------------------------------------------
def as_lists(sets, omega=None):
    """(set_ptr, set_col, omega) of a list of index arrays (omega: a list of arrays, None: ones)."""
    ptr = np.zeros(len(sets) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    col = np.concatenate([np.asarray(s, dtype=np.int32) for s in sets]) if sets else np.zeros(0, dtype=np.int32)
    om = np.ones(col.size) if omega is None else (np.concatenate([np.asarray(o, dtype=np.float64) for o in omega]) if sets else np.zeros(0))
    return ptr, col.astype(np.int32), om


def set_test(sp, w, sets, omega=None):
    """The statement on top of a plain spec sp (assoc_spec.score / score_dense with t = 1): dict of the per-set arrays m_used,
    burden_z, neglog10p_burden, skat_q, neglog10p_skat, skat_state, lambdas (laid out like set_col, NaN after m_used), cov (a list
    of m_s x m_s arrays over the entries, NaN in the rows and columns of non-members) and, per set, detail (members, K, M, lam, tail, T, S)."""
    ptr, col, om = as_lists(sets, omega)
    ns = len(sets)
    Um = sp["U"][:, 0]
    u = u_of(sp["b"], sp["Linv"])
    out = dict(m_used=np.zeros(ns, dtype=np.int32), burden_z=np.full(ns, np.nan), neglog10p_burden=np.full(ns, np.nan), skat_q=np.zeros(ns),
               neglog10p_skat=np.full(ns, np.nan), skat_state=np.zeros(ns, dtype=np.uint8), lambdas=np.full(col.size, np.nan), cov=[], detail=[])
    for s in range(ns):
        cols, oms = col[ptr[s]:ptr[s + 1]].astype(np.int64), om[ptr[s]:ptr[s + 1]]
        mem = members(sp, cols, oms)
        m = mem.size
        mc, mo = cols[mem], oms[mem]
        K = cov_members(sp, w, mc, u) if m else np.zeros((0, 0))
        M = m_of(K, mo) if m else K
        a = mo * Um[mc]
        T = 0.0
        Qs = 0.0
        for v in a:
            T = T + v
            Qs = Qs + v * v
        Ssum = 0.0
        for j in range(m):
            rs = 0.0
            for k in range(m):
                rs = rs + M[j, k]
            Ssum = Ssum + rs
        lam = eigenvalues(M)
        tl = skat_tail(lam, Qs)
        bz = T / math.sqrt(Ssum) if Ssum > 0.0 else math.nan
        out["m_used"][s], out["burden_z"][s], out["skat_q"][s] = m, bz, Qs
        out["neglog10p_burden"][s] = float(S.neglog10p(np.float64(bz)))
        out["neglog10p_skat"][s], out["skat_state"][s] = tl["neglog10p"], tl["state"]
        out["lambdas"][ptr[s]:ptr[s] + m] = lam
        full = np.full((cols.size, cols.size), np.nan)
        full[np.ix_(mem, mem)] = K
        out["cov"].append(full)
        out["detail"].append(dict(mem=mem, cols=mc, om=mo, K=K, M=M, lam=lam, tail=tl, T=T, S=Ssum, Q=Qs))
    return out


# ---- the margins of a clear decision -------------------------------------------------------------------------------------------------------
MIN_BURDEN_S = 1e-3


def clear(d):
    """Whether the spec's decisions on a set (its detail) leave the device no room to decide otherwise: lambda_2 / lambda_1 outside
    [2^-50, 2^-30] apart from exact rank one (m = 1), |w| outside [2^-30, 2^-10] (w^2 outside [2^-60, 2^-20]), at most 96
    evaluations, and S / sum sum |M_jk| >= 1e-3."""
    lam, tl = d["lam"], d["tail"]
    if lam.size == 0 or not lam[0] > 0:
        return True
    if lam.size > 1 and 2.0 ** -50 <= lam[1] / lam[0] <= 2.0 ** -30:
        return False
    if tl["evals"] > 96:
        return False
    if tl["state"] in (1, 3) and 2.0 ** -60 <= tl["w2"] <= 2.0 ** -20:
        return False
    return d["S"] / np.abs(d["M"]).sum() >= MIN_BURDEN_S


# ---- the bounds of the device's values --------------------------------------------------------------------------------------------------
def scan_bounds(sp, codes, flags, A, w, Z):
    """(dU, dV, du) per column (p) / (p x c) from the plain scan's bound (assoc_spec.bound and its parts): dU = dz sqrt(V);
    dV / V = dse / (2 se) (bound() forms dse = 2 (se dV / V + 3 u se)); u = Linv b through |L^-1|_2 = lmin^-1/2 with the relative
    perturbation of G and the chain of the fixed order, |du|_2 <= |db|_2 / sqrt(lmin) + (kappa eps_G + (c + 2) u) |u|_2."""
    X = sp["X"]
    n = X.shape[0]
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    A2 = np.asarray(A, dtype=np.float64).reshape(n, -1)
    Zm = np.asarray(Z, dtype=np.float64)
    c = Zm.shape[1]
    R = np.concatenate([A2, wv[:, None] * Zm], axis=1)
    dS = S._xtv_bound_dense(X, R) if codes is None else S._xtv_bound_snp(codes, flags, sp["stats"], R)
    db = dS[:, 1:]
    dz, _, dse = S.bound(sp, codes, flags, A, w, Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        dU = dz[:, 0] * np.sqrt(sp["V"])
        dV = sp["V"] * dse / (2 * sp["se"])
    ev = np.linalg.eigvalsh(sp["G"])
    lmin, kappa = float(ev[0]), float(ev[-1] / ev[0])
    eps_g = U * c * (n + 8 * c + 16)
    un = np.sqrt((u_of(sp["b"], sp["Linv"]) ** 2).sum(axis=1))
    du = np.sqrt((db * db).sum(axis=1)) / math.sqrt(lmin) + (kappa * eps_g + (c + 2) * U) * un
    return dU, dV, du, un


def cov_bound(sp, w, d, bounds):
    """dK (m x m) of a set: off the diagonal 2 (n u sum_i |w_i x~_ij x~_ik| + |u_j| du_k + |u_k| du_j + du_j du_k + (c + 2) u |u_j| |u_k|
    + u |K_jk|) -- the chain of n fused multiply-adds with one operand rounded, and the section-14 bound on u carried through the dot
    product; on the diagonal the scan's dV."""
    dU, dV, du, un = bounds
    cols = d["cols"]
    X = np.abs(sp["X"][:, cols])
    n = X.shape[0]
    wv = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    c = sp["b"].shape[1]
    absC = (X * wv[:, None]).T @ X
    uj, dj = un[cols], du[cols]
    dK = 2 * ((n + 2) * U * absC + uj[:, None] * dj[None, :] + dj[:, None] * uj[None, :] + dj[:, None] * dj[None, :]
              + (c + 2) * U * uj[:, None] * uj[None, :] + U * np.abs(d["K"]))
    dK[np.diag_indices_from(dK)] = dV[cols]
    return dK


def lambda_bound(d, dK):
    """|lambda_device - eigvalsh(M)| <= |dM|_F (Weyl) + 2 m u |M|_F, dM_jk = omega_j omega_k dK_jk + 2 u |M_jk|."""
    om = d["om"]
    dM = om[:, None] * om[None, :] * dK + 2 * U * np.abs(d["M"])
    return float(np.sqrt((dM * dM).sum()) + 2 * len(om) * U * np.sqrt((d["M"] ** 2).sum())), dM


def q_bound(sp, d, bounds):
    """|Q_device - Q|: dQ = sum omega_j^2 (2 |U_j| dU_j + dU_j^2) + (m + 2) u Q, doubled."""
    dU, cols, om = bounds[0], d["cols"], d["om"]
    return 2 * float((om * om * (2 * np.abs(sp["U"][cols, 0]) * dU[cols] + dU[cols] ** 2)).sum() + (len(cols) + 2) * U * d["Q"])


def device_tolerance(sp, d, bounds, dK):
    """(tol burden_z, tol neglog10p_burden, tol neglog10p_skat, dlam) of a set with members, from the spec alone.
    T: dT = sum omega_j dU_j + (m + 1) u sum |a_j|.  S: dS = sum sum dM_jk + (2 m + 3) u sum sum |M_jk|.  z = T / sqrt S:
    dz = dT / sqrt S + |z| dS / S + 3 u |z| (dS / S <= 1/2), doubled; its tail through the slope (|z| + 1 / |z|) / log 10 of the normal tail.
    Q: dQ = sum omega_j^2 (2 |U_j| dU_j + dU_j^2) + (m + 2) u Q.  SKAT, state 1: 16 SPEC_ERR |value| plus the first-order sensitivities
    d(-log p) / dQ = t_hat and d(-log p) / d lambda_i = -t_hat / (1 - 2 lambda_i t_hat), doubled for the prefactor; state 2:
    z = sqrt(Q / lambda_1), dz = z (dQ / (2 Q) + dlam / (2 lambda_1)) doubled, through the slope of the normal tail."""
    dU = bounds[0]
    cols, om, lam, tl = d["cols"], d["om"], d["lam"], d["tail"]
    m = len(cols)
    dlam, dM = lambda_bound(d, dK)
    a = np.abs(om * sp["U"][cols, 0])
    dT = float((om * dU[cols]).sum() + (m + 1) * U * a.sum())
    dS = float(dM.sum() + (2 * m + 3) * U * np.abs(d["M"]).sum())
    tz = tb = math.nan
    if d["S"] > 0:
        z = abs(d["T"]) / math.sqrt(d["S"])
        x = dS / d["S"]
        tz = 2 * (dT / math.sqrt(d["S"]) + z * x + 3 * U * z) if x <= 0.5 else math.inf
        tb = tz * (z + 1.0 / max(z, 1e-300)) / LN10 + 16 * S.U * 8
    dQ = q_bound(sp, d, bounds) / 2
    ts = math.nan
    if tl["state"] == 1:
        t = abs(tl["t_hat"])
        sens = t * dQ + float((t * dlam / (1.0 - 2.0 * lam * tl["t_hat"])).sum())
        ts = 16 * SPEC_ERR * abs(tl["neglog10p"]) + 2 * sens / LN10
    elif tl["state"] == 2:
        z = math.sqrt(d["Q"] / lam[0])
        dzz = 2 * z * (dQ / (2 * d["Q"]) + dlam / (2 * lam[0]) + 4 * U) if d["Q"] > 0 else math.inf
        ts = dzz * (z + 1.0 / max(z, 1e-300)) / LN10 + 16 * SPEC_ERR * abs(tl["neglog10p"])
    return tz, tb, ts, dlam


# ---- the inputs of the edge tests ----------------------------------------------------------------------------------------------------
EDGE_P = 150
EDGE_SIZES = (1, 2, 15, 16, 17, 33, 64, 65, 127, 128)
MAX_REDRAWN = 0.10
DUP = (10, 11)              # column 11 is made a copy of column 10: the duplicated-column set
# (source, n, c, missing share, flags, weights, seed).  n: fewer rows than one k-step and not a multiple of 4 (15), below the chunk
# (15), exactly one chunk (32), one chunk plus 1 (33), several chunks plus a tail (the rest).  "spa": the logistic null model of
# spa_spec.edge_inputs; "assoc": assoc_spec.edge_inputs with its weight kinds.
EDGE_CASES = (
    ("assoc", 15, 1, 0.0, (1, 1, 1), "none", 17000),
    ("assoc", 32, 2, 0.03, (1, 1, 0), "logistic", 17001),
    ("assoc", 33, 1, 0.0, (0, 0, 1), "ones", 17002),
    ("assoc", 63, 2, 0.03, (1, 0, 1), "zeros", 17003),
    ("spa", 64, 1, 0.03, (1, 1, 1), None, 17004),
    ("assoc", 65, 1, 0.03, (1, 1, 1), "outlier", 17005),
    ("assoc", 255, 5, 0.0, (1, 1, 0), "logistic", 17006),
    ("spa", 256, 2, 0.0, (0, 0, 1), None, 17007),
    ("assoc", 257, 2, 0.03, (1, 0, 1), "none", 17008),
    ("assoc", 513, 5, 0.03, (1, 1, 1), "zeros", 17009),
    ("spa", 1000, 5, 0.0, (1, 1, 0), None, 17010),
)


def null_inputs(case):
    """codes (n x 150, column 11 a copy of column 10), A (n), w (n or None), Z (n x c) of an edge case."""
    src, n, c, missing, flags, wk, seed = case
    if src == "spa":
        import spa_spec as P
        codes, y, eta, A, w, Z, _ = P.edge_inputs((n, EDGE_P, c, missing, flags, seed))
    else:
        codes, A, w, Z = S.edge_inputs((n, EDGE_P, 1, c, missing, flags, wk, seed))
        A = A[:, 0]
    codes = codes.copy()
    codes[:, DUP[1]] = codes[:, DUP[0]]
    return codes, np.ascontiguousarray(A), w, Z


def draw_sets(rng):
    """The sets of an edge case before the margins: one of every size in EDGE_SIZES (random columns, so the large ones overlap and
    hold the degenerate columns 3, 17 and 148), the set of the three degenerate columns alone, a set with a degenerate column, a
    set with an omega = 0 entry, the duplicated-column set, and a copy of the size-17 set at another position."""
    sets, omega = [], []
    for k in EDGE_SIZES:
        sets.append(np.sort(rng.choice(EDGE_P, k, replace=False)))
        omega.append(np.ones(k) if k in (1, 16, 128) else rng.uniform(0.5, 2.0, k))
    sets.append(np.array([3, 17, EDGE_P - 2])); omega.append(np.ones(3))
    sets.append(np.array([2, 3, 4, 5, 20])); omega.append(rng.uniform(0.5, 2.0, 5))
    sets.append(np.array([30, 31, 32, 33])); omega.append(np.array([1.0, 0.0, 2.0, 0.5]))
    sets.append(np.array(DUP)); omega.append(np.ones(2))
    sets.append(sets[4].copy()); omega.append(omega[4].copy())
    return sets, omega


FIXED_SETS = 5              # the last sets of draw_sets are not redrawn


def edge_inputs(case):
    """(codes, A, w, Z, sets, omega, sp, res, redrawn share): the inputs of an edge case with the spec's answer.  A random set
    whose decisions are not clear (clear()) is redrawn; the share of those among all drawn sets is returned."""
    codes, A, w, Z = null_inputs(case)
    flags = case[4]
    sp = S.score(codes, flags, A, w, Z)
    rng = np.random.default_rng(case[6] + 500)
    sets, omega = draw_sets(rng)
    drawn = unclear = 0
    for s in range(len(sets)):
        for _ in range(50):
            drawn += 1
            res = set_test(sp, w, [sets[s]], [omega[s]])
            if clear(res["detail"][0]):
                break
            assert s < len(sets) - FIXED_SETS, ("a fixed set without a clear decision", case, s)
            unclear += 1
            sets[s] = np.sort(rng.choice(EDGE_P, len(sets[s]), replace=False))
        else:
            raise AssertionError(("no set with a clear decision", case, s))
    sets[-1], omega[-1] = sets[4].copy(), omega[4].copy()
    res = set_test(sp, w, sets, omega)
    return codes, A, w, Z, sets, omega, sp, res, unclear / max(drawn, 1)
