"""The numpy statement of SKAT-O, the optimal combination of the burden and the SKAT test of a variant set (csrc/assoc_skato.hip and
csrc/skato_tail.h: mih_assoc_sets_skato; skato=True of set_test, assoc_sets and gwas_sets).  It builds on tests/sets_spec.py, whose
members, M, a = omega U, T, S, Q, eigenvalues and Kuonen tail (skat_tail) it takes as they are.

Over the m members of a set, with rs_j = sum_k M_jk (k ascending) and a grid rho_1 < ... < rho_R in [0, 1], R <= 16 (the default
is SKAT's optimal.adj grid; a value above 0.999 is used as 0.999):
    Q_rho    = (1 - rho) Q + rho (T T)
    M_rho    = R_rho^1/2 M R_rho^1/2,  R_rho = (1 - rho) I + rho 11',  in closed form: with c = sqrt(1 - rho) and
               d = (sqrt((1 - rho) + m rho) - c) / m,  M_rho[j, k] = ((c c) M_jk + (c d) (rs_j + rs_k)) + (d d) S  for j >= k, mirrored.
               At rho = 0: c = 1 and d = 0 exactly, so M_0 = M to the bit (a -0.0 becomes +0.0: no eigenvalue changes).
    lambda^(rho)  the eigenvalues of M_rho, descending, every value <= 0 set to 0;  p_rho the Kuonen tail of (lambda^(rho), Q_rho)
    p_min    = min_rho p_rho, skato_rho its rho (a tie goes to the smaller rho)
    q_rho    the quantile: tail_rho(q_rho) = p_min.  For skato_rho it is Q_rho itself.  For a rank-one lambda^(rho) (state 2) it is
               lambda_1 z^2 with z the two-sided normal quantile of p_min.  Otherwise the saddlepoint is inverted in its own
               parameter s = 2 lambda_1 t < 1:  q(s) = lambda_1 g(s),  log tail(s) = log Phi(-r(s)),  r increasing in s (quantile()).
    M~       = M - rs rs' / S  (entry j >= k: M_jk - (rs_j rs_k) / S, mirrored), its eigenvalues lambda~ (values <= 0 set to 0)
    mu = sum lambda~,  v_xi = 4 (rs' M~ rs) / S (not below 0),  v = 2 sum lambda~^2 + v_xi,  tau_rho = rho S + (1 - rho) (rs' rs) / S
    delta(x) = min_rho (q_rho - tau_rho x) / (1 - rho),   delta'(x) = (delta(x) - mu) sqrt((v - v_xi) / v) + mu
    u0^2     = min_rho q_rho / tau_rho
    p        = 2 int_0^u0 S~(delta'(u^2)) phi(u) du + 2 Phi(-u0),   S~ the Kuonen tail of lambda~, S~ = 1 where delta' <= 0.
The integral is a fixed composite Gauss-Legendre rule, 16 panels of [0, u0] with 16 nodes each, every term as a logarithm
(log weight + log S~ + log phi + log(h / 2), h the width of the panel), combined by the fixed pairwise log-sum-exp tree of the
device (term t = 16 panel + node; for k = 128, 64, ..., 1: term[t] = lse(term[t], term[t + k]), t < k).  delta has up to R - 1 kinks
where the minimising rho changes (kinks()); the panels are cut there (panel_edges()): with 16 equal panels the rule loses ten
digits on them (cut=False, for the measurement in tests/test_skato_spec_cpu.py only).

The quantile iteration, in y = 1 / (1 - s) (q and the log tail are close to linear in y), F(y) = log tail(1 - 1 / y) - log p_min:
    a = 1 / (1 - s_rho), s_rho the saddlepoint of Q_rho (F(a) >= 0 up to rounding: p_rho >= p_min); evaluate F(a).
    |F(a)| <= 2^-40 |log p_min|, or F(a) < 0: take a.  Otherwise b = 2 a, and while F(b) > 0: a = b, b = 2 b.
    Then the Illinois rule: y = b - F(b) (b - a) / (F(b) - F(a)), the midpoint if that is not inside (a, b); evaluate F(y);
    |F(y)| <= 2^-40 |log p_min|: converged.  F(y) > 0: a = y (and F(b) is halved if a moved last time too), else b = y (and F(a) is
    halved likewise).  b - a <= 2^-40 b: converged too, with the last y (near the mean the rounding of w^2 = s q + sum log1p(-mu s)
    leaves F a noise above the first tolerance).  128 evaluations of F in all: not converged -- the set falls back.

skato_state:  0 no value: m = 0, S <= 0 (or NaN), SKAT state 0, or some p_rho without a value.
              2 rank one: m = 1 or SKAT state 2: the value is neglog10p_skat bit for bit.
              4 fallback: some p_rho came from state 4 (Q_rho <= 0) or 5 (not converged), a quantile did not converge, or the
                integral is not a number: the value is min(1, R p_min).
              1 the integral's value.
              3 clamped: the integral left [p_min, R p_min] and was moved to the nearer end (SKAT's own rule)."""
import math

import numpy as np

import assoc_spec as S
import sets_spec as T

LN10 = math.log(10.0)
DEFAULT_GRID = (0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0)
RHO_CAP = 0.999
MAX_RHO = 16
PANELS = 16
NODES = 16
GL_X, GL_W = np.polynomial.legendre.leggauss(NODES)
TOL_P = 2.0 ** -40
MAX_EVALS = 128
NONE, INTEGRAL, RANK_ONE, CLAMPED, FALLBACK = 0, 1, 2, 3, 4
MARGIN = 1e-6               # the redraw rule: a decision closer than this (relative, in p) is not clear
# The spec's own relative error in log p against the same formulas in 50-digit mpmath (eigenvalues by mpmath.eigsy, the quantiles by
# bisection on the tail, the integral by mpmath.quad split at the kinks), measured on ALL sets of tests/test_gpu_assoc_skato.py's
# 2-bit cases with an integral and at most 17 members (30 sets: the four cases with the default grid, the first with 16 values);
# tests/test_skato_spec_cpu.py measures it again on a share of them, the worst among them, and holds the spec to twice this
# figure.  The worst is the omega = 0 set of the n = 1000 case; the median is 1.5e-14.
SPEC_ERR_O = 5.2e-12
# The same with 16 equal panels, not cut at the kinks of delta: what the cut buys (the quadrature's share of the error)
SPEC_ERR_O_EQUAL_PANELS = 1.7e-4

def grid_of(rho=None):
    g = np.asarray(DEFAULT_GRID if rho is None else rho, dtype=np.float64).reshape(-1)
    assert 1 <= g.size <= MAX_RHO and (g >= 0).all() and (g <= 1).all() and (np.diff(g) > 0).all()
    return np.minimum(g, RHO_CAP)


def row_sums(M):
    rs = np.zeros(M.shape[0])
    for k in range(M.shape[0]):
        rs = rs + M[:, k]
    return rs


def m_rho(M, rs, Ssum, rho):
    m = M.shape[0]
    c = math.sqrt(1.0 - rho)
    d = (math.sqrt((1.0 - rho) + m * rho) - c) / m
    A = np.tril(((c * c) * M + (c * d) * (rs[:, None] + rs[None, :])) + (d * d) * Ssum)
    return A + np.tril(A, -1).T


def m_tilde(M, rs, Ssum):
    A = np.tril(M - (rs[:, None] * rs[None, :]) / Ssum)
    return A + np.tril(A, -1).T


def dot_fixed(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s = s + x * y
    return s


# ---- the quantiles ---------------------------------------------------------------------------------------------------------------------
def tail_of_s(lam, s):
    """(q, log tail) at the saddlepoint parameter s of eigenvalues lam."""
    l1 = lam[0]
    g, g2 = T.evaluate(lam, s)
    lg = s2 = s3 = 0.0
    for v in lam:
        mu = v / l1
        lg = lg + math.log1p(-mu * s)
        s2, s3 = s2 + mu * mu, s3 + (mu * mu) * mu
    w2 = s * g + lg
    if not w2 >= T.NEAR_MEAN:
        r = (8.0 * s3 / (2.0 * s2) ** 1.5) / 6.0
    else:
        w = math.copysign(math.sqrt(w2), s)
        r = w + math.log((s * math.sqrt(g2 / 2.0)) / w) / w
    return l1 * g, T.log_phi_neg(r)


def quantile(lam, s0, logp):
    """(q, converged, evaluations): the q with log tail(q) = logp, from the saddlepoint s0 of a Q whose tail is not below it."""
    lam = [float(v) for v in lam]
    tol = TOL_P * abs(logp)
    n = 0

    def F(y):
        nonlocal n
        n += 1
        q, lt = tail_of_s(lam, 1.0 - 1.0 / y)
        return q, lt - logp

    a = 1.0 / (1.0 - s0)
    qa, Fa = F(a)
    if abs(Fa) <= tol or Fa < 0:
        return qa, True, n
    b = 2.0 * a
    qb, Fb = F(b)
    while Fb > 0:
        if n >= MAX_EVALS:
            return math.nan, False, n
        a, Fa, b = b, Fb, 2.0 * b
        qb, Fb = F(b)
    if abs(Fb) <= tol:
        return qb, True, n
    side = 0
    while True:
        if n >= MAX_EVALS:
            return math.nan, False, n
        y = b - Fb * (b - a) / (Fb - Fa)
        if not (a < y < b):
            y = (a + b) / 2
        qy, Fy = F(y)
        if abs(Fy) <= tol:
            return qy, True, n
        if Fy > 0:
            a, Fa = y, Fy
            if side == 1:
                Fb = Fb / 2
            side = 1
        else:
            b, Fb = y, Fy
            if side == -1:
                Fa = Fa / 2
            side = -1
        if b - a <= TOL_P * b:
            return qy, True, n


def chi1_quantile(l1, nlp):
    """lambda_1 z^2 with neglog10p(z) = nlp."""
    from scipy.special import ndtri_exp
    z = -float(ndtri_exp(-nlp * LN10 - math.log(2.0)))
    return l1 * (z * z)


# ---- the integral ----------------------------------------------------------------------------------------------------------------------
def lse(a, b):
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        out = hi + np.log1p(np.exp(lo - hi))
    out = np.where(np.isneginf(hi), hi, out)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, out)


def log_s_tilde(lam_t, dp):
    if not dp > 0.0:
        return 0.0 if dp <= 0.0 else math.nan
    return -T.skat_tail(lam_t, dp)["neglog10p"] * LN10


def delta_prime(x, q, tau, grid, mu, kfac):
    d = min((q[r] - tau[r] * x) / (1.0 - grid[r]) for r in range(len(grid)))
    return (d - mu) * kfac + mu


def kinks(q, tau, grid, x0):
    """The x in (0, x0) where the minimising line of delta(x) = min_rho (a_rho - b_rho x), a = q / (1 - rho), b = tau / (1 - rho),
    changes, ascending -- at most R - 1.  A walk along the lower envelope: from the line that is lowest at x = 0 (the steepest
    among equals), the next kink is the nearest crossing ahead with a steeper line (the steepest among equals), until x0."""
    R = len(grid)
    a = [q[r] / (1.0 - grid[r]) for r in range(R)]
    b = [tau[r] / (1.0 - grid[r]) for r in range(R)]
    cur = 0
    for r in range(1, R):
        if a[r] < a[cur] or (a[r] == a[cur] and b[r] > b[cur]):
            cur = r
    x, out = 0.0, []
    for _ in range(R - 1):
        nxt, xn = -1, x0
        for r in range(R):
            if b[r] > b[cur]:
                xc = (a[r] - a[cur]) / (b[r] - b[cur])
                if xc > x and (xc < xn or (xc == xn and nxt >= 0 and b[r] > b[nxt])):
                    nxt, xn = r, xc
        if nxt < 0:
            break
        out.append(xn)
        cur, x = nxt, xn
    return out


def panel_edges(q, tau, grid, u0, cut=True):
    """The PANELS + 1 edges of the panels in u.  The segments between 0, the kinks (as u = sqrt x) and u0 get one panel each, and
    the remaining panels go one at a time to the segment whose panels are widest (the first among equals); a segment's panels are
    equal: edge = lo + (hi - lo) i / k.  cut=False: PANELS equal panels of [0, u0]."""
    pts = [0.0] + ([math.sqrt(x) for x in kinks(q, tau, grid, u0 * u0)] if cut else []) + [u0]
    n = [1] * (len(pts) - 1)
    for _ in range(PANELS - len(n)):
        best = 0
        for i in range(1, len(n)):
            if (pts[i + 1] - pts[i]) / n[i] > (pts[best + 1] - pts[best]) / n[best]:
                best = i
        n[best] += 1
    edges = []
    for i in range(len(n)):
        edges += [pts[i] + (pts[i + 1] - pts[i]) * j / n[i] for j in range(n[i])]
    return edges + [u0]


def integral(lam_t, q, tau, grid, mu, kfac, u0, cut=True):
    """log of 2 int_0^u0 S~(delta'(u^2)) phi(u) du."""
    edges = panel_edges(q, tau, grid, u0, cut)
    terms = np.zeros(PANELS * NODES)
    for t in range(PANELS * NODES):
        pnl, nd = divmod(t, NODES)
        h = edges[pnl + 1] - edges[pnl]
        u = edges[pnl] + h * ((GL_X[nd] + 1.0) / 2.0)
        ls = log_s_tilde(lam_t, delta_prime(u * u, q, tau, grid, mu, kfac))
        with np.errstate(divide="ignore"):
            terms[t] = ((math.log(GL_W[nd]) + ls) + (-(u * u) / 2.0 - 0.9189385332046727)) + float(np.log(h / 2.0))
    k = PANELS * NODES // 2
    while k > 0:
        terms[:k] = lse(terms[:k], terms[k:2 * k])
        k //= 2
    return float(terms[0]) + math.log(2.0)


# ---- a set -------------------------------------------------------------------------------------------------------------------------------
def evaluate(m, lam_rho, lam_t, Q, Tt, rr, wt, Ssum, grid, skat, cut=True):
    """SKAT-O of one set from its numbers: lam_rho (R arrays), lam_t, Q, T, rr = rs' rs, wt = rs' M~ rs, S, the grid (capped), and
    skat = (neglog10p_skat, skat_state) of the set.  dict of state, neglog10p, rho (index), nlp_rho, st_rho, q, tau, mu, v, v_xi, u0,
    nlp_int (the integral's value before the clamp), margin (the closest decision, relative in p)."""
    R = len(grid)
    out = dict(state=NONE, neglog10p=math.nan, rho=-1, nlp_rho=np.full(R, np.nan), st_rho=np.zeros(R, dtype=np.int64), margin=math.inf, nlp_int=math.nan)
    if m < 1:
        return out
    tails = []
    for r in range(R):
        rho = float(grid[r])
        tl = T.skat_tail(lam_rho[r], (1.0 - rho) * Q + rho * (Tt * Tt))
        tails.append(tl)
        out["nlp_rho"][r], out["st_rho"][r] = tl["neglog10p"], tl["state"]
    if not Ssum > 0.0 or skat[1] == 0 or (out["st_rho"] == 0).any():
        return out
    if m == 1 or skat[1] == 2:
        out.update(state=RANK_ONE, neglog10p=skat[0])
        return out
    nlp = out["nlp_rho"]
    best = 0
    for r in range(1, R):
        if nlp[r] > nlp[best]:
            best = r
    out["rho"] = best
    pmin = nlp[best]
    srt = np.sort(nlp)[::-1]
    if R > 1:
        out["margin"] = abs(srt[0] - srt[1]) * LN10
    fallback = max(0.0, pmin - math.log10(R))
    if ((out["st_rho"] == 4) | (out["st_rho"] == 5)).any() or not pmin > 0.0:
        out.update(state=FALLBACK, neglog10p=fallback)
        return out
    logp = -pmin * LN10
    q, tau = np.zeros(R), np.zeros(R)
    for r in range(R):
        rho = float(grid[r])
        tau[r] = rho * Ssum + (1.0 - rho) * rr / Ssum
        l1 = float(lam_rho[r][0])
        if r == best:
            q[r] = (1.0 - rho) * Q + rho * (Tt * Tt)
        elif out["st_rho"][r] == 2:
            q[r] = chi1_quantile(l1, pmin)
        else:
            q[r], ok, _ = quantile(lam_rho[r], tails[r]["t_hat"] * (2.0 * l1), logp)
            if not ok:
                out.update(state=FALLBACK, neglog10p=fallback)
                return out
    mu = s2 = 0.0
    for v in lam_t:
        mu, s2 = mu + v, s2 + v * v
    vxi = max(4.0 * wt / Ssum, 0.0)
    v = 2.0 * s2 + vxi
    kfac = math.sqrt((v - vxi) / v)
    u0 = math.sqrt(min(q[r] / tau[r] for r in range(R)))
    out.update(q=q, tau=tau, mu=mu, v=v, v_xi=vxi, u0=u0)
    li = integral(lam_t, q, tau, grid, mu, kfac, u0, cut)
    lp = float(lse(li, math.log(2.0) + T.log_phi_neg(u0)))
    val = -lp / LN10
    out["nlp_int"] = val
    if math.isnan(val):
        out.update(state=FALLBACK, neglog10p=fallback)
        return out
    out["margin"] = min(out["margin"], abs(val - pmin) * LN10, abs(val - (pmin - math.log10(R))) * LN10)
    if val > pmin:
        out.update(state=CLAMPED, neglog10p=pmin)
    elif val < pmin - math.log10(R):
        out.update(state=CLAMPED, neglog10p=max(0.0, pmin - math.log10(R)))
    else:
        out.update(state=INTEGRAL, neglog10p=max(0.0, val))
    return out


def parts(d, grid):
    """What evaluate() takes, from a set's detail of sets_spec.set_test: dict of m, rs, M_rho (R matrices), Mt, lam_rho, lam_t, rr, wt."""
    M = d["M"]
    m = M.shape[0]
    if m == 0:
        return dict(m=0, rs=np.zeros(0), M_rho=[M] * len(grid), Mt=M, lam_rho=[np.zeros(0)] * len(grid), lam_t=np.zeros(0), rr=0.0, wt=0.0)
    rs = row_sums(M)
    Mr = [m_rho(M, rs, d["S"], float(r)) for r in grid]
    with np.errstate(all="ignore"):
        Mt = m_tilde(M, rs, d["S"])
    ok = np.isfinite(Mt).all()
    lam_t = T.eigenvalues(Mt) if ok else np.full(m, np.nan)
    wt = dot_fixed(rs, [dot_fixed(Mt[j], rs) for j in range(m)]) if ok else math.nan
    return dict(m=m, rs=rs, M_rho=Mr, Mt=Mt, lam_rho=[T.eigenvalues(A) for A in Mr], lam_t=lam_t, rr=dot_fixed(rs, rs), wt=wt)


def set_skato(d, grid, cut=True):
    """SKAT-O of a set from its detail; returns (evaluate()'s dict, parts()'s dict)."""
    p = parts(d, grid)
    ev = evaluate(p["m"], p["lam_rho"], p["lam_t"], d["Q"], d["T"], p["rr"], p["wt"], d["S"], grid, (d["tail"]["neglog10p"], d["tail"]["state"]), cut)
    return ev, p


def clear(ev):
    return ev["state"] in (NONE, RANK_ONE) or ev["margin"] >= MARGIN


# ---- the bounds of the device's values --------------------------------------------------------------------------------------------------
def lambda_rho_bounds(d, dK, grid):
    """|lambda_rho_device - eigvalsh(M_rho)| per grid value, and last for M~: sets_spec.lambda_bound's rule (Weyl on the
    perturbation of the matrix plus the Jacobi's 2 m u |.|_F) applied to M_rho and M~.  The device forms both from ITS M, so its
    matrices are the exact maps of M + dM plus the rounding of the entries:  |R^1/2 dM R^1/2|_F <= |R_rho|_2 |dM|_F =
    ((1 - rho) + m rho) |dM|_F;  M~ = M - M J M / S, J = 11':  |dM~|_F <= |dM|_F (1 + 2 sqrt(m) |rs|_2 / S + m |rs|_2^2 / S^2)
    (|dM J M|_F <= sqrt(m) |dM|_F |rs|_2, |dS| <= m |dM|_F).  Rounding: rs_j carries (m + 1) u sum_k |M_jk|, S twice that, each
    entry four more operations: (3 m + 10) u on the sums of the absolute terms, and for rs_j rs_k / S the relative
    (2 m + 4 + 2 m sum|M| / S) u."""
    M, m = d["M"], d["M"].shape[0]
    _, dM = T.lambda_bound(d, dK)
    fdM = float(np.sqrt((dM * dM).sum()))
    ars = np.abs(M).sum(axis=1)
    aS = float(ars.sum())
    rs = row_sums(M)
    out = []
    for rho in grid:
        c = math.sqrt(1.0 - rho)
        dd = (math.sqrt((1.0 - rho) + m * rho) - c) / m
        absM = c * c * np.abs(M) + c * dd * (ars[:, None] + ars[None, :]) + dd * dd * aS
        out.append(((1.0 - rho) + m * rho) * fdM + (5 * m + 10) * T.U * float(np.sqrt((absM * absM).sum())))
    Ss = d["S"]
    nrs = float(np.sqrt((rs * rs).sum()))
    outer = ars[:, None] * ars[None, :] / Ss
    absT = np.abs(M) + outer
    amp = 1.0 + 2.0 * math.sqrt(m) * nrs / Ss + m * nrs * nrs / (Ss * Ss)
    out.append(amp * fdM + T.U * ((2 * m + 8) * float(np.sqrt((absT * absT).sum())) + (2 * m + 4 + 2 * m * aS / Ss) * float(np.sqrt((outer * outer).sum()))))
    return out, dM, amp * fdM


def device_tolerance(sp, d, bounds, dK, grid, ev, p):
    """(tolerance of neglog10p_skato, the bounds of lambda_rho) of a set in the integral, clamped or fallback state, from the spec
    alone: 16 SPEC_ERR_O |value| plus the change of the spec's own value when its inputs move by the device's bounds -- two
    perturbed evaluations, one with every input moved towards a smaller p (Q + dQ, |T| + dT, every eigenvalue down by its bound, S,
    rs' rs and rs' M~ rs down), one the other way.  dT, dS, dQ are sets_spec.device_tolerance's; rs_j moves by sum_k dM_jk +
    (m + 1) u sum_k |M_jk|, rs' M~ rs by that through both factors plus |rs|^2 |dM~|_F."""
    dU = bounds[0]
    cols, om = d["cols"], d["om"]
    m = len(cols)
    dl, dM, dMt = lambda_rho_bounds(d, dK, grid)
    a = np.abs(om * sp["U"][cols, 0])
    dT = float((om * dU[cols]).sum() + (m + 1) * T.U * a.sum())
    dS = float(dM.sum() + (2 * m + 3) * T.U * np.abs(d["M"]).sum())
    dQ = T.q_bound(sp, d, bounds)
    drs = dM.sum(axis=1) + (m + 1) * T.U * np.abs(d["M"]).sum(axis=1)
    rs, Mt = p["rs"], p["Mt"]
    vals = []
    for sg in (1.0, -1.0):
        lr = [np.maximum(p["lam_rho"][r] - sg * dl[r], 0.0) for r in range(len(grid))]
        lt = np.maximum(p["lam_t"] - sg * dl[-1], 0.0)
        rs2 = rs - sg * np.sign(rs) * np.minimum(drs, np.abs(rs))
        wt = dot_fixed(rs2, Mt @ rs2) - sg * float((rs * rs).sum()) * dMt
        e2 = evaluate(m, lr, lt, max(d["Q"] + sg * dQ, 0.0), math.copysign(max(abs(d["T"]) + sg * dT, 0.0), d["T"]), dot_fixed(rs2, rs2), wt,
                      d["S"] - sg * dS, grid, (d["tail"]["neglog10p"], d["tail"]["state"]))
        vals.append(e2["neglog10p"])
    change = max(abs(v - ev["neglog10p"]) for v in vals)
    return 16 * SPEC_ERR_O * abs(ev["neglog10p"]) + change, dl


# ---- the inputs of the device tests ------------------------------------------------------------------------------------------------------
GRID16 = tuple((k / 15.0) ** 2 for k in range(16))
SIZES = (1, 2, 3, 17, 64, 65, 128)
SIGN_SET = np.arange(40, 48)                    # the set whose scores a "same" / "alt" case gives one sign / alternating signs
MAX_REDRAWN = 0.10
# (source, n, c, missing share, flags, weights, seed) as sets_spec.EDGE_CASES, then the scores: "drawn", "same", "alt"
CASES = (
    ("assoc", 257, 2, 0.03, (1, 0, 1), "none", 17008, "drawn"),
    ("assoc", 1000, 2, 0.03, (1, 1, 1), "logistic", 18001, "drawn"),
    ("assoc", 257, 2, 0.03, (1, 0, 1), "none", 17008, "same"),
    ("assoc", 257, 2, 0.03, (1, 0, 1), "none", 17008, "alt"),
)


def draw_sets(rng):
    """One set of every size in SIZES (random columns among those that are neither degenerate nor the duplicate, so that every
    entry is a member: 64 members is the last LDS order, 65 the first with slabs, 128 the limit), a set with a degenerate column
    (3), a set with an omega = 0 entry, the set of the three degenerate columns (no members) and the sign set."""
    sets, omega = [], []
    for k in SIZES:
        sets.append(np.sort(rng.choice(GOOD, k, replace=False)))
        omega.append(np.ones(k) if k in (1, 128) else rng.uniform(0.5, 2.0, k))
    sets.append(np.array([2, 3, 4, 5, 20])); omega.append(rng.uniform(0.5, 2.0, 5))
    sets.append(np.array([30, 31, 32, 33])); omega.append(np.array([1.0, 0.0, 2.0, 0.5]))
    sets.append(np.array([3, 17, T.EDGE_P - 2])); omega.append(np.ones(3))
    sets.append(SIGN_SET.copy()); omega.append(np.ones(SIGN_SET.size))
    return sets, omega


GOOD = np.setdiff1d(np.arange(T.EDGE_P), [3, 17, T.EDGE_P - 2, T.DUP[1]])
FIXED_SETS = 4


def inputs(case, grid=None):
    """(codes, A, w, Z, sets, omega, sp, res, sk, redrawn share): the inputs of a case, sets_spec.set_test's answer res and, per
    set, sk = (evaluate()'s dict, parts()'s dict).  A drawn set whose decisions are not clear -- sets_spec.clear, or two p_rho or
    the clamp closer than MARGIN -- is redrawn."""
    grid = grid_of(grid)
    codes, A, w, Z = T.null_inputs(case[:7])
    flags = case[4]
    if case[7] != "drawn":                       # scores along the sign set's columns: A = 0.12 X~ sgn, projected off the covariates
        X = S.score(codes, flags, A, w, Z)["X"]
        sgn = np.ones(SIGN_SET.size) if case[7] == "same" else (-1.0) ** np.arange(SIGN_SET.size)
        A = 0.12 * (X[:, SIGN_SET] @ sgn) + 0.05 * np.random.default_rng(case[6] + 7).standard_normal(X.shape[0])
        wz = Z if w is None else w[:, None] * Z
        A = np.ascontiguousarray(A - wz @ np.linalg.solve(Z.T @ wz, Z.T @ A))
    sp = S.score(codes, flags, A, w, Z)
    rng = np.random.default_rng(case[6] + 900)
    sets, omega = draw_sets(rng)
    drawn = unclear = 0
    for s in range(len(sets)):
        for _ in range(50):
            drawn += 1
            d = T.set_test(sp, w, [sets[s]], [omega[s]])["detail"][0]
            if T.clear(d) and clear(set_skato(d, grid)[0]):
                break
            assert s < len(sets) - FIXED_SETS, ("a fixed set without a clear decision", case, s)
            unclear += 1
            sets[s] = np.sort(rng.choice(GOOD, len(sets[s]), replace=False))
        else:
            raise AssertionError(("no set with a clear decision", case, s))
    res = T.set_test(sp, w, sets, omega)
    sk = [set_skato(d, grid) for d in res["detail"]]
    return codes, A, w, Z, sets, omega, sp, res, sk, unclear / max(drawn, 1)
