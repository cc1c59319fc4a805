"""The numpy statement of the saddlepoint-corrected p-value of the case-control association scan (csrc/assoc_spa.hip:
mih_assoc_score_spa; score_test_spa and assoc(..., spa=True) of the matrix classes).  It is the yardstick of the device path and
builds on tests/assoc_spec.py, whose U, b, V, z and degenerate-column rule it takes as they are.

One Bernoulli trait, logit link.  h_i = eta_i is the null model's linear predictor, mu_i = sigma(h_i).  Per column j
    u = Linv b_j (u_k = sum_{l <= k} Linv[k, l] b_l, l ascending),   alpha_k = sum_{l >= k} Linv[l, k] u_l (l ascending)   (= G^-1 b_j)
    c_i = x_ij - sum_k Z_ik alpha_k          (the sum from 0.0 with k ascending, every operation rounded by itself: float64)
    K(t)   = sum_i [softplus(h_i + c_i t) - softplus(h_i)] - t M1,      M1 = sum_i c_i mu_i
    K'(t)  = sum_i c_i [sigma(h_i + c_i t) - mu_i]
    K''(t) = sum_i c_i^2 sigma(h_i + c_i t) (1 - sigma(h_i + c_i t))
with, for x = h_i + c_i t (one product, one sum), e = exp(-|x|), r = 1 / (1 + e):
    sigma(x) = r (x >= 0), e r (x < 0);   sigma (1 - sigma) = (e r) r;   softplus(x) = max(x, 0) + log1p(e);
mu_i is sigma(h_i) by the same expressions, so every term of K'(0) is exactly 0.  q = U_j.  The range of the statistic:
    S_min = sum_i min(c_i, 0) - M1,   S_max = sum_i max(c_i, 0) - M1.

The root of K'(t) = s (root()):  t = 0, lo = -inf, hi = +inf, no evaluations yet.  Repeat:
    evaluate K'(t), K''(t) (one evaluation); f = K'(t) - s
    |f| <= 2^-30 sqrt(V_j): converged; t_hat = t - f / K''(t) (one more Newton step, taken as it is) -- stop
    64 evaluations made: not converged -- stop
    f < 0: lo = t, else hi = t
    tn = t - f / K''(t); if not lo < tn < hi (a NaN is not):
        f < 0: tn = (t + hi) / 2 if hi is finite, else 2 t if t > 0, else 1
        f > 0: tn = (lo + t) / 2 if lo is finite, else 2 t if t < 0, else -1
    t = tn
(t, lo, hi, f and the comparisons in float64.)  K and K'' at t_hat take one more pass over the rows (the only one with log1p).

A tail at target s (tail()):  w = sign(t_hat) sqrt(2 (t_hat s - K)), v = t_hat sqrt(K''), r = w + log(v / w) / w, the tail
log Phi(-|r|).  It is ACCEPTED when the iteration converged, t_hat is finite, K''(t_hat) >= 2^-20 V_j, and r is finite and not
zero with the sign of t_hat.  (The third condition: with every carrier a case the statistic sits at the end of its range, K'
approaches s only as t -> infinity, the float iteration "converges" at t ~ 1e3 with K'' / V ~ 1e-11 and r means nothing.)

The column (spa()):  state 0 -- degenerate, or |z_j| < cutoff (z_j = 0 with cutoff = 0 is tried and refused: s = 0 gives w = 0):
neglog10p_spa = neglog10p.  Otherwise tail 0 has target +|q| and tail 1 has -|q|; the observed side (the sign of q) is always
computed; the other one contributes exactly 0 -- and is not computed -- if its target is >= S_max (tail 0) or <= S_min (tail 1).
Every computed tail accepted: state 1, neglog10p_spa = -log10(exp(l_0) + exp(l_1)) as m + log1p(exp(l_min - m)), m the larger.
Any computed tail refused: state 2, neglog10p_spa = neglog10p.  t_hat is p x 2 (tail 0, tail 1), NaN where a tail was not
computed or did not converge.

The sums over the rows are evaluated in numpy longdouble (the terms too) and rounded once, so that the spec's own error is far
below the device's: the device sums float64 terms per thread in row order (rows tid, tid + 256, ...) and then over a fixed tree.
The control values and the finish are float64 on both sides."""
import math

import numpy as np

import assoc_spec as S

LD = np.longdouble
TOL_F = 2.0 ** -30          # |K'(t) - s| <= TOL_F sqrt(V)
MIN_K2 = 2.0 ** -20         # K''(t_hat) >= MIN_K2 V
MAX_EVALS = 64
# The spec's own relative error in log p against 40-digit mpmath, measured on the inputs of tests/test_gpu_assoc_spa.py
# (tests/test_spa_spec_cpu.py measures it again on a share of them and holds it to this figure): the yardstick of the device
# tolerance, see device_tolerance().
SPEC_ERR = 8.25e-16         # (548 + 19 tried columns, the worst at case (256, 150, 5, ...), column 7)


# ---- the functions of a column -----------------------------------------------------------------------------------------------------
def alpha_of(b, Linv):
    """alpha = Linv' (Linv b) per row of b (p x c) in the fixed order of the module docstring."""
    p, c = b.shape
    u = np.zeros((p, c))
    for k in range(c):
        a = np.zeros(p)
        for l in range(k + 1):
            a = a + Linv[k, l] * b[:, l]
        u[:, k] = a
    al = np.zeros((p, c))
    for k in range(c):
        a = np.zeros(p)
        for l in range(k, c):
            a = a + Linv[l, k] * u[:, l]
        al[:, k] = a
    return al


def adjusted(x, Z, alpha):
    """c_i = x_i - sum_k Z_ik alpha_k, float64, k ascending."""
    a = np.zeros(x.shape[0])
    for k in range(Z.shape[1]):
        a = a + Z[:, k] * alpha[k]
    return x - a


def _parts(x):
    e = np.exp(-np.abs(x))
    r = 1.0 / (1.0 + e)
    return e, r


def sigma(x):
    e, r = _parts(x)
    return np.where(x >= 0, r, e * r)


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


class Column:
    """The cumulant generating function of one column: c (float64), h = eta; the sums in longdouble, rounded once."""
    def __init__(self, c, h):
        self.c, self.h = LD(c), LD(h)
        self.mu = sigma(self.h)
        self.m1 = float(np.sum(self.c * self.mu))
        m1 = np.sum(self.c * self.mu)
        self.smin = float(np.sum(np.minimum(self.c, 0)) - m1)
        self.smax = float(np.sum(np.maximum(self.c, 0)) - m1)
        self.evals = 0

    def k12(self, t):
        x = self.h + self.c * LD(t)
        e, r = _parts(x)
        sg = np.where(x >= 0, r, e * r)
        self.evals += 1
        return float(np.sum(self.c * (sg - self.mu))), float(np.sum((self.c * self.c) * ((e * r) * r)))

    def k02(self, t):
        x = self.h + self.c * LD(t)
        e, r = _parts(x)
        k0 = np.sum(softplus(x) - softplus(self.h)) - LD(t) * np.sum(self.c * self.mu)
        return float(k0), float(np.sum((self.c * self.c) * ((e * r) * r)))


def root(col, s, V):
    """(t_hat, converged, evaluations) of K'(t) = s by the iteration of the module docstring."""
    tol = TOL_F * math.sqrt(V)
    t, lo, hi = 0.0, -math.inf, math.inf
    n = 0
    with np.errstate(all="ignore"):
        while True:
            k1, k2 = col.k12(t)
            n += 1
            f = k1 - s
            if abs(f) <= tol:
                return float(np.float64(t) - np.float64(f) / np.float64(k2)), True, n
            if n == MAX_EVALS:
                return math.nan, False, n
            if f < 0:
                lo = t
            else:
                hi = t
            tn = float(np.float64(t) - np.float64(f) / np.float64(k2))
            if not (lo < tn < hi):
                if f < 0:
                    tn = (t + hi) / 2 if math.isfinite(hi) else (2 * t if t > 0 else 1.0)
                else:
                    tn = (lo + t) / 2 if math.isfinite(lo) else (2 * t if t < 0 else -1.0)
            t = tn


def log_phi_neg(a):
    """log Phi(-a), a >= 0."""
    from scipy.special import log_ndtr
    return float(log_ndtr(-a))


def finish_tail(t, s, K, K2, V, converged):
    """(accepted, log tail, r) from the values at t_hat."""
    with np.errstate(all="ignore"):
        if not converged or not math.isfinite(t) or not (K2 >= MIN_K2 * V):
            return False, math.nan, math.nan
        w2 = np.float64(2.0) * (np.float64(t) * np.float64(s) - np.float64(K))
        w = math.copysign(1.0, t) * float(np.sqrt(w2))
        v = t * math.sqrt(K2)
        r = float(np.float64(w) + np.log(np.float64(v) / np.float64(w)) / np.float64(w))
    if not math.isfinite(r) or r == 0.0 or (r > 0) != (t > 0):
        return False, math.nan, r
    return True, log_phi_neg(abs(r)), r


def tail(col, s, V):
    """dict of one computed tail: accepted, logp, t, r, K, K2, evals, converged."""
    t, conv, n = root(col, s, V)
    K, K2 = col.k02(t) if conv and math.isfinite(t) else (math.nan, math.nan)
    ok, lp, r = finish_tail(t, s, K, K2, V, conv)
    return dict(accepted=ok, logp=lp, t=t, r=r, K=K, K2=K2, evals=n, converged=conv, s=s)


def combine(l0, l1):
    """-log10(exp(l0) + exp(l1)); either may be -inf."""
    m, o = (l0, l1) if l0 >= l1 else (l1, l0)
    return -(m + math.log1p(math.exp(o - m))) / math.log(10.0)


def column(c, h, q, V, nlp):
    """(state 1 or 2, neglog10p_spa, t_hat pair, the computed tails) of one tried column; nlp is the normal value."""
    col = Column(c, h)
    aq = abs(q)
    tails = [None, None]
    obs = 0 if q >= 0 else 1
    logs = [-math.inf, -math.inf]
    for k, s in ((0, aq), (1, -aq)):
        if k != obs and (s >= col.smax if k == 0 else s <= col.smin):
            continue
        tails[k] = tail(col, s, V)
        logs[k] = tails[k]["logp"]
    that = [tl["t"] if tl is not None else math.nan for tl in tails]
    if all(tl["accepted"] for tl in tails if tl is not None):
        return 1, combine(logs[0], logs[1]), that, tails, col
    return 2, nlp, that, tails, col


def spa(sp, eta, Z, cutoff, columns=None):
    """The whole statement on top of a plain spec sp (assoc_spec.score / score_dense with t = 1): dict of state (uint8 p),
    neglog10p_spa (p), t_hat (p x 2), neglog10p (p, scipy), and per tried column its tails and Column (for the margins)."""
    X, z, V, Um = sp["X"], sp["z"][:, 0], sp["V"], sp["U"][:, 0]
    p = X.shape[1]
    eta = np.asarray(eta, dtype=np.float64)
    al = alpha_of(sp["b"], sp["Linv"])
    nlp = S.neglog10p(z)
    state = np.zeros(p, dtype=np.uint8)
    out = nlp.copy()
    that = np.full((p, 2), np.nan)
    detail = {}
    for j in (range(p) if columns is None else columns):
        if np.isnan(z[j]) or not (abs(z[j]) >= cutoff) or math.isinf(z[j]):
            continue
        c = adjusted(X[:, j], Z, al[j])
        st, val, th, tails, col = column(c, eta, float(Um[j]), float(V[j]), float(nlp[j]))
        state[j], out[j], that[j] = st, val, th
        detail[j] = dict(tails=tails, col=col, c=c)
    return dict(state=state, neglog10p_spa=out, t_hat=that, neglog10p=nlp, detail=detail, alpha=al)


# ---- the margins of a clear decision ----------------------------------------------------------------------------------------------
def clear(sp, res, j, cutoff, dz):
    """Whether the spec's decisions on column j leave the device no room to decide otherwise: |z| - cutoff at least 100 x the plain
    bound on z either way; for every computed tail K''(t_hat) / V outside [2^-30, 2^-10], at most 48 evaluations, |r| >= 0.1; and the
    other tail's target more than 1e-6 (S_max - S_min) from the end of the range (where the observed tail is refused the column
    has state 2 whatever the other one does, and this last margin is not asked for)."""
    z = sp["z"][j, 0]
    if np.isnan(z):
        return True
    if math.isfinite(cutoff) and abs(abs(z) - cutoff) < 100 * dz[j, 0]:
        return False
    if j not in res["detail"]:
        return True
    d = res["detail"][j]
    col, q, V = d["col"], float(sp["U"][j, 0]), float(sp["V"][j])
    for tl in d["tails"]:
        if tl is None:
            continue
        if tl["evals"] > 48:
            return False
        if tl["converged"] and math.isfinite(tl["K2"]) and 2.0 ** -30 <= tl["K2"] / V <= 2.0 ** -10:
            return False
        if tl["accepted"] and abs(tl["r"]) < 0.1:
            return False
        if tl["converged"] and not tl["accepted"] and not (tl["K2"] < MIN_K2 * V):     # refused for another reason than the guard
            return False
    obs = d["tails"][0 if q >= 0 else 1]
    if not obs["accepted"]:                  # state 2 whatever the other tail does
        return True
    span = col.smax - col.smin
    other = -abs(q) if q >= 0 else abs(q)
    end = col.smin if q >= 0 else col.smax
    return abs(other - end) > 1e-6 * span


def device_tolerance(sp, res, dz):
    """|device - spec| allowed on neglog10p_spa where state = 1.  The derivation of a full bound (assoc_spec.bound carried through
    alpha, c, the three sums, device exp / log1p and the root) was not reached; this is the yardstick the issue names in its
    place, built from the spec's own error and not from the device's output:
        16 SPEC_ERR neglog10p_spa          (SPEC_ERR: the spec against 40-digit mpmath on these inputs, measured on the CPU; 16 x for a
                                            2-ulp device exp against numpy's 1 and the float64 row sums in another order)
      + dz |d neglog10p / dz|              (the plain scan's bound on z: the device's q = U and V are its own; the normal tail's
                                            slope |z| + 1 / |z| >= phi(z) / Phi(-|z|), over log 10, stands in for the saddlepoint tail's, which is flatter)."""
    z = np.abs(sp["z"][:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        slope = (z + 1.0 / np.maximum(z, 1e-300)) / math.log(10.0)
        return 16 * SPEC_ERR * np.abs(res["neglog10p_spa"]) + dz[:, 0] * slope


# ---- the inputs of the edge tests ----------------------------------------------------------------------------------------------------
EDGE_N = (15, 64, 65, 255, 256, 257, 511, 513, 1000)
EDGE_P = (1, 33, 150)
EDGE_C = (1, 2, 5, 19)
EDGE_MISSING = (0.0, 0.03)
CUTOFF = 1.0                # of the edge tests: about a third of the null columns are tried
MAX_REDRAWN = 0.10
# beside edge_cases(): the one n-dependent path of k_assoc_spa (rows four at a time from n = 769 on) at one and at several groups
EXTRA_CASES = ((2500, 33, 2, 0.03, (1, 1, 1), 15100), (1024, 33, 1, 0.0, (1, 0, 1), 15101))


def edge_cases():
    """(n, p, c, missing share, flags, seed): every (n, p) once, the other factors cycling.  c <= n / 3 always, and c <= n / 20: at
    most 15 % of the rows are cases, and a logistic null model with fewer than 3 c of them is as good as always separated."""
    out = []
    t = 0
    for n in EDGE_N:
        for p in EDGE_P:
            ci = t
            while 3 * EDGE_C[ci % 4] > n or 20 * EDGE_C[ci % 4] > max(n, 20):
                ci += 1
            out.append((n, p, EDGE_C[ci % 4], EDGE_MISSING[(t + t // 4) % 2], S.EDGE_FLAGS[(t // 2) % 4], 15000 + t))
            t += 1
    return out


def null_model(y, Z):
    """The package's fit_null run to convergence (Bernoulli, logit), or None where the cases are (nearly) separated."""
    from mendeliht_amd import api
    from mendeliht_amd.assoc import fit_null
    try:
        with np.errstate(all="ignore"):
            m = fit_null(y, Z, api.Bernoulli(), tol=1e-14, max_iter=200)
    except (np.linalg.LinAlgError, FloatingPointError):
        return None
    if not m.converged or not np.isfinite(m.eta).all() or np.abs(m.eta).max() > 20:
        return None
    return m


def edge_inputs(case, cutoff=CUTOFF):
    """(codes n x p, y, eta, A, w, Z, redrawn share) of an edge case.  Z: an intercept and covariates as assoc_spec.edge_inputs
    makes them.  y: Bernoulli with 3 % .. 15 % cases, never fewer than 2 (nor than 3 c), the null model fitted by the package's fit_null
    run to convergence (redrawn where the cases are separated), A = y - mu, w = mu (1 - mu).  Columns: binomial genotypes, allele frequencies 0.02 .. 0.3; where p >= 31 the plain
    scan's three degenerate columns (3, 17, p - 2), a planted-effect column (5, and the only column of p = 1: carriers drawn three times as often among the
    cases) and a boundary column (7): c = 1 -- carriers exactly the cases, so the statistic is at the end of its range and the
    spec gives state 2; c > 1 -- carriers among the cases only (monomorphic among the controls), held to whatever the spec says.
    Another column that comes out degenerate, or with V / Q < 10 MIN_V_OVER_Q, is redrawn as in assoc_spec; a column whose decision is not clear (clear()) is redrawn
    too, and the share of those among all drawn columns is returned: tests/test_spa_spec_cpu.py holds it to MAX_REDRAWN."""
    n, p, c, missing, flags, seed = case
    rng = np.random.default_rng(seed)
    Zr = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1)
    Qf, Rf = np.linalg.qr(Zr)
    Z = Qf * np.sign(np.diag(Rf))[None, :] * math.sqrt(n)
    Z[:, 0] = 1.0
    for _ in range(20):
        ncase = max(2, 3 * c, int(round(rng.uniform(0.03, 0.15) * n)))
        lin = 0.5 * (Z[:, 1:] @ rng.standard_normal(c - 1)) / math.sqrt(max(c - 1, 1)) + rng.gumbel(size=n)
        y = np.zeros(n)
        y[np.argsort(-lin)[:ncase]] = 1.0
        null = null_model(y, Z)
        if null is not None:
            break
    else:
        raise AssertionError(("no logistic null model", case))
    eta, mu = null.eta, sigma(null.eta)
    A, w = y - mu, mu * (1.0 - mu)
    cases_idx = np.flatnonzero(y == 1.0)

    def draw(kind="plain"):
        f = rng.uniform(0.02, 0.3)
        col = rng.binomial(2, f, n).astype(np.int64)
        if kind == "planted":
            col[cases_idx] = rng.binomial(2, min(3 * f, 0.9), cases_idx.size)
        elif kind == "boundary":
            col[:] = 0
            if c == 1:
                col[cases_idx] = 1
            else:
                col[cases_idx] = rng.binomial(1, 0.7, cases_idx.size)
                col[cases_idx[0]] = 1
                return col                     # (no missing entries: they would be imputed among the controls)
        if missing > 0 and kind != "boundary":
            col[rng.random(n) < missing] = -1
        return col
    kinds = ["plain"] * p
    if p >= 31:
        kinds[5], kinds[7] = "planted", "boundary"
    elif p == 1:
        kinds[0] = "planted"
    codes = np.stack([draw(k) for k in kinds], axis=1)
    if p >= 31:
        codes[:, 3], codes[:, 17], codes[:, p - 2] = 0, 2, -1
    G, Linv = S.null_factor(Z, w)
    drawn, unclear = 0, 0
    for j in range(p):
        for _ in range(50):
            drawn += 1
            cj = codes[:, j:j + 1]
            if p >= 31 and j in (3, 17, p - 2):
                break
            sp = S.score(cj, flags, A, w, Z) if not S.degenerate(cj)[0] else None
            if sp is None or not (sp["V"][0] / sp["Q"][0] >= 10 * S.MIN_V_OVER_Q):
                drawn -= 1                     # (assoc_spec's own redraw: not a margin of this spec)
                codes[:, j] = draw(kinds[j])
                continue
            dz = S.bound(sp, cj, flags, A, w, Z)[0]
            if clear(sp, spa(sp, eta, Z, cutoff), 0, cutoff, dz):
                break
            unclear += 1
            codes[:, j] = draw(kinds[j])
        else:
            raise AssertionError(("no column with a clear decision", case, j))
    return codes, y, eta, A, w, Z, unclear / max(drawn, 1)
