"""The numpy statement of the Firth-penalised effect size and likelihood-ratio p-value of the case-control association scan
(csrc/assoc_firth.hip: mih_assoc_score_firth; score_test_firth and assoc(..., firth=True) of the matrix classes).  It is the
yardstick of the device path and builds on tests/assoc_spec.py (U, b, V, z, beta, se, the degenerate-column rule) and on
tests/spa_spec.py, whose alpha_of, adjusted, sigma, softplus and row-sum conventions it takes as they are.

One Bernoulli trait, logit link.  A = y - mu, w = mu (1 - mu) and eta come from the caller's null fit.  h_i = eta_i, mu_i =
sigma(h_i); per column j the covariate-adjusted genotype c_i = x_ij - sum_k Z_ik alpha_k, the cumulant generating function
    K(b) = sum_i [softplus(h_i + c_i b) - softplus(h_i)] - b M1,      M1 = sum_i c_i mu_i,
q = U_j and V_j are exactly those of spa_spec.  The approximate Firth test (REGENIE's): the covariates' effects are held at the
null fit as an offset, which leaves a one-parameter logistic model in c_i with
    log-likelihood  l(b) - l(0) = b q - K(b),      score  q - K'(b),      information  K''(b)
(at b = 0 it reproduces the scan's U and V), and Jeffreys' penalty is added to it.

Per row, with x = h_i + c_i b (one product, one sum), e = exp(-|x|), r = 1 / (1 + e):
    sigma = r (x >= 0) or e r        s = (e r) r        d = (1 - e) r        omega = -d (x >= 0) or d      (omega = 1 - 2 sigma)
    K1 = sum c (sigma - mu)      K2 = sum (c c) s      K3 = sum ((c c) c) (s omega)      K4 = sum ((c c) (c c)) (s (1 - 6 s))
K1 .. K4 are K', K'', K''' and K''''; one exp and one division per row.

The penalised log-likelihood relative to b = 0 is  L*(b) = b q - K(b) + log(K2(b) / K2(0)) / 2.  Its stationarity condition is
g(b) = q with
    g = K1 - (K3 / K2) / 2
    D = K2 - ((K4 K2 - K3 K3) / (K2 K2)) / 2            (g'(b); D := K2 where D is not finite or not > 0)
in float64, every operation rounded by itself.

The root (root()): Newton from b = 0 with slope D under exactly the safeguard of spa_spec.root with k1 := g, k2 := D, s := q:
b = 0, lo = -inf, hi = +inf.  Repeat:
    evaluate K1 .. K4 at b (one evaluation); form g and D; f = g - q
    f not finite: not converged -- stop
    |f| <= 2^-30 sqrt(V_j): converged; b_hat = b - f / D (one more Newton step, taken as it is) -- stop
    64 evaluations made: not converged -- stop
    f < 0: lo = b, else hi = b
    bn = b - f / D; if not lo < bn < hi (a NaN is not):
        f < 0: bn = (b + hi) / 2 if hi is finite, else 2 b if b > 0, else 1
        f > 0: bn = (lo + b) / 2 if lo is finite, else 2 b if b < 0, else -1
    b = bn
A root always exists: g - q has opposite signs at -inf and +inf.

At the root one more pass (spa_spec.Column.k02) gives K(b_hat) and K2(b_hat).  I0 is the K2 of the first evaluation (b = 0).
    dev = 2 ((b_hat q - K(b_hat)) + log(K2(b_hat) / I0) / 2)            (negative -> 0)
    beta_firth = b_hat,   se_firth = 1 / sqrt(K2(b_hat)),   neglog10p_firth = neglog10p of z = sqrt(dev)   (the chi^2_1 tail)

States.  0: the column is degenerate or |z_j| < cutoff.  1: the iteration converged, b_hat and dev are finite, and K2(b_hat) is
finite and >= 2^-40 V_j.  2: otherwise.  In states 0 and 2 the three Firth outputs are the plain scan's beta, se and neglog10p,
bit for bit.  beta_firth is per unit of x~, like the scan's beta.

The sums over the rows are evaluated in numpy longdouble (the terms too) and rounded once, as in spa_spec; g, D, the control
values and the finish are float64."""
import math

import numpy as np

import assoc_spec as S
import spa_spec as P

LD = np.longdouble
TOL_F = P.TOL_F             # |g(b) - q| <= TOL_F sqrt(V)
MIN_K2 = 2.0 ** -40         # state 1 needs K2(b_hat) >= MIN_K2 V
MAX_EVALS = P.MAX_EVALS
# The spec's own error against 50-digit mpmath (tests/test_firth_spec_cpu.py: a bracketed solve of g(b) = q from the same float64
# c_i), measured on the inputs of tests/test_gpu_assoc_firth.py -- every tried column of spa_spec.edge_cases() and EXTRA_CASES at
# cutoff 1 and of case (513, 150) at cutoff 0; the CPU test measures them again on a share of the inputs and holds them to these
# figures.  They are the yardstick of device_tolerance().
# 577 + 147 tried columns, all of them in state 1, 5.2 evaluations on average and 9 at most, K2(b_hat) / V >= 5.3e-4.  The
# worst columns: the boundary column 7 of case (511, 150, 1, ...) for b_hat (6.37e-14) and se (4.51e-14) -- b_hat q and K(b_hat)
# cancel there -- and column 105 of case (513, 150, 19, ...) at cutoff 0 for neglog10p (6.07e-13: dev = 6e-5 is the small
# difference of its terms).
SPEC_ERR_BETA = 6.4e-14     # |b_hat - ref| / se_firth
SPEC_ERR_SE = 4.6e-14       # |se_firth - ref| / ref
SPEC_ERR_NLP = 6.1e-13      # |neglog10p_firth - ref| / ref


class Column(P.Column):
    """spa_spec.Column with the four sums of an evaluation."""
    def k1234(self, b):
        x = self.h + self.c * LD(b)
        e, r = P._parts(x)
        er = e * r
        sg = np.where(x >= 0, r, er)
        s = er * r
        d = (1 - e) * r
        om = np.where(x >= 0, -d, d)
        c2 = self.c * self.c
        self.evals += 1
        return (float(np.sum(self.c * (sg - self.mu))), float(np.sum(c2 * s)), float(np.sum((c2 * self.c) * (s * om))),
                float(np.sum((c2 * c2) * (s * (1 - 6 * s)))))


def g_and_slope(k1, k2, k3, k4):
    """(g, D) from the four sums, float64."""
    with np.errstate(all="ignore"):
        k1, k2, k3, k4 = (np.float64(v) for v in (k1, k2, k3, k4))
        g = k1 - np.float64(0.5) * (k3 / k2)
        D = k2 - np.float64(0.5) * ((k4 * k2 - k3 * k3) / (k2 * k2))
    if not (D > 0) or not math.isfinite(D):
        D = k2
    return float(g), float(D)


def root(sums, q, V):
    """(b_hat, converged, evaluations, I0) of g(b) = q by the iteration of the module docstring; sums(b) gives K1 .. K4."""
    tol = TOL_F * math.sqrt(V)
    b, lo, hi = 0.0, -math.inf, math.inf
    n, I0 = 0, math.nan
    with np.errstate(all="ignore"):
        while True:
            k = sums(b)
            n += 1
            if n == 1:
                I0 = k[1]
            g, D = g_and_slope(*k)
            f = g - q
            if not math.isfinite(f):
                return math.nan, False, n, I0
            if abs(f) <= tol:
                return float(np.float64(b) - np.float64(f) / np.float64(D)), True, n, I0
            if n == MAX_EVALS:
                return math.nan, False, n, I0
            if f < 0:
                lo = b
            else:
                hi = b
            bn = float(np.float64(b) - np.float64(f) / np.float64(D))
            if not (lo < bn < hi):
                if f < 0:
                    bn = (b + hi) / 2 if math.isfinite(hi) else (2 * b if b > 0 else 1.0)
                else:
                    bn = (lo + b) / 2 if math.isfinite(lo) else (2 * b if b < 0 else -1.0)
            b = bn


def neglog10p_of_dev(dev):
    return float(S.neglog10p(np.array([math.sqrt(dev)]))[0])


def finish(b, conv, K, K2, I0, q, V):
    """(state 1 or 2, dev) from the values at the root."""
    if not conv or not math.isfinite(b) or not math.isfinite(K2) or not (K2 >= MIN_K2 * V):
        return 2, math.nan
    with np.errstate(all="ignore"):
        dev = float(np.float64(2.0) * ((np.float64(b) * np.float64(q) - np.float64(K)) + np.float64(0.5) * np.log(np.float64(K2) / np.float64(I0))))
    if not math.isfinite(dev):
        return 2, math.nan
    return 1, max(dev, 0.0)


def column(c, h, q, V, plain, sums=None):
    """One tried column: dict of state, beta, se, nlp (the Firth outputs; plain = (beta, se, neglog10p) of the scan where the
    state is 2), evals, converged, b (b_hat), K, K2, I0, dev and, in state 1, D and K3 at b_hat (for the tolerance).  sums: another
    source of K1 .. K4 than the column's own (the tests put a NaN in)."""
    col = Column(c, h)
    b, conv, n, I0 = root(col.k1234 if sums is None else sums, q, V)
    K, K2 = col.k02(b) if conv and math.isfinite(b) else (math.nan, math.nan)
    state, dev = finish(b, conv, K, K2, I0, q, V)
    out = dict(state=state, beta=plain[0], se=plain[1], nlp=plain[2], evals=n, converged=conv, b=b, K=K, K2=K2, I0=I0, dev=dev, col=col, c=c)
    if state == 1:
        k = col.k1234(b)
        out.update(beta=b, se=float(np.float64(1.0) / np.sqrt(np.float64(K2))), nlp=neglog10p_of_dev(dev), D=g_and_slope(*k)[1], K3=k[2])
    return out


def firth(sp, eta, Z, cutoff, columns=None):
    """The whole statement on top of a plain spec sp (assoc_spec.score / score_dense with t = 1): dict of state (uint8 p),
    beta_firth, se_firth, neglog10p_firth (p), evals (int32 p, 0 where not tried), neglog10p (p, scipy) and per tried column its
    column() (for the margins and the tolerance)."""
    X, z, V, Um = sp["X"], sp["z"][:, 0], sp["V"], sp["U"][:, 0]
    p = X.shape[1]
    eta = np.asarray(eta, dtype=np.float64)
    al = P.alpha_of(sp["b"], sp["Linv"])
    nlp = S.neglog10p(z)
    state = np.zeros(p, dtype=np.uint8)
    evals = np.zeros(p, dtype=np.int32)
    bf, sf, nf = sp["beta"][:, 0].copy(), np.array(sp["se"], dtype=np.float64).copy(), nlp.copy()
    detail = {}
    for j in (range(p) if columns is None else columns):
        if np.isnan(z[j]) or not (abs(z[j]) >= cutoff) or math.isinf(z[j]):
            continue
        c = P.adjusted(X[:, j], Z, al[j])
        d = column(c, eta, float(Um[j]), float(V[j]), (float(bf[j]), float(sf[j]), float(nlp[j])))
        state[j], bf[j], sf[j], nf[j], evals[j] = d["state"], d["beta"], d["se"], d["nlp"], d["evals"]
        detail[j] = d
    return dict(state=state, beta_firth=bf, se_firth=sf, neglog10p_firth=nf, evals=evals, neglog10p=nlp, detail=detail, alpha=al)


# ---- the margins of a clear decision ----------------------------------------------------------------------------------------------
MAX_UNCLEAR = 0.10          # of the tried columns of a case


def clear(sp, res, j, cutoff, dz):
    """Whether the spec's decision on column j leaves the device no room to decide otherwise: |z| - cutoff at least 100 x the
    plain bound on z either way, at most 48 evaluations, and K2(b_hat) / V outside [2^-50, 2^-30]."""
    z = sp["z"][j, 0]
    if np.isnan(z):
        return True
    if math.isfinite(cutoff) and abs(abs(z) - cutoff) < 100 * dz[j, 0]:
        return False
    if j not in res["detail"]:
        return True
    d = res["detail"][j]
    if d["evals"] > 48:
        return False
    if d["converged"] and math.isfinite(d["K2"]) and 2.0 ** -50 <= d["K2"] / float(sp["V"][j]) <= 2.0 ** -30:
        return False
    return True


def device_tolerance(sp, res, dz):
    """(tol beta_firth, tol se_firth, tol neglog10p_firth), p each: |device - spec| allowed where the state is 1 (NaN elsewhere).
    The derivation of a full bound (assoc_spec.bound carried through alpha, c, the four sums, device exp / log1p and the root) was
    not reached; this is the yardstick of spa_spec.device_tolerance, built from the spec's own error and never from the device's
    output:
      base         16 SPEC_ERR_* (the spec against 50-digit mpmath on these inputs, measured on the CPU; 16 x for a 2-ulp device exp
                   against numpy's 1 and the float64 row sums in another order): 16 SPEC_ERR_BETA se_firth, 16 SPEC_ERR_SE se_firth,
                   16 SPEC_ERR_NLP neglog10p_firth
      propagated   the plain scan's bound dz on z carried through the exact sensitivities (the device's q = U and V are its own):
                   dq = dz sqrt(V);  dbeta = dq / D(b_hat);  ddev = 2 |b_hat| dq (the envelope theorem: dL* / dq = b_hat at the
                   maximum);  neglog10p takes the slope (sqrt dev + 1 / sqrt dev) / ln 10 on dsqrt dev = ddev / (2 sqrt dev);
                   se takes |K3(b_hat)| / (2 K2(b_hat)^(3/2)) dbeta."""
    p = sp["z"].shape[0]
    tb, ts, tn = (np.full(p, np.nan) for _ in range(3))
    for j, d in res["detail"].items():
        if d["state"] != 1:
            continue
        dq = float(dz[j, 0]) * math.sqrt(float(sp["V"][j]))
        db = dq / d["D"]
        ddev = 2.0 * abs(d["b"]) * dq
        rt = math.sqrt(max(d["dev"], 1e-300))
        tb[j] = 16 * SPEC_ERR_BETA * d["se"] + db
        ts[j] = 16 * SPEC_ERR_SE * d["se"] + abs(d["K3"]) / (2.0 * d["K2"] ** 1.5) * db
        tn[j] = 16 * SPEC_ERR_NLP * abs(d["nlp"]) + (rt + 1.0 / rt) / math.log(10.0) * ddev / (2.0 * rt)
    return tb, ts, tn
