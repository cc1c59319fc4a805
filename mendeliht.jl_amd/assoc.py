"""The host side of the marginal association scan (mih_assoc_score): the null model of the covariates, fitted in numpy, and the
result of the scan.  The C ABI takes score residuals and working weights; a Julia caller has GLM.jl for them, this mirror has
fit_null -- GLM.jl's IRLS (its starting values, working response and deviance stopping rule) for every family and link the fits
accept."""
import math
import statistics

import numpy as np

_ND = statistics.NormalDist()
_erfc = np.frompyfunc(math.erfc, 1, 1)
_ndtri = np.frompyfunc(_ND.inv_cdf, 1, 1)
_EPS = np.finfo(np.float64).eps


def _f(a):
    return np.asarray(a, dtype=np.float64)


def _ndtr(x):
    return 0.5 * _f(_erfc(-_f(x) / math.sqrt(2.0)))


def _npdf(x):
    return np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# link code (api.*Link.code) -> (linkfun, linkinv, mueta), GLM.jl's glmtools.jl closed forms
LINKS = {
    0: (lambda mu: mu, lambda eta: eta, lambda eta: np.ones_like(eta)),
    1: (lambda mu: np.log(mu / (1.0 - mu)), lambda eta: 1.0 / (1.0 + np.exp(-eta)),
        lambda eta: np.exp(-np.abs(eta)) / (1.0 + np.exp(-np.abs(eta))) ** 2),
    2: (np.log, np.exp, np.exp),
    3: (lambda mu: _f(_ndtri(np.clip(mu, 1e-300, 1.0 - 1e-16))), _ndtr, lambda eta: np.maximum(_npdf(eta), _EPS)),
    4: (lambda mu: np.log(-np.log1p(-mu)), lambda eta: np.clip(-np.expm1(-np.exp(eta)), _EPS, 1.0 - _EPS),
        lambda eta: np.maximum(np.exp(eta) * np.exp(-np.exp(eta)), _EPS)),
    5: (lambda mu: np.tan(math.pi * (mu - 0.5)), lambda eta: 0.5 + np.arctan(eta) / math.pi,
        lambda eta: 1.0 / (math.pi * (1.0 + eta * eta))),
    6: (lambda mu: 1.0 / mu, lambda eta: 1.0 / eta, lambda eta: -1.0 / (eta * eta)),
    7: (lambda mu: 1.0 / (mu * mu), lambda eta: 1.0 / np.sqrt(eta), lambda eta: -(1.0 / np.sqrt(eta)) ** 3 / 2.0),
    8: (np.sqrt, lambda eta: eta * eta, lambda eta: 2.0 * eta),
}


def _xlogy(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 0.0, x * np.log(y))


# family code (api distributions) -> (variance(mu, r), unit deviance summed (y, mu, r), mustart(y), dispersion estimated?)
FAMILIES = {
    0: (lambda mu, r: np.ones_like(mu), lambda y, mu, r: np.sum((y - mu) ** 2), lambda y: y.copy(), True),
    1: (lambda mu, r: mu * (1.0 - mu), lambda y, mu, r: -2.0 * np.sum(_xlogy(y, mu) + _xlogy(1.0 - y, 1.0 - mu)),
        lambda y: (y + 0.5) / 2.0, False),
    2: (lambda mu, r: mu, lambda y, mu, r: 2.0 * np.sum(_xlogy(y, y / mu) - (y - mu)), lambda y: y + 0.1, False),
    3: (lambda mu, r: mu + mu * mu / r,
        lambda y, mu, r: 2.0 * np.sum(_xlogy(y, y / mu) - (y + r) * np.log((y + r) / (mu + r))),
        lambda y: y + (y == 0.0) / 6.0, False),
    4: (lambda mu, r: mu * mu, lambda y, mu, r: -2.0 * np.sum(np.log(y / mu) - (y - mu) / mu), lambda y: y.copy(), True),
    5: (lambda mu, r: mu ** 3, lambda y, mu, r: np.sum((y - mu) ** 2 / (y * mu * mu)), lambda y: y.copy(), True),
}
_CANONICAL = {0: 0, 1: 1, 2: 2, 3: 2, 4: 6, 5: 7}


class NullModel:
    """The fitted null model y ~ Z: coefficients gamma, eta = Z gamma, mu, the dispersion phi, and what the score test takes --
    A = (y - mu) mu'(eta) / (phi var(mu)) and w = mu'(eta)^2 / (phi var(mu))."""
    def __init__(self, gamma, eta, mu, phi, A, w, dev, iters, converged):
        self.gamma, self.eta, self.mu, self.phi, self.A, self.w = gamma, eta, mu, phi, A, w
        self.dev, self.iters, self.converged = dev, iters, converged

    def __repr__(self):
        return f"NullModel(c={self.gamma.size}, phi={self.phi!r}, dev={self.dev!r}, iters={self.iters}, converged={self.converged})"


def _codes(d, l):
    d = d() if isinstance(d, type) else d
    l = l() if isinstance(l, type) else l
    dc = int(d.code)
    if dc not in FAMILIES:
        raise ValueError(f"fit_null: no univariate GLM family for {d!r}")
    lc = _CANONICAL[dc] if l is None else int(l.code)
    if lc not in LINKS:
        raise ValueError(f"fit_null: unknown link {l!r}")
    return dc, lc, float(getattr(d, "r", 1.0))


def _wls(z, wt, resp):
    sw = np.sqrt(wt)
    return np.linalg.lstsq(z * sw[:, None], resp * sw, rcond=None)[0]


def fit_null(y, z, d, l=None, tol=1e-8, max_iter=100, est_r="None"):
    """IRLS fit of y ~ z for family d and link l (None: the canonical link, LogLink for NegativeBinomial), as GLM.jl runs it:
    mustart by family, working response eta + (y - mu) / mu'(eta) with weights mu'(eta)^2 / var(mu), weighted least squares, step
    halving while the deviance is not finite or rises, stop when |dev - dev_old| <= max(tol dev, tol).  The dispersion: RSS / (n - c)
    for Normal, Pearson chi^2 / (n - c) for Gamma and InverseGaussian, 1 otherwise; NegativeBinomial takes its r as given (est_r is
    refused: the score test conditions on a known r)."""
    if est_r not in (None, "None", False):
        raise ValueError("fit_null: est_r is not supported; give NegativeBinomial(r) its r")
    y, z = _f(y), _f(z)
    if z.ndim == 1:
        z = z[:, None]
    n, c = z.shape
    if y.shape != (n,):
        raise ValueError(f"fit_null: y has shape {y.shape}, expected ({n},)")
    dc, lc, r = _codes(d, l)
    variance, deviance, mustart, has_phi = FAMILIES[dc]
    linkfun, linkinv, mueta = LINKS[lc]
    with np.errstate(all="ignore"):
        if dc == 0 and lc == 0:                       # one exact least-squares step
            gamma = np.linalg.lstsq(z, y, rcond=None)[0]
            eta = z @ gamma
            mu, dev, iters, converged = eta, float(np.sum((y - eta) ** 2)), 1, True
        else:
            mu = mustart(y)
            eta = linkfun(mu)
            dev, gamma, converged, iters = float(deviance(y, mu, r)), np.zeros(c), False, 0
            for iters in range(1, max_iter + 1):
                me = mueta(eta)
                new = _wls(z, me * me / variance(mu, r), eta + (y - mu) / me)
                step = 1.0
                for _ in range(30):
                    g = gamma + step * (new - gamma) if iters > 1 else new
                    eta_n = z @ g
                    mu_n = linkinv(eta_n)
                    dev_n = float(deviance(y, mu_n, r))
                    if math.isfinite(dev_n) and (iters == 1 or dev_n <= dev + tol * abs(dev)):
                        break
                    if iters == 1:
                        raise FloatingPointError("fit_null: the first IRLS step has no finite deviance")
                    step *= 0.5
                gamma, eta, mu = g, eta_n, mu_n
                done = abs(dev - dev_n) <= max(tol * abs(dev_n), tol)
                dev = dev_n
                if done:
                    converged = True
                    break
        me, var = mueta(eta), variance(mu, r)
        phi = 1.0
        if has_phi:
            phi = float(np.sum((y - mu) ** 2 / var) / (n - c))
        A = (y - mu) * me / (phi * var)
        w = me * me / (phi * var)
    return NullModel(gamma, eta, mu, phi, A, w, dev, iters, converged)


class LmmNull:
    """The fitted variance-component null model y = Z alpha + g + e, g ~ N(0, tau_g Phi), e ~ N(0, tau_e I) (lmm_null of
    SnpLinAlg and DosageMatrix): tau = (tau_e, tau_g), h2 = tau_g dbar / (tau_g dbar + tau_e) with dbar the mean diagonal of
    Phi, alpha, Py (what the score test takes as A), gamma -- the mean of the variance ratios `ratios` of the marker columns
    `marker_cols` (None when the caller gave the genotypes), ratio_cv their coefficient of variation -- trace (the last
    Hutchinson estimates of tr P and tr P Phi), tau_path (the start and every iterate), iters, state (1 converged, 2 on the
    boundary tau_g = 0, 0 max_iter reached), cg_iters, worst_residual, and the covariates Z the model was fitted with."""
    def __init__(self, tau, alpha, Py, gamma, ratios, trace, dbar, tau_path, iters, state, cg_iters, worst_residual, marker_cols, Z):
        self.tau, self.alpha, self.Py, self.gamma, self.ratios, self.trace, self.dbar = tau, alpha, Py, gamma, ratios, trace, dbar
        self.tau_path, self.iters, self.state, self.cg_iters, self.worst_residual = tau_path, iters, state, cg_iters, worst_residual
        self.marker_cols, self.Z = marker_cols, Z
        self.h2 = float(tau[1] * dbar / (tau[1] * dbar + tau[0]))
        m = float(np.mean(ratios)) if len(ratios) else float("nan")
        self.ratio_cv = float(np.std(ratios) / m) if len(ratios) else float("nan")

    @property
    def converged(self):
        return self.state != 0

    def __repr__(self):
        return (f"LmmNull(tau_e={self.tau[0]!r}, tau_g={self.tau[1]!r}, h2={self.h2!r}, gamma={self.gamma!r}, iters={self.iters}, "
                f"state={self.state})")


class AssocResult:
    """z, beta, neglog10p: p (one trait) or p x t; se likewise.  NaN marks a degenerate column.  null: the NullModel (a list of
    them for several Normal traits).  With the saddlepoint pass (score_test_spa, assoc(..., spa=True)): neglog10p_spa (p),
    spa_state (p, uint8: 0 not tried, 1 saddlepoint value, 2 refused -- the normal value) and t_hat (p x 2: the roots of the
    upper and the lower tail, NaN where none); None without it.  With the Firth pass (score_test_firth, assoc(..., firth=True)):
    beta_firth, se_firth, neglog10p_firth (p: the penalised-likelihood estimate, its standard error and the likelihood-ratio
    p-value; the plain values where firth_state is not 1), firth_state (p, uint8: 0 not tried, 1 penalised values, 2 refused)
    and firth_evals (p, int32: the evaluations of the root, 0 where not tried); None without it."""
    def __init__(self, z, beta, se, neglog10p, null=None, wsum=None, neglog10p_spa=None, spa_state=None, t_hat=None,
                 beta_firth=None, se_firth=None, neglog10p_firth=None, firth_state=None, firth_evals=None):
        self.z, self.beta, self.se, self.neglog10p, self.null, self.wsum = z, beta, se, neglog10p, null, wsum
        self.neglog10p_spa, self.spa_state, self.t_hat = neglog10p_spa, spa_state, t_hat
        self.beta_firth, self.se_firth, self.neglog10p_firth = beta_firth, se_firth, neglog10p_firth
        self.firth_state, self.firth_evals = firth_state, firth_evals

    def top(self, k, trait=0):
        """The k columns with the largest |z| of a trait (0-based, by falling |z|; ties by index; degenerate columns never); with
        the saddlepoint pass, the k columns with the largest neglog10p_spa."""
        if self.neglog10p_spa is not None:
            a = np.asarray(self.neglog10p_spa)
        else:
            a = np.abs(self.z if self.z.ndim == 1 else self.z[:, trait])
        ok = np.flatnonzero(~np.isnan(a))
        order = ok[np.lexsort((ok, -a[ok]))]
        return order[:int(k)]

    def __repr__(self):
        return f"AssocResult(p={self.z.shape[0]}, traits={1 if self.z.ndim == 1 else self.z.shape[1]})"


class SetResult:
    """The set-based tests of set_test / assoc_sets.  Per set: m_used (int32: the members -- entries whose column is not degenerate
    and whose omega > 0), burden_z, neglog10p_burden, skat_q, neglog10p_skat and skat_state (uint8: 0 no value, 1 saddlepoint,
    2 rank one: the exact chi-square tail, 3 at the mean: the limit, 4 Q <= 0: p = 1, 5 the root iteration gave up: the
    moment-matched normal).  set_ptr, set_col, omega: the sets as they went in.  lambdas: the eigenvalues of every set's M, laid
    out like set_col (NaN after m_used); lambdas_of(s) gives one set's.  cov: None, or the list of the sets' covariance matrices.
    assoc: the AssocResult of the per-column scan of the same call.
    With skato=True (None otherwise): neglog10p_skato, the SKAT-O p-value; skato_rho, the grid value whose test has the smallest
    p-value (NaN without one); skato_state (uint8: 0 no value, 1 the integral, 2 rank one: neglog10p_skat itself, 3 the integral
    clamped to [p_min, R p_min], 4 fallback: min(1, R p_min)); neglog10p_rho (sets x R: the p-value of every grid value) and
    lambda_rho ((R + 1) x entries: the eigenvalues behind them and, last, those of the remainder M~)."""
    def __init__(self, set_ptr, set_col, omega, m_used, burden_z, neglog10p_burden, skat_q, neglog10p_skat, skat_state, lambdas, cov, assoc, skato=None):
        self.set_ptr, self.set_col, self.omega, self.m_used = set_ptr, set_col, omega, m_used
        self.burden_z, self.neglog10p_burden, self.skat_q, self.neglog10p_skat = burden_z, neglog10p_burden, skat_q, neglog10p_skat
        self.skat_state, self.lambdas, self.cov, self.assoc = skat_state, lambdas, cov, assoc
        self.neglog10p_skato, self.skato_rho, self.skato_state, self.neglog10p_rho, self.lambda_rho = skato if skato is not None else (None,) * 5

    def lambdas_of(self, s):
        return self.lambdas[self.set_ptr[s]:self.set_ptr[s] + self.m_used[s]]

    def top(self, k, by="skat"):
        """The k sets with the largest neglog10p_skat (by="burden": neglog10p_burden; by="skato_o": neglog10p_skato, which needs
        skato=True), falling; ties by index; sets without a value never."""
        if by == "skato_o" and self.neglog10p_skato is None:
            raise ValueError("top(by=\"skato_o\") needs a result of skato=True")
        a = np.asarray(self.neglog10p_burden if by == "burden" else self.neglog10p_skato if by == "skato_o" else self.neglog10p_skat)
        ok = np.flatnonzero(~np.isnan(a))
        return ok[np.lexsort((ok, -a[ok]))][:int(k)]

    def __repr__(self):
        return f"SetResult(sets={self.m_used.shape[0]}, p={self.assoc.z.shape[0]})"
