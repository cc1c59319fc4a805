"""CPU twin of tests/test_gpu_debias_refit.py: the inputs of the GLM refit tests are what that file takes them for, and its
references hold on a restatement of the kernels -- every refit problem converges in the oracle and is reproduced by it under other
row orders to 1e-12 max|beta| (the condition of the 1e-9 parity tolerance), the host rebuild of the panel equals the oracle's
standardized columns, the exact Gram and its counted bound hold for a float64 restatement of k_db_gram's slice order (and catch a
dropped row, a swapped tile pair and a row read twice), and the mpmath closed forms agree with the oracle's."""
import numpy as np
import pytest

from gpu_helpers import (DEBIAS_DIST, DEBIAS_FORMS, DEBIAS_LINK, DEBIAS_P, _pack, _row_orders, debias_form_errors, debias_forms_f64, debias_forms_mp,
                         debias_gamma, debias_gram_exact, debias_gram_jobs, debias_gram_misses, debias_gram_problem, debias_gram_restated,
                         debias_oracle_beta, debias_panel_snp, debias_refit_cases, debias_refit_problem, snp_host_stats)


@pytest.mark.parametrize("form", range(len(DEBIAS_FORMS)))
def test_every_refit_problem_converges_in_the_oracle_and_is_reproduced_under_other_row_orders(oracle, form):
    for dist, link, nb_r, n, k, attempt in debias_refit_cases():
        if (dist, link, nb_r) != DEBIAS_FORMS[form]:
            continue
        code, csi, idx, y = debias_refit_problem(dist, link, nb_r, n, k, attempt)
        if dist in ("poisson", "negbin"):
            assert (y == 0.0).sum() >= 3, (dist, link, n, k)                  # the y + 0.1 and 1/6 starts are run
        if dist in ("gamma", "invgauss") or (dist, link) == ("normal", "log"):
            assert (y > 0.0).all()
        b = debias_oracle_beta(oracle, code, csi, idx, y, dist, link, nb_r)      # raises where the oracle's refit fails
        assert np.isfinite(b).all() and np.count_nonzero(b) == k
        own = [debias_oracle_beta(oracle, code, csi, idx, y, dist, link, nb_r, perm) for perm in _row_orders(n)]
        spread = max(float(np.max(np.abs(o - b))) for o in own)
        assert spread <= 1e-12 * np.max(np.abs(b)), (dist, link, nb_r, n, k, spread / np.max(np.abs(b)))


def test_host_panel_equals_the_oracles_standardized_columns(oracle):
    """debias_panel_snp against x[:, j] of the oracle, read off xv_masked with a unit coefficient, under the four uses of the flags
    (and snp_host_stats against the oracle's mu and sinv)."""
    from gpu_helpers import debias_codes
    rng = np.random.default_rng(20282)
    n = 257
    code = debias_codes(rng, n, DEBIAS_P)
    assert (code == 1).any(axis=1).sum() > DEBIAS_P // 2
    mu, sinv = snp_host_stats(_pack(code), n)
    for csi in ((1, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0)):
        ox = oracle.Mat.from_bed_columns(_pack(code), n, center=csi[0], scale=csi[1], impute=csi[2])
        omu, osinv = ox.mu_sinv()
        np.testing.assert_allclose(mu, omu, rtol=4e-16); np.testing.assert_allclose(sinv, osinv, rtol=4e-16)
        idx = np.array([0, 31, 32, 64, DEBIAS_P - 1])
        P = debias_panel_snp(code, idx, mu, sinv, *csi)
        for t, j in enumerate(idx):
            mask = np.zeros(DEBIAS_P, np.uint8); mask[j] = 1
            coef = np.zeros(DEBIAS_P); coef[j] = 1.0
            np.testing.assert_allclose(P[:, t], ox.xv_masked(mask, coef), rtol=1e-15, atol=1e-15, err_msg=str((csi, j)))


@pytest.mark.parametrize("n,m", [(17, 5), (64, 17), (1000, 18), (4097, 34), (4161, 49)])
def test_exact_gram_and_counted_bound_on_a_restatement_of_the_slice_order(n, m):
    """debias_gram_exact against fractions.Fraction on a sample of entries; the float64 restatement of the kernel's order stays
    inside debias_gamma(n) (far inside: it is a worst-case count); the mutations the GPU test must catch leave it."""
    from fractions import Fraction
    rng = np.random.default_rng([20283, n, m])
    P = rng.standard_normal((n, m)) * np.exp(rng.uniform(-2, 2, m))
    P[:, 1] = rng.integers(0, 3, n)                                          # a whole-number column
    w = rng.uniform(0.01, 3.0, n)
    E, S = debias_gram_exact(P, w)
    for a, b in ((0, 0), (0, m - 1), (1, 1), (1, m - 1), (m - 1, m - 1), (m // 2, m - 2)):
        ex = sum((Fraction(float(P[i, a])) * Fraction(float(w[i])) * Fraction(float(P[i, b])) for i in range(n)), Fraction(0))
        assert E[a, b] == ex and S[a, b] == sum((abs(Fraction(float(P[i, a])) * Fraction(float(w[i])) * Fraction(float(P[i, b]))) for i in range(n)), Fraction(0))
    G = debias_gram_restated(P, w)
    bad, worst = debias_gram_misses(G.ravel(order="F"), P, w, n, exact=(E, S))
    assert not bad and worst < 1.0, (bad[:3], worst)
    drop = debias_gram_restated(np.delete(P, n // 2, axis=0), np.delete(w, n // 2))            # one row dropped
    assert debias_gram_misses(drop, P, w, n, exact=(E, S))[0]
    twice = G + np.multiply.outer(P[n - 1] * w[n - 1], P[n - 1])                                # the last row read twice
    assert debias_gram_misses(twice, P, w, n, exact=(E, S))[0]
    if m > 16:                                                               # tile pair (0, 1) stored transposed
        sw = G.copy()
        for a in range(16):
            for b in range(min(16, m - 16)):
                sw[a, 16 + b] = G[b, 16 + a] if 16 + a < m else 0.0
        assert debias_gram_misses(sw, P, w, n, exact=(E, S))[0]
    assert debias_gamma(4097) == Fraction(65 + 64 + 2, 2 ** 53)


def test_gram_jobs_cover_every_tile_slice_and_flag_edge():
    jobs = debias_gram_jobs()
    snp = [(n, k) for kind, n, k, _, _ in jobs if kind == "snp"]
    assert {k for n, k in snp if n == 4097} == {1, 15, 16, 17, 31, 32, 33, 48}
    assert {n for n, k in snp if k == 17} == {17, 63, 64, 65, 1000, 4095, 4096, 4097, 4161}
    assert {f for kind, _, _, f, _ in jobs if kind == "snp"} == {(1, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0)}
    assert {kind for kind, *_ in jobs} == {"snp", "f64", "f32", "dosage"} and len(jobs) < 60
    for kind, n, k, flags, seed in jobs:
        data, idx, y = debias_gram_problem(kind, n, k, flags, seed)
        p = DEBIAS_P if kind == "snp" else 40
        assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < p and y.shape == (n,)
        if k >= 6:
            assert {0, p - 1, 31, 32} <= set(idx.tolist())
        if kind == "snp" and n >= 63 and k >= 15:
            assert (data[idx] == 1).any()                                    # missing entries in the support
    assert DEBIAS_P % 32 != 0


def test_n_below_k_is_not_positive_definite_in_the_oracle(oracle):
    """The n < k jobs: a matrix of whole numbers -- the Gram is exact in any order, so the device's Cholesky sees the oracle's matrix."""
    for kind, n, k, flags, seed in debias_gram_jobs():
        if n >= k:
            continue
        code, idx, y = debias_gram_problem(kind, n, k, flags, seed)
        assert flags == (0, 0, 1) and not (code == 1).any()
        with pytest.raises(RuntimeError):
            debias_oracle_beta(oracle, code, flags, idx, y, "normal", "identity", 1.0)


def test_closed_forms_in_mpmath_agree_with_the_oracles(oracle):
    """linkinv, mueta and glmvar of gpu_helpers._mp_forms against orc_linkinv / orc_mueta / orc_glmvar, and the float64 forms of
    debias_forms_f64 against debias_forms_mp on the responses of the refit problems (a few ulps times the condition of the form)."""
    import mpmath as mp
    from gpu_helpers import _mp_forms
    _, linkfun, linkinv, mueta, glmvar = _mp_forms()
    L = oracle.lib()
    rng = np.random.default_rng(20284)
    with mp.workdps(50):
        for link, code in DEBIAS_LINK.items():
            lo, hi = (0.2, 3.0) if link in ("inverse", "invsquare", "sqrt") else (-3.0, 3.0)
            for e in rng.uniform(lo, hi, 40):
                for mine, theirs in ((linkinv[link], L.orc_linkinv), (mueta[link], L.orc_mueta)):
                    want = mine(mp.mpf(float(e)))
                    assert abs(mp.mpf(theirs(code, float(e))) - want) <= mp.mpf(2e-14) * abs(want), (link, e)
                if link != "probit":
                    assert abs(linkfun[link](linkinv[link](mp.mpf(float(e)))) - mp.mpf(float(e))) < mp.mpf(10) ** -40      # linkfun inverts linkinv
        for dist, code in DEBIAS_DIST.items():
            for m in rng.uniform(0.05, 0.95, 20):
                want = glmvar[dist](mp.mpf(float(m)), mp.mpf(4))
                assert abs(mp.mpf(L.orc_glmvar(code, float(m), 4.0)) - want) <= mp.mpf(1e-15) * abs(want)
    for dist, link, nb_r in DEBIAS_FORMS:
        y = debias_refit_problem(dist, link, nb_r, 257, 17)[3]
        w, t = debias_forms_f64(dist, link, nb_r, y)
        W, T = debias_forms_mp(dist, link, nb_r, y)
        assert debias_form_errors(w, W)[0].max() < 1e-12 and debias_form_errors(t, T)[0].max() < 1e-12, (dist, link)
