"""tests/assoc_spec.py, the numpy statement of the association scan, checked on the CPU: against a brute-force statement, against
the OLS t-statistic, its null fits against scikit-learn, its invariances, the conditions its edge inputs promise the GPU test,
and the shipped example's planted SNPs."""
import os
import re

import numpy as np
import pytest

import assoc_spec as S
from conftest import FIX, ROOT


@pytest.fixture(scope="module")
def edge():
    return [(case, S.edge_inputs(case)) for case in S.edge_cases()]


def test_edge_cases_cover_every_value_of_every_factor():
    cases = S.edge_cases()
    assert len(cases) == len(S.EDGE_N) * len(S.EDGE_P) == len({(c[0], c[1]) for c in cases})
    assert {(c[2], c[3]) for c in cases} == set(S.EDGE_TC)
    assert {c[4] for c in cases} == set(S.EDGE_MISSING) and {c[5] for c in cases} == set(S.EDGE_FLAGS)
    assert {c[6] for c in cases} == set(S.EDGE_WEIGHTS)
    assert all(3 * c[3] <= c[0] for c in cases)
    for wk in S.EDGE_WEIGHTS:                          # every weight kind meets every p, several n and both missing shares
        mine = [c for c in cases if c[6] == wk]
        assert {c[1] for c in mine} == set(S.EDGE_P) and len({c[0] for c in mine}) >= 6 and {c[4] for c in mine} == set(S.EDGE_MISSING), wk
    for tc in S.EDGE_TC[:3]:
        assert len({c[6] for c in cases if (c[2], c[3]) == tc}) >= 4, tc
    for tc in S.EDGE_TC[3:]:                           # the wide ones: with and without weights
        kinds = {c[6] for c in cases if (c[2], c[3]) == tc}
        assert kinds & {"none", "ones"} and kinds & {"logistic", "zeros"}, (tc, kinds)


def test_spec_against_the_brute_force_statement_and_the_conditions_of_the_edge_inputs(edge):
    """Residualise x_j on Z under W, V = x_perp' W x_perp, U = x_perp' A.  Tolerance: the brute force goes through a least-squares
    solve, so it is held to 1e-9 relative -- seven orders above the spec's own rounding at kappa <= 100 -- not to the derived bound.
    The conditions the GPU test relies on, for every case: V_j / Q_j >= 1e-3 on the non-degenerate columns, kappa(G) <= 100, NaN
    exactly at the degenerate columns, and the derived bound finite there."""
    worst_v, worst_k = np.inf, 0.0
    for case, (codes, A, w, Z) in edge:
        n, p, t, c, missing, flags, wk, seed = case
        sp = S.score(codes, flags, A, w, Z)
        ok = ~sp["deg"]
        assert np.array_equal(np.isnan(sp["z"][:, 0]), sp["deg"]), case
        if p >= 31:
            assert sp["deg"][3] and sp["deg"][17] and sp["deg"][p - 2], case
        ev = np.linalg.eigvalsh(sp["G"])
        kappa = ev[-1] / ev[0]
        assert kappa <= S.MAX_KAPPA, (case, kappa)
        worst_k = max(worst_k, kappa)
        if ok.any():
            vq = (sp["V"][ok] / sp["Q"][ok]).min()
            assert vq >= S.MIN_V_OVER_Q, (case, vq)
            worst_v = min(worst_v, vq)
            zb, bb, sb, Vb = S.brute(sp["X"][:, ok], A, w, Z)
            np.testing.assert_allclose(sp["z"][ok], zb, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(sp["beta"][ok], bb, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(sp["se"][ok], sb, rtol=1e-9)
            dz, dbeta, dse = S.bound(sp, codes, flags, A, w, Z)
            assert np.isfinite(dz[ok]).all() and np.isfinite(dbeta[ok]).all() and np.isfinite(dse[ok]).all(), case
            assert (dz[ok] <= 1e-6 * (1.0 + np.abs(sp["z"][ok]))).all(), (case, float(dz[ok].max()))     # a bound that means something
    print(f"edge inputs: min V/Q = {worst_v:.3g}, max kappa(G) = {worst_k:.3g}")


def test_quantised_class_sums_are_within_half_a_quantum_per_row_of_the_true_ones(edge):
    from fractions import Fraction
    done = 0
    for case, (codes, A, w, Z) in edge:
        if w is None or case[0] > 129 or case[1] > 33:
            continue
        q = Fraction(S.quantum(w))
        exact = S.class_sums_quantised(codes, w)
        true = S.class_sums(codes, w)
        for k, v in enumerate((0, 1, 2, -1)):
            cnt = (codes == v).sum(axis=0)
            for j in range(codes.shape[1]):
                assert abs(exact[k][j] - Fraction(float(true[k, j]))) <= q / 2 * int(cnt[j]) + Fraction(float(true[k, j])) / 2 ** 52, (case, k, j)
        done += 1
    assert done >= 8


def _fixture_problem():
    n = 1000
    bed = np.fromfile(os.path.join(FIX, "normal.bed"), dtype=np.uint8)[3:].reshape(-1, (n + 3) // 4)
    two = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n]
    codes = np.array([0, -1, 1, 2], dtype=np.int64)[two].T.copy()
    y = np.loadtxt(os.path.join(FIX, "normal_y_fam6.txt"))
    z = np.loadtxt(os.path.join(FIX, "covariates.txt"), delimiter=",")
    return codes, y, z


def _normal_null(y, z):
    gamma = np.linalg.lstsq(z, y, rcond=None)[0]
    r = y - z @ gamma
    phi = float(r @ r) / (len(y) - z.shape[1])
    return r / np.sqrt(phi)


def test_normal_identity_against_the_ols_t_statistic():
    """z^2 = (n - c) T^2 / (n - c - 1 + T^2), T the OLS t-statistic of the SNP in y ~ Z + x (numpy lstsq), on the shipped data."""
    codes, y, z = _fixture_problem()
    n, c = z.shape
    sp = S.score(codes, (1, 1, 1), _normal_null(y, z), None, z)
    top = int(np.nanargmax(np.abs(sp["z"][:, 0])))
    assert top == 9414
    for j in (top, 4716, 17, 5000):
        D = np.concatenate([z, sp["X"][:, j:j + 1]], axis=1)
        coef = np.linalg.lstsq(D, y, rcond=None)[0]
        res = y - D @ coef
        s2 = float(res @ res) / (n - c - 1)
        T = coef[-1] / np.sqrt(s2 * np.linalg.inv(D.T @ D)[-1, -1])
        want = (n - c) * T * T / (n - c - 1 + T * T)
        assert abs(sp["z"][j, 0] ** 2 - want) <= 1e-9 * want, (j, sp["z"][j, 0] ** 2, want)
        if j == top:
            assert abs(want - 554.82227036049) < 1e-6 and abs(sp["z"][j, 0] ** 2 - 554.82227036049) < 1e-6


def test_the_seven_largest_z_of_the_shipped_example_are_its_planted_snps():
    codes, y, z = _fixture_problem()
    sp = S.score(codes, (1, 1, 1), _normal_null(y, z), None, z)
    az = np.abs(sp["z"][:, 0])
    order = np.argsort(-np.where(np.isnan(az), -1.0, az), kind="stable")
    assert order[:7].tolist() == [9414, 4716, 8374, 6289, 7754, 4245, 3136]
    with open(os.path.join(FIX, "normal_true_beta.txt")) as f:         # snpID (1-based "snp<k>"), effect size
        tb = {int(ln.split(",")[0][3:]) - 1: float(ln.split(",")[1]) for ln in f.read().split()[1:]}
    assert sorted(order[:7].tolist()) == sorted(j for j, b in tb.items() if abs(b) >= 0.46)
    assert abs(az[order[6]] - 4.14) < 0.01 and abs(az[order[7]] - 3.76) < 0.01
    ok = ~sp["deg"]
    ev = np.linalg.eigvalsh(sp["G"])
    assert (sp["V"][ok] / sp["Q"][ok]).min() > 0.98 and abs(ev[-1] / ev[0] - 6.5) < 0.1
    raw = S.score(codes, (0, 0, 1), _normal_null(y, z), None, z)       # the uncentred matrix: the intercept takes the mean out of Q
    assert abs((raw["V"][ok] / raw["Q"][ok]).min() - 0.30) < 0.01
    assert np.argsort(-np.where(np.isnan(raw["z"][:, 0]), -1.0, np.abs(raw["z"][:, 0])), kind="stable")[:7].tolist() == order[:7].tolist()


def test_fit_null_against_scikit_learn():
    """Coefficients of the mirror's IRLS against scikit-learn's unpenalised GLMs.  Both stop on their own criteria: fit_null at a
    relative deviance change of 1e-13, the lbfgs solvers at a projected gradient of 1e-10 (tol below); lbfgs's criterion bounds the
    coefficients only through the curvature, so the comparison is held to 1e-6 -- the square root of its tolerance, the usual
    guarantee of a gradient criterion -- and Normal against lstsq to 1e-10."""
    from sklearn.linear_model import GammaRegressor, LogisticRegression, PoissonRegressor

    import mendeliht_amd as m
    rng = np.random.default_rng(5)
    n, c = 400, 4
    z = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1)
    g = np.array([0.3, 0.5, -0.4, 0.2])
    eta = z @ g
    y = eta + rng.standard_normal(n)
    nm = m.fit_null(y, z, m.Normal())
    np.testing.assert_allclose(nm.gamma, np.linalg.lstsq(z, y, rcond=None)[0], rtol=1e-10, atol=1e-12)
    assert abs(nm.phi - np.sum((y - z @ nm.gamma) ** 2) / (n - c)) <= 1e-12 * nm.phi
    yb = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float)
    nb = m.fit_null(yb, z, m.Bernoulli(), tol=1e-13)
    sk = LogisticRegression(penalty=None, fit_intercept=False, tol=1e-10, max_iter=10000).fit(z, yb)
    np.testing.assert_allclose(nb.gamma, sk.coef_[0], rtol=1e-6, atol=1e-6)
    assert nb.converged and nb.phi == 1.0
    np.testing.assert_allclose(nb.w, nb.mu * (1 - nb.mu), rtol=1e-12)
    np.testing.assert_allclose(nb.A, yb - nb.mu, rtol=1e-9, atol=1e-12)
    yp = rng.poisson(np.exp(eta)).astype(float)
    npo = m.fit_null(yp, z, m.Poisson(), tol=1e-13)
    sk = PoissonRegressor(alpha=0, fit_intercept=False, tol=1e-10, max_iter=10000).fit(z, yp)
    np.testing.assert_allclose(npo.gamma, sk.coef_, rtol=1e-6, atol=1e-6)
    yg = rng.gamma(4.0, np.exp(eta) / 4.0)
    ng = m.fit_null(yg, z, m.Gamma(), m.LogLink(), tol=1e-13)
    sk = GammaRegressor(alpha=0, fit_intercept=False, tol=1e-10, max_iter=10000).fit(z, yg)
    np.testing.assert_allclose(ng.gamma, sk.coef_, rtol=1e-6, atol=1e-6)
    assert abs(ng.phi - np.sum((yg - ng.mu) ** 2 / ng.mu ** 2) / (n - c)) <= 1e-12 * ng.phi
    with pytest.raises(ValueError):
        m.fit_null(yp, z, m.NegativeBinomial(r=2.0), est_r="Newton")
    nn = m.fit_null(yp, z, m.NegativeBinomial(r=2.0), tol=1e-13)
    assert nn.converged and nn.phi == 1.0
    # every other link the fits accept runs and converges on data of its own shape
    for d, l, yy in ((m.Bernoulli(), m.ProbitLink(), yb), (m.Bernoulli(), m.CloglogLink(), yb), (m.Bernoulli(), m.CauchitLink(), yb),
                     (m.Poisson(), m.SqrtLink(), yp), (m.Gamma(), m.InverseLink(), rng.gamma(4.0, 1.0 / (4.0 * (2.0 + 0.2 * z[:, 1])))),
                     (m.InverseGaussian(), m.LogLink(), yg), (m.Normal(), m.LogLink(), np.exp(0.2 * eta) + 0.05 * rng.standard_normal(n))):
        fit = m.fit_null(yy, z[:, :2], d, l, tol=1e-12)
        assert fit.converged and np.isfinite(fit.gamma).all() and np.isfinite(fit.A).all() and (fit.w >= 0).all(), (d, l)


def test_statistic_does_not_depend_on_center_and_scale(edge):
    """With an intercept in span(Z) and impute = True: z is the same for every (center, scale); beta and se scale by 1 / sinv."""
    done = 0
    for case, (codes, A, w, Z) in edge:
        if case[0] not in (64, 129) or case[6] == "outlier":
            continue
        ref = S.score(codes, (1, 1, 1), A, w, Z)
        ok = ~ref["deg"]
        for flags in ((0, 0, 1), (1, 0, 1), (0, 1, 1)):
            sp = S.score(codes, flags, A, w, Z)
            np.testing.assert_allclose(sp["z"][ok], ref["z"][ok], rtol=1e-8, atol=1e-10)
            s = ref["stats"][1][ok] if not flags[1] else np.ones(ok.sum())
            np.testing.assert_allclose(sp["beta"][ok], ref["beta"][ok] * s[:, None], rtol=1e-8, atol=1e-10)
            np.testing.assert_allclose(sp["se"][ok], ref["se"][ok] * s, rtol=1e-8)
        done += 1
    assert done >= 10


def test_header_declares_the_entry_point_and_the_mirror_lists_it():
    from mendeliht_amd import api
    header = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"^int\s+(mih_\w+)\s*\(", header, flags=re.M))
    assert "mih_assoc_score" in declared and "mih_assoc_score" in api.exported_symbols()
    assert "assoc.hip" in open(os.path.join(ROOT, "mendeliht.jl_amd", "csrc", "Makefile")).read()


def test_top_orders_by_falling_absolute_z_and_skips_nan():
    from mendeliht_amd.assoc import AssocResult
    z = np.array([1.0, np.nan, -3.0, 2.0, 3.0])
    r = AssocResult(z, z, z, z)
    assert r.top(3).tolist() == [2, 4, 3] and r.top(10).tolist() == [2, 4, 3, 0]
