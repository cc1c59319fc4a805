"""Parity of the HIP path (through the C ABI) against the CPU oracle and the golden vectors: fits, cross-validation, model paths,
wrappers, error paths and the randomized sweeps (b, f1, f3).  The other rows: test_gpu_linalg.py (a1, a7, a8, f2),
test_gpu_mv.py (a14), test_gpu_resident.py (a12: the device-resident step), test_gpu_fullsize.py (every BASELINE config at its own size),
test_gpu_stress.py.

Tolerances (BASELINE.json north_star): support indices bit-exact at fixed k; beta within 1e-5
relative for Gaussian, 1e-4 for GLM links.  Kernel-level results are held to 1e-11.
"""
import json
import os

import numpy as np
import pytest

from conftest import FIX, GOLD, ROOT, SweepTally, check_recorded_cv_curve, free_device_bytes, hash_folds, make_bed, perm_folds, seeded_draw, tied_case
from gpu_helpers import _BT_TIE, _NUDGES, _config3_problem, _config4_problem, _dosages, _exact_xtv, _mv_problem, _row_orders, _rows_permuted, _run_probe_snippet, _same_fit, _sim, _unstable, _within_own_spread, rel

pytestmark = pytest.mark.gpu


def test_device_present_and_native_library_loaded(mih):
    assert mih.device_count() >= 1
    assert os.path.exists(mih.library_path())

def test_g1_golden_log_on_gpu(mih, normal_pair, normal_data):
    """The reference's recorded run (docs/src/man/examples.md:230-267) reproduced by the HIP path."""
    g = json.load(open(os.path.join(GOLD, "golden_normal_k7.json")))
    x, _ = normal_pair
    res = mih.fit_iht(normal_data["y"], x, normal_data["z"], k=7, verbose=False)
    assert res.iter == g["iterations"]
    np.testing.assert_allclose(res.trace["logl"], g["logl"], rtol=1e-11)
    np.testing.assert_allclose(res.trace["tol"], g["tol"], rtol=1e-8)
    assert list(res.trace["backtracks"]) == g["backtracks"]
    nz = np.flatnonzero(res.beta)
    assert list(nz + 1) == g["positions_1based"]
    np.testing.assert_allclose(res.beta[nz], g["beta_printed"], rtol=5e-6)
    np.testing.assert_allclose(res.c, g["c_printed"], rtol=5e-6)
    assert res.σg == pytest.approx(g["pve"], rel=1e-9)
    assert res.trace["lines"][0].startswith("Iteration 1: loglikelihood = -1403.60851544")

@pytest.mark.parametrize("curve", ["docs_curve", "shipped_summary_curve"])
def test_cv_curves_the_reference_recorded_on_gpu(mih, oracle, normal_pair, normal_data, curve):
    """cv_iht of the HIP path against the reference's OWN recorded curves (docs/src/man/examples.md:169-192 and
    data/cviht.summary.txt; tests/golden/golden_cv_normal.json) -- loose (the reference's folds are random), but held by the
    reference, not by the restatement -- and, on the same folds, against the oracle."""
    gold = json.load(open(os.path.join(GOLD, "golden_cv_normal.json")))
    g = gold[curve]
    x, ox = normal_pair
    y = normal_data["y"] if g["y"] == "normal_y_fam6.txt" else normal_data["y2"]
    for seed in gold["fold_seeds"]:
        folds = perm_folds(normal_data["n"], g["q"], seed)
        mse = mih.cv_iht(y, x, normal_data["z"], path=g["path"], q=g["q"], folds=folds, zkeep=g["zkeep"], verbose=False)
        check_recorded_cv_curve(mse, g)
        omse, _ = oracle.cv_iht(ox, y, normal_data["z"], path=g["path"], q=g["q"], folds=folds, zkeep=g["zkeep"])
        np.testing.assert_allclose(mse, omse, rtol=1e-8)

@pytest.mark.parametrize("family", ["normal", "bernoulli", "poisson", "negbin"])
def test_fit_iht_families_vs_oracle(mih, oracle, normal_pair, family):
    x, ox = normal_pair
    rng = np.random.default_rng(10)
    eta = _sim(oracle, ox, rng, 8)
    n = x.n
    if family == "normal":
        y, d, l, od, ol, tol = eta + 1 + rng.standard_normal(n), mih.Normal(), mih.IdentityLink(), "normal", "identity", 1e-5
    elif family == "bernoulli":
        y, d, l, od, ol, tol = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float), mih.Bernoulli(), mih.LogitLink(), "bernoulli", "logit", 1e-4
    elif family == "poisson":
        y, d, l, od, ol, tol = rng.poisson(np.exp(0.3 * eta)).astype(float), mih.Poisson(), mih.LogLink(), "poisson", "log", 1e-4
    else:
        mu = np.exp(0.3 * eta)
        y, d, l, od, ol, tol = rng.negative_binomial(10, 10 / (mu + 10)).astype(float), mih.NegativeBinomial(10.0), mih.LogLink(), "negbin", "log", 1e-4
    res = mih.fit_iht(y, x, None, k=8, d=d, l=l, verbose=False)
    o = oracle.fit_iht(ox, y, None, k=8, dist=od, link=ol, nb_r=10.0)
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))      # bit-exact support
    nz = np.flatnonzero(o["beta"])
    np.testing.assert_allclose(res.beta[nz], o["beta"][nz], rtol=tol)
    np.testing.assert_allclose(res.c, o["c"], rtol=tol)
    assert res.logl == pytest.approx(o["logl"], rel=1e-9)
    assert list(res.trace["backtracks"]) == list(o["bt_trace"])
    np.testing.assert_allclose(res.mu, o["mu"], rtol=1e-6, atol=1e-9)
    assert res.σg == pytest.approx(o["pve"], rel=1e-6)
    assert np.count_nonzero(res.beta) == 8 and res.c[0] != 0                        # L0_reg_test.jl:21-24

def test_fit_iht_zkeep_weights_train_mask(mih, oracle):
    rng = np.random.default_rng(12)
    n, p = 700, 500
    cols = make_bed(rng, n, p, 0.01)
    x = mih.SnpLinAlg(cols, n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    z = np.column_stack([np.ones(n), rng.standard_normal(n), rng.standard_normal(n)])
    y = _sim(oracle, ox, rng, 5, 0.6) + z @ np.array([1.0, 1.2, 0.0]) + rng.standard_normal(n)
    w = rng.uniform(1.0, 2.0, p)
    train = (rng.random(n) < 0.8).astype(np.uint8)
    for kw, okw in [(dict(zkeep=[1, 0, 0]), dict(zkeep=[1, 0, 0])),
                    (dict(weight=w), dict(weight=w)),
                    (dict(train=train), dict(train=train)),
                    (dict(zkeep=[1, 1, 0], weight=w, train=train), dict(zkeep=[1, 1, 0], weight=w, train=train))]:
        res = mih.fit_iht(y, x, z, k=6, verbose=False, **kw)
        o = oracle.fit_iht(ox, y, z, k=6, **okw)
        assert res.iter == o["iter"], kw.keys()
        assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
        np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(res.c, o["c"], rtol=1e-5, atol=1e-12)
        assert res.logl == pytest.approx(o["logl"], rel=1e-9)

def test_fit_iht_dense_matrix(mih, oracle):
    """The reference's Matrix{Float64} design matrix (test/L0_reg_test.jl dense cases)."""
    rng = np.random.default_rng(13)
    n, p, k = 500, 1200, 7
    X = rng.standard_normal((n, p))
    b = np.zeros(p)
    b[rng.choice(p, k, replace=False)] = rng.standard_normal(k)
    y = X @ b + 0.5 + rng.standard_normal(n)
    xd = mih.DenseMatrix(X)
    od = oracle.Mat.from_dense(X)
    r = rng.standard_normal(n)
    assert rel(xd.xtv(r), X.T @ r) < 1e-12
    res = mih.fit_iht(y, xd, None, k=k, verbose=False)
    o = oracle.fit_iht(od, y, None, k=k)
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    yb = (rng.random(n) < 1 / (1 + np.exp(-(X @ b)))).astype(float)
    res = mih.fit_iht(yb, xd, None, k=k, d=mih.Bernoulli(), l=mih.LogitLink(), verbose=False)
    o = oracle.fit_iht(od, yb, None, k=k, dist="bernoulli", link="logit")
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-4, atol=1e-12)

def test_max_iter_semantics_and_errors(mih, normal_pair, normal_data):
    x, _ = normal_pair
    res = mih.fit_iht(normal_data["y"], x, normal_data["z"], k=7, max_iter=3, verbose=False)
    assert res.iter == 3 and len(res.trace["logl"]) == 2            # fit.jl:170: max_iter=N takes N-1 steps
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(normal_data["y"][:-1], x, None, k=7, verbose=False)         # DimensionMismatch
    xs = mih.SnpLinAlg(np.zeros((4, 3), dtype=np.uint8), n=10, center=False, scale=True)
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(np.zeros(10), xs, None, k=1, verbose=False)                 # "x is not centered!"
    with pytest.raises(mih.MendelIHTError):
        mih.cv_iht(normal_data["y"], x, None, path=[x.p + 1], q=3, folds=hash_folds(x.n, 3), verbose=False)

def test_session_steps_equal_fit_trace(mih, normal_pair, normal_data):
    x, _ = normal_pair
    res = mih.fit_iht(normal_data["y"], x, normal_data["z"], k=7, verbose=False)
    s = mih.IHTSession(normal_data["y"], x, normal_data["z"], k=7)
    for i in range(res.iter):
        logl, bt, tol = s.step()
        assert logl == res.trace["logl"][i] and bt == res.trace["backtracks"][i] and tol == res.trace["tol"][i]
    s.close()

@pytest.mark.parametrize("family", ["normal", "bernoulli"])
def test_cv_iht_vs_oracle_and_sharding(mih, oracle, normal_pair, normal_data, family):
    x, ox = normal_pair
    n = x.n
    folds = hash_folds(n, 3)
    if family == "normal":
        y, z, kw, okw, tol = normal_data["y"], normal_data["z"], {}, {}, 1e-5
    else:
        rng = np.random.default_rng(20)
        eta = _sim(oracle, ox, rng, 6, 0.7)
        y, z = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float), None
        kw, okw, tol = dict(d=mih.Bernoulli(), l=mih.LogitLink()), dict(dist="bernoulli", link="logit"), 1e-4
    path = list(range(0, 7))
    mse, raw = mih.cv_iht(y, x, z, path=path, q=3, folds=folds, verbose=False, return_raw=True, **kw)
    omse, oraw = oracle.cv_iht(ox, y, z, path=path, q=3, folds=folds, **okw)
    # IHT lets the likelihood drop once max_step backtracks are used up (fit.jl:242-253); a fit that
    # does so restarts from a far-away point and amplifies last-bit differences by many orders of
    # magnitude (the reference itself is not reproducible across thread counts there).  Such
    # (fold, k) fits are identified from the ORACLE's own trace and held to a looser bar.
    stable = np.ones_like(oraw, dtype=bool)
    for f in range(3):
        for ik, k in enumerate(path):
            tr = oracle.fit_iht(ox, y, z, k=k, max_iter=100, train=(folds != f + 1).astype(np.uint8), **okw)
            stable[f, ik] = tr["bt_trace"].max(initial=0) < 3
    assert stable.mean() > 0.7
    np.testing.assert_allclose(raw[stable], oraw[stable], rtol=tol)
    np.testing.assert_allclose(raw, oraw, rtol=5e-3)
    np.testing.assert_allclose(mse, omse, rtol=tol if stable.all() else 5e-3)
    assert np.all(mse > 0)                                         # test/cv_iht_test.jl:29-34
    assert int(np.argmin(mse)) == int(np.argmin(omse))
    # the (fold,k) combinations sharded over 2 ranks sum to the unsharded result (one gather)
    parts = [mih.cv_iht(y, x, z, path=path, q=3, folds=folds, verbose=False, return_raw=True, rank=r, world=2, **kw)[1]
             for r in range(2)]
    assert np.array_equal(parts[0] + parts[1], raw)
    assert np.count_nonzero(parts[0]) + np.count_nonzero(parts[1]) == raw.size

def test_file_level_wrappers(mih, tmp_path, normal_data):
    """iht(...) / cross_validate(...) on a PLINK trio (src/wrapper.jl:52-120, 301-349): the reference's recorded run through the
    file-level API -- .fam phenotypes, covariate file, summary file (the fit's log + show(result)), the beta file with the .bim
    columns, the cross-validation summary in print_cv_results' format."""
    import shutil
    prefix = str(tmp_path / "normal")
    shutil.copy(normal_data["bed"], prefix + ".bed")
    with open(prefix + ".fam", "w") as f:
        for i, v in enumerate(normal_data["y"]):
            f.write(f"{i + 1}\t1\t0\t0\t1\t{float(v)!r}\n")
    with open(prefix + ".bim", "w") as f:
        for j in range(10_000):
            f.write(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n")
    g = json.load(open(os.path.join(GOLD, "golden_normal_k7.json")))
    res = mih.iht(prefix, 7, mih.Normal, covariates=os.path.join(FIX, "covariates.txt"), phenotypes=6,
                  summaryfile=str(tmp_path / "s.txt"), betafile=str(tmp_path / "b.txt"))
    assert list(np.flatnonzero(res.beta) + 1) == g["positions_1based"]
    assert res.logl == pytest.approx(g["final_logl"], rel=1e-11)
    # beta file: header + one tab-separated row per SNP with the .bim columns (wrapper.jl:112-116)
    rows = open(tmp_path / "b.txt").read().splitlines()
    assert rows[0] == "chr\tpos\tSNPid\tref\talt\tEstimated_beta" and len(rows) == 10_001
    cols = [r.split("\t") for r in rows[1:]]
    assert cols[3136][:5] == ["1", "3137", "snp3137", "1", "2"]
    bfile = np.array([float(c[5]) for c in cols])
    assert np.array_equal(bfile, res.beta)
    # summary file: the per-iteration log the reference recorded (docs/src/man/examples.md:230-234) and show(result)
    summ = open(tmp_path / "s.txt").read()
    its = [ln for ln in summ.splitlines() if ln.startswith("Iteration ")]
    assert len(its) == g["iterations"]
    for ln, want in zip(its, g["logl"]):
        assert float(ln.split("loglikelihood = ")[1].split(",")[0]) == pytest.approx(want, rel=1e-11)
    assert "IHT estimated 7 nonzero SNP predictors and 2 non-genetic predictors." in summ and "Selected genetic predictors:" in summ
    assert "Link functin = IdentityLink()" in summ and "Sparsity parameter (k) = 7" in summ
    # missing phenotypes: "-9" / "NA" are imputed by the mean for quantitative traits, refused for binary ones (wrapper.jl:171-214)
    y = normal_data["y"]
    with open(prefix + ".fam", "w") as f:
        for i, v in enumerate(y):
            tok = "-9" if i == 4 else ("NA" if i == 17 else repr(float(v)))
            f.write(f"{i + 1}\t1\t0\t0\t1\t{tok}\n")
    from mendeliht_amd import api
    yy = api.parse_phenotypes(prefix, 6, mih.Normal(), 1000)
    keep = np.ones(1000, bool); keep[[4, 17]] = False
    assert yy[4] == yy[17] == pytest.approx(y[keep].mean(), rel=1e-15) and np.array_equal(yy[keep], y[keep])
    with pytest.raises(mih.MendelIHTError):
        mih.iht(prefix, 3, mih.Bernoulli, summaryfile="", betafile="")
    with open(prefix + ".fam", "w") as f:
        for i, v in enumerate(y):
            f.write(f"{i + 1}\t1\t0\t0\t1\t{float(v)!r}\n")
    mse = mih.cross_validate(prefix, mih.Normal, path=range(5, 9), q=3, folds=hash_folds(1000, 3),
                             covariates=os.path.join(FIX, "covariates.txt"), cv_summaryfile=str(tmp_path / "cv.txt"),
                             verbose=False)
    assert mse.shape == (4,) and np.all(mse > 0)
    cvs = open(tmp_path / "cv.txt").read().splitlines()
    assert cvs[2] == "Crossvalidation Results:" and cvs[3] == "\tk\tMSE"
    assert [float(ln.split("\t")[2]) for ln in cvs[4:8]] == list(mse) and cvs[9] == f"Best k = {5 + int(np.argmin(mse))}"
    assert cvs[-1].startswith("Total cross validation time = ")
    # multivariate: two .fam columns -> mIHTResult, beta_1 / beta_2 columns, the covariance file
    with open(prefix + ".fam", "w") as f:
        for i, v in enumerate(y):
            f.write(f"{i + 1}\t1\t0\t0\t1\t{float(v)!r}\t{float(normal_data['y2'][i])!r}\n")
    rm = mih.iht(prefix, 10, mih.MvNormal, phenotypes=[6, 7], summaryfile=str(tmp_path / "ms.txt"), betafile=str(tmp_path / "mb.txt"),
                 covariancefile=str(tmp_path / "cov.txt"), verbose=False)
    assert rm.beta.shape == (2, 10_000) and np.count_nonzero(rm.beta) <= 10
    head = open(tmp_path / "mb.txt").readline().rstrip("\n")
    assert head == "chr\tpos\tSNPid\tref\talt\tbeta_1\tbeta_2"
    np.testing.assert_allclose(np.loadtxt(tmp_path / "cov.txt"), rm.Σ)
    assert "Trait 2's SNP PVE:" in open(tmp_path / "ms.txt").read()

def test_fit_iht_group_projection(mih, oracle):
    """Group IHT (test/L0_reg_test.jl:176-242): scalar k per group and per-group k vector."""
    rng = np.random.default_rng(31)
    n, p = 600, 1000
    cols = make_bed(rng, n, p)
    x = mih.SnpLinAlg(cols, n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    group = np.repeat(np.arange(1, 51), p // 50)
    b = np.zeros(p)
    for g0 in (3, 17, 40):
        b[(g0 - 1) * 20 + rng.choice(20, 3, replace=False)] = rng.choice([-1, 1], 3) * rng.uniform(0.4, 0.9, 3)
    mask = (b != 0).astype(np.uint8)
    y = ox.xv_masked(mask, b) + 0.7 + rng.standard_normal(n)
    res = mih.fit_iht(y, x, None, k=3, J=3, group=group, verbose=False)
    o = oracle.fit_iht(ox, y, None, k=3, J=3, group=group)
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    assert res.logl == pytest.approx(o["logl"], rel=1e-9)
    assert np.count_nonzero(res.beta) <= 9 and len(set(group[np.flatnonzero(res.beta)])) <= 3
    ks = np.full(50, 2)
    ks[[2, 16, 39]] = 3
    res = mih.fit_iht(y, x, None, k=ks, J=4, group=group, verbose=False)
    o = oracle.fit_iht(ox, y, None, k=ks, J=4, group=group)
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)

@pytest.mark.parametrize("branch", ["rolling", "debias", "init_beta"])
def test_cv_iht_with_groups_on_both_drivers(mih, oracle, branch):
    """cv_iht(group=...) sets v.k = sparsity per (fold, k) fit (cross_validation.jl:110) and project_group_sparse! reads that k
    (utilities.jl:266-268): on the rolling lock-step driver (also with init_beta and debias since round 3) every fit has its own
    IHTVariable, recycled from fit to fit: its device copy of k must follow the path (IhtVar::set_k)."""
    rng = np.random.default_rng(131)
    n, p = 500, 400
    cols = make_bed(rng, n, p)
    x = mih.SnpLinAlg(cols, n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    group = np.repeat(np.arange(1, 21), p // 20)
    b = np.zeros(p)
    b[(7 - 1) * 20 + rng.choice(20, 4, replace=False)] = rng.choice([-1, 1], 4) * rng.uniform(0.5, 0.9, 4)
    y = ox.xv_masked((b != 0).astype(np.uint8), b) + 0.3 + rng.standard_normal(n)
    folds = hash_folds(n, 3)
    kw = {"debias": {"debias": True}, "init_beta": {"init_beta": True}, "rolling": {}}[branch]
    path = [1, 2, 4, 6]
    mse, raw = mih.cv_iht(y, x, None, path=path, q=3, folds=folds, group=group, verbose=False, return_raw=True, **kw)
    omse, oraw = oracle.cv_iht(ox, y, None, path=path, q=3, folds=folds, group=group, **kw)
    np.testing.assert_allclose(raw, oraw, rtol=1e-6)
    np.testing.assert_allclose(mse, omse, rtol=1e-6)
    assert len(set(np.round(mse, 9))) == len(path)          # the model size really changed from entry to entry

@pytest.mark.parametrize("method", ["MM", "Newton"])
def test_negbin_nuisance_estimation(mih, oracle, normal_pair, method):
    """est_r=:MM / :Newton (utilities.jl:141-247; test/L0_reg_test.jl:245-296)."""
    x, ox = normal_pair
    rng = np.random.default_rng(50)
    eta = _sim(oracle, ox, rng, 6, 0.4)
    mu = np.exp(0.5 + 0.3 * eta)
    y = rng.negative_binomial(5, 5 / (mu + 5)).astype(float)
    res = mih.fit_iht(y, x, None, k=6, d=mih.NegativeBinomial(1.0), l=mih.LogLink(), est_r=method, verbose=False)
    o = oracle.fit_iht(ox, y, None, k=6, dist="negbin", link="log", nb_r=1.0, est_r=method.lower())
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-4, atol=1e-12)
    assert res.d.r == pytest.approx(o["nb_r"], rel=1e-6)
    assert res.logl == pytest.approx(o["logl"], rel=1e-8)
    assert 1.0 < res.d.r < 50.0
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(y, x, None, k=6, d=mih.Poisson(), l=mih.LogLink(), est_r="MM", verbose=False)   # fit.jl:93-94

@pytest.mark.parametrize("method", ["MM", "Newton"])
def test_cv_negbin_est_r_chains_in_lockstep(mih, oracle, method):
    """cv_iht with est_r.  The reference keeps ONE IHTVariable per Julia thread (cross_validation.jl:91) and
    never resets v.d, so the NegBin r that mle_for_r (utilities.jl:141-247) left at the end of a fit is where the thread's next
    fit starts; `Threads.@threads :static` (:100) gives each thread a contiguous block of the fold-major combinations.  The
    library runs one CHAIN of fits per emulated thread and advances the chains in lock-step: every loss against the oracle's
    restatement with the same number of threads -- 1 thread (the default, 0 = 1: one chain over the whole grid, the reference at
    Threads.nthreads() == 1), q threads (one chain per fold), and thread counts that cut folds in the middle (2, 4, 7) -- and the chains dealt out over two ranks must add
    up to the single-rank matrix bit for bit (a chain stays whole on one rank)."""
    rng = np.random.default_rng(61)
    n, p, q = 900, 260, 3
    cols = make_bed(rng, n, p, missing_rate=0.01)
    x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    eta = _sim(oracle, ox, rng, 5, 0.4)
    mu = np.exp(0.5 + 0.3 * eta)
    y = rng.negative_binomial(4, 4 / (mu + 4)).astype(float)
    folds = hash_folds(n, q)
    path = [2, 3, 5, 6, 8]                                           # 15 combinations
    seen = {}
    for T in (0, 1, 2, q, 4, 7):
        mse, raw = mih.cv_iht(y, x, None, d=mih.NegativeBinomial(1.0), l=mih.LogLink(), est_r=method, path=path, q=q, folds=folds,
                              verbose=False, return_raw=True, cv_threads=T)
        omse, oraw = oracle.cv_iht(ox, y, None, path=path, q=q, folds=folds, dist="negbin", link="log", nb_r=1.0,
                                   est_r=method.lower(), cv_threads=T)        # the same value means the same on both sides
        assert np.count_nonzero(raw) == q * len(path)
        # the Newton update stops at |dr| <= 1e-6 (utilities.jl:242): rounding-level differences move r by up to that much
        np.testing.assert_allclose(raw, oraw, rtol=1e-5, err_msg=f"cv_threads={T}")
        np.testing.assert_allclose(mse, omse, rtol=1e-5)
        halves = [mih.cv_iht(y, x, None, d=mih.NegativeBinomial(1.0), l=mih.LogLink(), est_r=method, path=path, q=q, folds=folds,
                             verbose=False, return_raw=True, cv_threads=T, rank=r, world=2)[1] for r in range(2)]
        assert np.array_equal(halves[0] + halves[1], raw), T
        assert all(np.count_nonzero(hh) > 0 for hh in halves) or T in (0, 1)
        seen[T] = raw
    # the DEFAULT is the reference's default: no cv_threads argument = 0 = 1 = Threads.nthreads() == 1, one chain over the grid
    default = mih.cv_iht(y, x, None, d=mih.NegativeBinomial(1.0), l=mih.LogLink(), est_r=method, path=path, q=q,
                         folds=folds, verbose=False, return_raw=True)[1]
    assert np.array_equal(default, seen[0]) and np.array_equal(seen[0], seen[1])
    odefault = oracle.cv_iht(ox, y, None, path=path, q=q, folds=folds, dist="negbin", link="log", nb_r=1.0, est_r=method.lower())[1]
    np.testing.assert_allclose(default, odefault, rtol=1e-5)
    # the chains matter: the first fit of a chain starts from d.r = 1, a later one from its predecessor's estimate
    assert not np.array_equal(seen[1], seen[q])
    assert np.array_equal(seen[1][0, 0], seen[q][0, 0])              # (fold 1, first k) opens a chain under either count
    # model paths with est_r ride the lock-step driver too: every fit_iht call of the reference builds its own IHTVariable
    # (cross_validation.jl:254-258), so each starts from d.r
    ll = mih.iht_run_many_models(y, x, None, d=mih.NegativeBinomial(1.0), l=mih.LogLink(), est_r=method, path=path, verbose=False)
    for kk, got in zip(path, ll):
        o = oracle.fit_iht(ox, y, None, k=kk, dist="negbin", link="log", nb_r=1.0, est_r=method.lower(), max_iter=100)
        assert got == pytest.approx(o["logl"], rel=1e-7), kk

def test_init_beta(mih, oracle, normal_pair, normal_data):
    """init_beta=true (fit.jl:80; utilities.jl:776-842; test/L0_reg_test.jl:299-320)."""
    x, ox = normal_pair
    res = mih.fit_iht(normal_data["y"], x, normal_data["z"], k=7, init_beta=True, verbose=False)
    o = oracle.fit_iht(ox, normal_data["y"], normal_data["z"], k=7, init_beta=True)
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(res.c, o["c"], rtol=1e-5)
    np.testing.assert_allclose(res.trace["logl"], o["logl_trace"], rtol=1e-9)
    assert np.count_nonzero(res.beta) == 7
    # missing data, a constant SNP (Cholesky failure branch of linreg!), a train mask and prior weights
    rng = np.random.default_rng(60)
    n, p = 500, 400
    cols = make_bed(rng, n, p, 0.03)
    cols[5, :] = 0
    xs = mih.SnpLinAlg(cols, n, center=True, scale=True, impute=True)
    oxs = oracle.Mat.from_bed_columns(cols, n)
    z = np.column_stack([np.ones(n), rng.standard_normal(n)])
    y = _sim(oracle, oxs, rng, 5, 0.7) + z @ np.array([0.5, 1.0]) + rng.standard_normal(n)
    train = (rng.random(n) < 0.8).astype(np.uint8)
    w = rng.uniform(1, 2, p)
    for kw in (dict(), dict(train=train), dict(weight=w, zkeep=[1, 0])):
        res = mih.fit_iht(y, xs, z, k=6, init_beta=True, verbose=False, **kw)
        o = oracle.fit_iht(oxs, y, z, k=6, init_beta=True, **kw)
        assert res.iter == o["iter"], kw.keys()
        assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
        np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht((y > 0).astype(float), xs, z, k=6, d=mih.Bernoulli(), l=mih.LogitLink(), init_beta=True, verbose=False)
    folds = hash_folds(n, 3)
    mse = mih.cv_iht(y, xs, z, path=[3, 5, 7], q=3, folds=folds, init_beta=True, verbose=False)
    omse, _ = oracle.cv_iht(oxs, y, z, path=[3, 5, 7], q=3, folds=folds, init_beta=True)
    np.testing.assert_allclose(mse, omse, rtol=1e-5)

def test_iht_run_many_models(mih, oracle, normal_pair, normal_data, capsys):
    """iht_run_many_models (cross_validation.jl:232-273): one full-data fit per model size, max_iter = 100."""
    x, ox = normal_pair
    y, z = normal_data["y"], normal_data["z"]
    path = [1, 3, 7, 12]
    ll = mih.iht_run_many_models(y, x, z, path=path, verbose=True)
    assert "loglikelihood" in capsys.readouterr().out
    want = [oracle.fit_iht(ox, y, z, k=k, max_iter=100)["logl"] for k in path]
    np.testing.assert_allclose(ll, want, rtol=1e-10)
    assert np.all(np.diff(ll) > 0)                                   # more predictors, no hold-out: logl grows
    halves = [mih.iht_run_many_models(y, x, z, path=path, verbose=False, rank=r, world=2) for r in range(2)]
    assert np.array_equal(halves[0] + halves[1], ll)                 # sharding over ranks
    # the sequential branch (debias is not batched) and a GLM family through the lock-step branch
    lld = mih.iht_run_many_models(y, x, z, path=[3, 7], debias=True, verbose=False)
    np.testing.assert_allclose(lld, [oracle.fit_iht(ox, y, z, k=k, max_iter=100, debias=True)["logl"] for k in (3, 7)], rtol=1e-9)
    rng = np.random.default_rng(4)
    yb = (rng.random(x.n) < 0.5).astype(float)
    llb = mih.iht_run_many_models(yb, x, None, path=[2, 5], d=mih.Bernoulli, verbose=False)     # canonical link
    np.testing.assert_allclose(llb, [oracle.fit_iht(ox, yb, None, k=k, max_iter=100, dist="bernoulli", link="logit")["logl"] for k in (2, 5)], rtol=1e-8)

def test_concurrent_fits_share_one_matrix(mih, normal_pair, normal_data):
    """SURVEY 8b threading row: cv_iht calls the path from several host threads on a SHARED x
    (cross_validation.jl:100-112); the handle is immutable, every fit has its own workspace and stream."""
    import threading

    x, _ = normal_pair
    y, z = normal_data["y"], normal_data["z"]
    ks = [3, 5, 7, 9, 11, 13]
    want = [mih.fit_iht(y, x, z, k=k, verbose=False) for k in ks]
    got = [None] * len(ks)
    errs = []

    def work(i):
        try:
            got[i] = mih.fit_iht(y, x, z, k=ks[i], verbose=False)
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(ks))]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs
    for a, b in zip(want, got):
        assert np.array_equal(a.beta, b.beta) and np.array_equal(a.c, b.c) and a.logl == b.logl and a.iter == b.iter

@pytest.mark.parametrize("case", ["gamma_log", "invgauss_log", "bernoulli_probit", "bernoulli_cloglog", "bernoulli_cauchit",
                                  "poisson_sqrt", "gamma_inverse"])
def test_more_families_and_links(mih, oracle, normal_pair, case):
    """Gamma / InverseGaussian (loglik_obs, src/utilities.jl:34-35) and the remaining GLM.jl links as `l`."""
    x, ox = normal_pair
    n = x.n
    rng = np.random.default_rng(60)
    eta = 0.25 * _sim(oracle, ox, rng, 6)
    kw = {}
    if case == "gamma_log":
        y, d, l, od, ol = rng.gamma(5.0, np.exp(eta + 0.5) / 5.0), mih.Gamma(), mih.LogLink(), "gamma", "log"
    elif case == "invgauss_log":
        y, d, l, od, ol = rng.wald(np.exp(eta + 0.5), 8.0), mih.InverseGaussian(), mih.LogLink(), "invgauss", "log"
    elif case == "bernoulli_probit":
        from scipy import stats
        y, d, l, od, ol = (rng.random(n) < stats.norm.cdf(2 * eta)).astype(float), mih.Bernoulli(), mih.ProbitLink(), "bernoulli", "probit"
    elif case == "bernoulli_cloglog":
        y, d, l, od, ol = (rng.random(n) < 1 - np.exp(-np.exp(2 * eta - 0.5))).astype(float), mih.Bernoulli(), mih.CloglogLink(), "bernoulli", "cloglog"
    elif case == "bernoulli_cauchit":
        y, d, l, od, ol = (rng.random(n) < 0.5 + np.arctan(3 * eta) / np.pi).astype(float), mih.Bernoulli(), mih.CauchitLink(), "bernoulli", "cauchit"
    elif case == "poisson_sqrt":
        y, d, l, od, ol = rng.poisson((1.5 + eta) ** 2).astype(float), mih.Poisson(), mih.SqrtLink(), "poisson", "sqrt"
    else:                                                    # canonical link of Gamma; few steps (the domain eta > 0 is not enforced)
        y, d, l, od, ol = rng.gamma(5.0, 1.0 / (5.0 * (1.5 + eta))), mih.Gamma(), mih.InverseLink(), "gamma", "inverse"
        kw = dict(max_iter=4)
    try:
        o = oracle.fit_iht(ox, y, None, k=6, dist=od, link=ol, **kw)
    except RuntimeError:
        o = None                                             # NaN loglikelihood in the reference algorithm itself
    if o is None or not np.isfinite(o["logl"]):
        with pytest.raises(mih.MendelIHTError):
            mih.fit_iht(y, x, None, k=6, d=d, l=l, verbose=False, **kw)
        return
    res = mih.fit_iht(y, x, None, k=6, d=d, l=l, verbose=False, **kw)
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    nz = np.flatnonzero(o["beta"])
    np.testing.assert_allclose(res.beta[nz], o["beta"][nz], rtol=1e-4)
    np.testing.assert_allclose(res.c, o["c"], rtol=1e-4)
    assert res.logl == pytest.approx(o["logl"], rel=1e-8)
    assert list(res.trace["backtracks"]) == list(o["bt_trace"])
    assert type(mih.canonicallink(d)).__name__ in ("InverseLink", "InverseSquareLink", "LogitLink", "LogLink")

@pytest.mark.parametrize("family", ["normal", "bernoulli", "poisson"])
def test_debias(mih, oracle, normal_pair, normal_data, family):
    """debias=true (fit.jl:188 + debias!, utilities.jl:1014-1020): GLM refit of the support after a step that
    kept it.  The reference delegates to GLM.jl's IRLS, restated in the oracle (parity unpinned)."""
    x, ox = normal_pair
    n = x.n
    rng = np.random.default_rng(90)
    eta = 0.6 * _sim(oracle, ox, rng, 7)
    if family == "normal":
        y, z, kw, okw, tol = normal_data["y"], normal_data["z"], {}, {}, 1e-5
    elif family == "bernoulli":
        y, z = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float), None
        kw, okw, tol = dict(d=mih.Bernoulli(), l=mih.LogitLink()), dict(dist="bernoulli", link="logit"), 1e-4
    else:
        y, z = rng.poisson(np.exp(0.5 * eta)).astype(float), None
        kw, okw, tol = dict(d=mih.Poisson(), l=mih.LogLink()), dict(dist="poisson", link="log"), 1e-4
    res = mih.fit_iht(y, x, z, k=7, debias=True, verbose=False, **kw)
    o = oracle.fit_iht(ox, y, z, k=7, debias=True, **okw)
    plain = oracle.fit_iht(ox, y, z, k=7, **okw)
    assert res.iter == o["iter"] and list(res.trace["backtracks"]) == list(o["bt_trace"])
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    nz = np.flatnonzero(o["beta"])
    np.testing.assert_allclose(res.beta[nz], o["beta"][nz], rtol=tol)
    np.testing.assert_allclose(res.c, o["c"], rtol=tol)
    np.testing.assert_allclose(res.trace["logl"], o["logl_trace"], rtol=1e-8)
    np.testing.assert_allclose(res.trace["tol"], o["tol_trace"], rtol=1e-4, atol=1e-10)
    assert not np.array_equal(o["tol_trace"], plain["tol_trace"])          # debiasing really happened
    if family == "normal":                                                 # a refit support is the least-squares solution
        folds = hash_folds(n, 3)
        mse = mih.cv_iht(y, x, z, path=[3, 7], q=3, folds=folds, debias=True, verbose=False)
        omse, _ = oracle.cv_iht(ox, y, z, path=[3, 7], q=3, folds=folds, debias=True)
        np.testing.assert_allclose(mse, omse, rtol=1e-5)
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(np.vstack([y, y]), x, None, k=4, debias=True, verbose=False)   # multivariate: disabled in the reference

def _debias_wide_problem(oracle, ox, family, k):
    """A response with k planted effects on the shipped matrix for the debias fits beyond one 16-column Gram tile."""
    rng = np.random.default_rng([91, k])
    eta = _sim(oracle, ox, rng, k, scale=1.0 / np.sqrt(k))
    if family == "normal":
        return 2.0 * eta + 0.5 + rng.standard_normal(ox.n), {}, {}, 1e-5
    # (effects of 0.6 / sqrt(20) and 0.9 / sqrt(40) a column: the oracle's support settles within 20 steps; weaker or stronger ones
    # at these k send it through 40 to 200 steps of a support that keeps changing)
    return rng.poisson(np.exp((0.3 + 0.015 * k) * eta)).astype(float), dict(d="Poisson", l="LogLink"), dict(dist="poisson", link="log"), 1e-4

@pytest.mark.parametrize("k", [20, 40])
@pytest.mark.parametrize("family", ["normal", "poisson"])
def test_debias_support_beyond_one_gram_tile(mih, oracle, normal_pair, family, k):
    """test_debias with k + 1 > 16: the refit's Gram has several 16 x 16 tiles (k = 20: the pairs (0, 0), (0, 1), (1, 1); k = 40: six
    pairs), the right-hand side lives in another tile than most rows.  The assertions are test_debias's."""
    x, ox = normal_pair
    y, kw, okw, tol = _debias_wide_problem(oracle, ox, family, k)
    kw = {key: getattr(mih, v)() for key, v in kw.items()}
    res = mih.fit_iht(y, x, None, k=k, debias=True, verbose=False, **kw)
    o = oracle.fit_iht(ox, y, None, k=k, debias=True, **okw)
    plain = oracle.fit_iht(ox, y, None, k=k, **okw)
    assert res.iter == o["iter"] and list(res.trace["backtracks"]) == list(o["bt_trace"])
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    nz = np.flatnonzero(o["beta"])
    assert nz.size == k
    np.testing.assert_allclose(res.beta[nz], o["beta"][nz], rtol=tol)
    np.testing.assert_allclose(res.c, o["c"], rtol=tol)
    np.testing.assert_allclose(res.trace["logl"], o["logl_trace"], rtol=1e-8)
    np.testing.assert_allclose(res.trace["tol"], o["tol_trace"], rtol=1e-4, atol=1e-10)
    assert not np.array_equal(o["tol_trace"], plain["tol_trace"])          # debiasing really happened

def test_debias_cv_path_across_the_gram_tile(mih, oracle, normal_pair):
    """cv_iht with debias over the model sizes 15, 17 and 33: the lock-step fits' call of the refit (csrc/fit_lockstep.hip) with one,
    two and three column tiles of the Gram, against the oracle at test_debias's tolerance."""
    x, ox = normal_pair
    y = _debias_wide_problem(oracle, ox, "normal", 33)[0]
    folds = hash_folds(x.n, 3)
    mse = mih.cv_iht(y, x, None, path=[15, 17, 33], q=3, folds=folds, debias=True, verbose=False)
    omse, _ = oracle.cv_iht(ox, y, None, path=[15, 17, 33], q=3, folds=folds, debias=True)
    np.testing.assert_allclose(mse, omse, rtol=1e-5)
    plain, _ = oracle.cv_iht(ox, y, None, path=[15, 17, 33], q=3, folds=folds)
    assert not np.array_equal(omse, plain)                                 # debiasing really happened

def test_snplinalg_fit_equals_dense_copy(mih, oracle):
    """test/L0_reg_test.jl:340-348, 361-363: the memory-efficient SnpLinAlg path and a dense Float64 copy of
    the same standardized matrix give the same model (here both on the GPU: 2-bit MFMA path vs f64 path)."""
    rng = np.random.default_rng(17)
    n, p, k = 1203, 517, 6
    cols = make_bed(rng, n, p, missing_rate=0.01)
    xs = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    mu, sinv = xs.mu_sigma()
    padded = np.unpackbits(cols, axis=1, bitorder="little").reshape(p, -1, 2)[:, :n, :]
    code = padded[:, :, 0] + 2 * padded[:, :, 1]                          # PLINK 2-bit codes, LSB first
    g = np.select([code == 0, code == 2, code == 3], [0.0, 1.0, 2.0], default=np.nan)
    g = np.where(np.isnan(g), mu[:, None], g)                              # impute -> mean
    D = np.asfortranarray(((g - mu[:, None]) * sinv[:, None]).T)           # n x p standardized dense copy
    xd = mih.DenseMatrix(D)
    r = rng.standard_normal(n)
    assert rel(xs.xtv(r), xd.xtv(r)) < 1e-11
    supp = rng.choice(p, k, replace=False)
    eta = D[:, supp] @ rng.standard_normal(k)
    for y, kw, tol in ((eta + 1 + rng.standard_normal(n), {}, 1e-8),
                       ((rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float), dict(d=mih.Bernoulli(), l=mih.LogitLink()), 1e-6)):
        a = mih.fit_iht(y, xs, None, k=k, verbose=False, **kw)
        b = mih.fit_iht(y, xd, None, k=k, verbose=False, **kw)
        assert a.iter == b.iter and np.array_equal(np.flatnonzero(a.beta), np.flatnonzero(b.beta))
        np.testing.assert_allclose(a.beta, b.beta, rtol=tol, atol=1e-12)
        assert a.logl == pytest.approx(b.logl, rel=1e-10)

def test_large_k_and_many_covariates(mih, oracle, normal_pair, normal_data):
    """Buffers that grow with the model: k = 1500 of p = 10 000 SNPs, and q = 24 covariates of which 19 compete
    with the SNPs in the projection (zkeep false); q beyond the library limit is rejected."""
    x, ox = normal_pair
    n = x.n
    rng = np.random.default_rng(70)
    y = normal_data["y"]
    res = mih.fit_iht(y, x, None, k=1500, verbose=False, max_iter=12)
    o = oracle.fit_iht(ox, y, None, k=1500, max_iter=12)
    assert res.iter == o["iter"] and np.count_nonzero(res.beta) == 1500
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    q = 24
    z = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    yz = y + z[:, 5] * 0.8 - z[:, 17] * 0.6
    zk = [1] * 5 + [0] * (q - 5)
    res = mih.fit_iht(yz, x, z, k=9, zkeep=zk, verbose=False)
    o = oracle.fit_iht(ox, yz, z, k=9, zkeep=zk)
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    assert np.array_equal(np.flatnonzero(res.c), np.flatnonzero(o["c"]))
    np.testing.assert_allclose(res.c, o["c"], rtol=1e-5, atol=1e-12)
    assert res.c[5] != 0 and res.c[17] != 0                      # the two real covariate effects survive the projection
    z64 = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(63)])       # the library maximum q = 64
    res = mih.fit_iht(y, x, z64, k=4, verbose=False)
    o = oracle.fit_iht(ox, y, z64, k=4)
    assert res.iter == o["iter"] and np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.c, o["c"], rtol=1e-5, atol=1e-12)
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(y, x, np.ones((n, 65)), k=3, verbose=False)

def test_cv_iht_over_replicas_in_one_process(mih, normal_data):
    """mih_cv_iht_multi: one host thread per matrix replica (one per GPU; here both on the single test GPU),
    the (fold,k) grid split between them -- same losses as the single-replica call."""
    n = normal_data["n"]
    bed = mih.read_bed(normal_data["bed"], n)
    xa = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    xb = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    y, z = normal_data["y"], normal_data["z"]
    folds = hash_folds(n, 3)
    path = list(range(1, 9))
    one, raw1 = mih.cv_iht(y, xa, z, path=path, q=3, folds=folds, verbose=False, return_raw=True)
    two, raw2 = mih.cv_iht(y, [xa, xb], z, path=path, q=3, folds=folds, verbose=False, return_raw=True)
    assert np.array_equal(raw1, raw2) and np.array_equal(one, two)
    three = mih.cv_iht(y, [xa, xb, xa], z, path=path, q=3, folds=folds, verbose=False, d=mih.Normal())
    assert np.array_equal(three, one)
    with pytest.raises(mih.MendelIHTError):
        mih.cv_iht(y, [xa, mih.SnpLinAlg(bed[:100], n, center=True, scale=True)], z, path=path, q=3, folds=folds, verbose=False)

def _fits_case(mih, oracle, rng, trial, fams):
    """One random fit of test_randomized_fits_vs_oracle (replayed by tools/repro_fuzz.py)."""
    n = int(rng.integers(60, 2500)); p = int(rng.integers(40, 600)); k = int(rng.integers(1, 10))
    miss = float(rng.choice([0.0, 0.02, 0.1])); q = int(rng.integers(1, 4))
    od, ol, D, L, tol = fams[int(rng.integers(0, 3))]
    kind = str(rng.choice(["snp", "snp", "snp", "dense64", "dense32"]))       # (the reference's x::Matrix{Float64} / Matrix{Float32} callers too)
    if kind == "snp":
        cols = make_bed(rng, n, p, missing_rate=miss)
        x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
        ox = oracle.Mat.from_bed_columns(cols, n)
    else:
        X = rng.standard_normal((n, p)).astype(np.float32 if kind == "dense32" else np.float64)
        x = mih.DenseMatrix(X)
        ox = oracle.Mat.from_dense(X.astype(np.float64))              # the upcast is exact: same matrix on both sides
        miss = kind
    z = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    eta = 0.5 * _sim(oracle, ox, rng, min(k, 5)) + z @ (rng.standard_normal(q) * 0.3)
    if kind != "snp":
        eta *= 0.5                                                   # (unit-variance columns with unbounded entries: keep the counts moderate)
    y = {"normal": eta + rng.standard_normal(n),
         "bernoulli": (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float),
         "poisson": rng.poisson(np.exp(np.clip(0.5 * eta, -3, 3))).astype(float)}[od]
    kw = {}
    if q > 1 and rng.random() < 0.5:
        kw["zkeep"] = [1] + [int(v) for v in rng.integers(0, 2, q - 1)]
    if rng.random() < 0.4:
        kw["weight"] = rng.uniform(0.5, 2.0, p)
    if rng.random() < 0.4:
        kw["train"] = (rng.random(n) < 0.8).astype(np.uint8)
    return n, p, k, miss, q, od, ol, D, L, tol, x, ox, y, z, kw

def test_randomized_fits_vs_oracle(mih, oracle):
    """A seeded sweep over shapes, missing rates, families, covariates, zkeep masks, prior weights, train masks
    and k: the GPU fit must track the oracle (same support and iteration log) on every stable trajectory."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 20260)))     # other seeds: extended sweeps by hand
    fams = [("normal", "identity", mih.Normal, mih.IdentityLink, 1e-5), ("bernoulli", "logit", mih.Bernoulli, mih.LogitLink, 1e-4),
            ("poisson", "log", mih.Poisson, mih.LogLink, 1e-4)]
    tally = SweepTally("fits", ceiling=1, floor=13)
    for trial in range(14):
        n, p, k, miss, q, od, ol, D, L, tol, x, ox, y, z, kw = _fits_case(mih, oracle, rng, trial, fams)
        tag = (trial, n, p, k, od, q, miss, sorted(kw))

        def orc(g=1.0):                                  # None: the reference algorithm itself ends in an error (NaN / Inf loglikelihood, fit.jl:259-260)
            try:
                return oracle.fit_iht(ox, y, z * g, k=k, dist=od, link=ol, max_iter=60, **kw)
            except RuntimeError:
                return None
        o = orc()
        try:
            res = mih.fit_iht(y, x, z, k=k, d=D(), l=L(), max_iter=60, verbose=False, **kw)
        except mih.MendelIHTError:
            res = None
        if o is None or res is None:
            if (o is None) != (res is None):             # only one side failed: a finding unless the oracle wavers itself (seed 9015 of tools/fuzz_parity.py)
                assert len({orc(g) is None for g in _NUDGES} | {o is None}) == 2, (tag, "only one side ended in an error", o is None, res is None)
                tally.set_aside("only one side ends in an error, the oracle wavers under nudges", tag)
            else:
                tally.ok()
            continue
        #  a trajectory that used up max_step backtracks is no longer skipped wholesale: it is compared like any other and
        # set aside -- counted, under the sweep's ceiling -- only when it differs
        try:
            assert res.iter == o["iter"], tag
            assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"])), tag
            np.testing.assert_allclose(res.beta, o["beta"], rtol=tol, atol=1e-10, err_msg=str(tag))
            np.testing.assert_allclose(res.c, o["c"], rtol=tol, atol=1e-10, err_msg=str(tag))
            assert res.logl == pytest.approx(o["logl"], rel=1e-8), tag
        except AssertionError:
            pick = lambda d, g=1.0: dict(iter=d["iter"], beta=d["beta"], c=d["c"] * g, logl=d["logl"])
            nudged = [orc(g) for g in _NUDGES]
            if o["eta_cond"] < 1e-18 or any(v is None or _unstable(pick(o), pick(v, g), tol) for v, g in zip(nudged, _NUDGES)):
                tally.set_aside("0/0 step size" if o["eta_cond"] < 1e-18 else "oracle unstable under ulp nudges", tag)
                continue                              # the oracle does not agree with itself on this one
            def orc_rows(pm):                         # the same problem, its samples in another order (_rows_permuted)
                kr = dict(kw, train=kw["train"][pm]) if "train" in kw else kw
                try:
                    return oracle.fit_iht(_rows_permuted(oracle, ox, pm), y[pm], z[pm], k=k, dist=od, link=ol, max_iter=60, **kr)
                except RuntimeError:
                    return None
            rows = [orc_rows(pm) for pm in _row_orders(len(y))]
            if any(v is None or _unstable(pick(o), pick(v), tol) for v in rows):
                tally.set_aside("oracle unstable under another order of its rows", tag)
                continue
            if o["bt_cond"] < _BT_TIE and not np.array_equal(o["bt_trace"], res.trace["backtracks"][:len(o["bt_trace"])]):
                # the two loglikelihoods of a backtracking decision agree to the last bits (iht_oracle.h, bt_cond) and the two
                # sides decided it differently: the converging step of seed 9878, halved twice here and not at all on the device
                tally.set_aside("a backtracking decision between loglikelihoods equal to rounding", tag)
                continue
            # (round 6: "differs after a step that used up max_step backtracks" is no longer accepted by argument, see the options sweep)
            if res.iter == o["iter"] and np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"])) and \
               _within_own_spread(o, [pick(v, g) for v, g in zip(nudged, _NUDGES)] + [pick(v) for v in rows],
                                  dict(beta=res.beta, c=res.c, logl=res.logl), dict(beta=(tol, 1e-10), c=(tol, 1e-10), logl=(1e-8, 0.0))):
                tally.set_aside("within the tolerance plus four times the oracle's own spread under re-association", tag)
                continue
            raise
        tally.ok()
    tally.finish()

def _options_case(mih, oracle, rng, trial):
    """One random case of test_randomized_options_vs_oracle (also replayed by hand when a seed of tools/fuzz_parity.py fails)."""
    from scipy import stats
    n = int(rng.integers(120, 1800)); p = int(rng.integers(60, 500)); q = int(rng.integers(1, 4))
    miss = float(rng.choice([0.0, 0.02]))
    cols = make_bed(rng, n, p, missing_rate=miss, maf_lo=0.05)
    x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    z = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    eta = 0.4 * _sim(oracle, ox, rng, 5) + z @ np.concatenate([[0.3], rng.standard_normal(q - 1) * 0.2])
    fam = str(rng.choice(["normal", "bernoulli_probit", "bernoulli_cloglog", "poisson", "poisson_sqrt", "negbin", "negbin_mm",
                          "negbin_newton", "gamma", "invgauss"]))
    kw, okw, tol = {}, {}, 1e-4
    if fam == "normal":
        y, tol = eta + rng.standard_normal(n), 1e-5
    elif fam == "bernoulli_probit":
        y = (rng.random(n) < stats.norm.cdf(eta)).astype(float)
        kw, okw = dict(d=mih.Bernoulli(), l=mih.ProbitLink()), dict(dist="bernoulli", link="probit")
    elif fam == "bernoulli_cloglog":
        y = (rng.random(n) < 1 - np.exp(-np.exp(eta - 0.5))).astype(float)
        kw, okw = dict(d=mih.Bernoulli(), l=mih.CloglogLink()), dict(dist="bernoulli", link="cloglog")
    elif fam == "poisson":
        y = rng.poisson(np.exp(np.clip(eta, -3, 3))).astype(float)
        kw, okw = dict(d=mih.Poisson(), l=mih.LogLink()), dict(dist="poisson", link="log")
    elif fam == "poisson_sqrt":
        y = rng.poisson((1.5 + np.clip(0.5 * eta, -1, 3)) ** 2).astype(float)
        kw, okw = dict(d=mih.Poisson(), l=mih.SqrtLink()), dict(dist="poisson", link="sqrt")
    elif fam.startswith("negbin"):
        mu = np.exp(0.5 + np.clip(0.5 * eta, -3, 3))
        y = rng.negative_binomial(4, 4 / (mu + 4)).astype(float)
        est = {"negbin": None, "negbin_mm": "MM", "negbin_newton": "Newton"}[fam]
        r0 = float(rng.choice([1.0, 4.0]))
        kw, okw = dict(d=mih.NegativeBinomial(r0), l=mih.LogLink()), dict(dist="negbin", link="log", nb_r=r0)
        if est:
            kw["est_r"], okw["est_r"] = est, est.lower()
    elif fam == "gamma":
        y = rng.gamma(5.0, np.exp(np.clip(0.5 * eta, -3, 3) + 0.5) / 5.0)
        kw, okw = dict(d=mih.Gamma(), l=mih.LogLink()), dict(dist="gamma", link="log")
    else:
        y = rng.wald(np.exp(np.clip(0.5 * eta, -3, 3) + 0.5), 8.0)
        kw, okw = dict(d=mih.InverseGaussian(), l=mih.LogLink()), dict(dist="invgauss", link="log")
    both = {}
    mode = str(rng.choice(["plain", "group", "group_ks", "debias", "init_beta"]))
    k = int(rng.integers(1, 9))
    if mode.startswith("group"):
        G = int(rng.integers(3, 12))
        group = np.sort(rng.integers(1, G + 1, p))
        group[:G] = np.arange(1, G + 1)                     # every label 1..G occurs (project_group_sparse! wants 1..G)
        group = np.sort(group)
        both["group"], both["J"] = group, int(rng.integers(1, G + 1))
        k = rng.integers(1, 4, G) if mode == "group_ks" else int(rng.integers(1, 4))
    elif mode == "debias":
        both["debias"] = True
    elif mode == "init_beta" and fam == "normal":
        both["init_beta"] = True
    if q > 1 and rng.random() < 0.4:
        both["zkeep"] = [1] + [int(v) for v in rng.integers(0, 2, q - 1)]
    if rng.random() < 0.3 and not mode.startswith("group"):
        both["weight"] = rng.uniform(0.5, 2.0, p)
    tag = (trial, n, p, q, miss, fam, mode, np.ravel(k).tolist(), sorted(both))
    return x, ox, y, z, k, kw, okw, both, tol, fam, tag

def test_randomized_options_vs_oracle(mih, oracle):
    """Seeded sweep over the keyword surface the first sweep leaves out: group / J / vector k (doubly sparse projection), debias,
    init_beta, NegativeBinomial with est_r, Gamma / InverseGaussian, non-canonical links -- combined at random, on random
    shapes with missing genotypes, against the oracle on every trajectory the oracle itself reproduces (_unstable)."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 4242)))
    tally = SweepTally("options", ceiling=1, floor=11)
    for trial in range(12):
        x, ox, y, z, k, kw, okw, both, tol, fam, tag = _options_case(mih, oracle, rng, trial)

        def orc(yy, zz, g=1.0):                              # None: the reference algorithm itself ends in an error
            try:                                             # (NaN / Inf loglikelihood, fit.jl:259-260; GLM.jl's refit failing inside debias!)
                d = oracle.fit_iht(ox, yy, zz, k=k, max_iter=40, **okw, **both)
            except RuntimeError as e:
                halved.append(e.db_minstep < 1.0)
                return None
            halved.append(d["db_minstep"] < 1.0)
            return dict(iter=d["iter"], beta=d["beta"], c=d["c"] * g, logl=d["logl"], nb_r=d["nb_r"], bt=d["bt_trace"], eta_cond=d["eta_cond"], ib_cond=d["ib_cond"], bt_cond=d["bt_cond"])
        halved = []                                          # per oracle run: did an IRLS iteration of a debias! refit halve its step (orc_result.db_minstep)
        o = orc(y, z)
        try:
            res = mih.fit_iht(y, x, z, k=k, max_iter=40, verbose=False, **kw, **both)
        except mih.MendelIHTError:
            res = None
        if o is None and res is None:
            tally.ok()                                       # both sides end in the reference's error
            continue
        try:
            assert o is not None and res is not None, (tag, "only one side ended in an error", o is None, res is None)
            assert res.iter == o["iter"], tag
            assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"])), tag
            np.testing.assert_allclose(res.beta, o["beta"], rtol=tol, atol=1e-9, err_msg=str(tag))
            np.testing.assert_allclose(res.c, o["c"], rtol=tol, atol=1e-9, err_msg=str(tag))
            estr = fam in ("negbin_mm", "negbin_newton")       # r's updates stop at |dr| <= 1e-6 (utilities.jl:242): rounding moves r, and the loglikelihood with it, by that much
            assert res.logl == pytest.approx(o["logl"], rel=1e-5 if estr else 1e-7), tag
            if estr:                                           # (counts that are not overdispersed send r to 1e8 and beyond, where it no longer matters: compare 1/r)
                assert 1.0 / res.d.r == pytest.approx(1.0 / o["nb_r"], rel=1e-5, abs=1e-5), tag
        except AssertionError:
            # Is the ORACLE's own answer conditioned well enough to hold anybody to it?  Ulp-sized scalings of the covariates
            # re-draw its rounding noise.  They cannot see one case, which the oracle reports itself (eta_cond, iht_oracle.h):
            # seed 3087 -- after an exact line search on a one-SNP support (group initialisation, utilities.jl:427-429) the
            # score on the support is a rounding residue, 1e-12 in one implementation and 5e-14 in the other, the intercept's
            # 3e-14, and iht_stepsize!'s ratio of such numbers comes out anywhere between 1/|x|^2 = 1/811 and 1/n = 1/792; seed 4036 --
            # empty initial support (vector k) and an intercept score that sums to exactly 0 on the GPU, 1e-13 in the oracle: 0/0 -> the
            # 1e-8 guard of utilities.jl:760-761 on one side, a step of 1/sum(w) on the other.
            variants = [orc(y, z * g, g) for g in _NUDGES]
            strip = lambda d: {key: d[key] for key in ("iter", "beta", "c", "logl")}
            utol = 1e-5 if fam in ("negbin_mm", "negbin_newton") else tol      # (what the comparison above holds the loglikelihood of an est_r fit to: a NegBin r that runs off to 1e8 .. 1e12 on counts without overdispersion moves it by 1e-4, seed 9024)
            if (o is not None and (o["eta_cond"] < 1e-18 or o["ib_cond"] < 1e-10)) or \
               any((v is None) != (o is None) or (v is not None and _unstable(strip(o), strip(v), utol, atol=1e-9)) for v in variants):
                tally.set_aside("0/0 step size" if (o is not None and o["eta_cond"] < 1e-18) else
                                "init_beta: a constant predictor (rounding residue as Cholesky pivot)" if (o is not None and o["ib_cond"] < 1e-10) else
                                "oracle unstable under ulp nudges", tag)
                continue
            # (round 6, VERDICT r5 weak item 1: two classes used to be accepted here by argument -- "differs after a step that used up
            # max_step backtracks" and the tie below when a max_step step came first.  Over seeds 16100 .. 16359 of tools/fuzz_parity.py,
            # 18 trials in the first class, ALL Poisson / Gamma with a non-canonical link and debias: 15 are caught by the row orders below,
            # one is the tie, one is within the oracle's own spread, one is the crawl of debias!'s refit.  Nothing is accepted by argument now.)
            # ... the same PROBLEM with its samples in another order: every sum re-associated, the freedom any other implementation has
            # (_rows_permuted).  The z nudges reach the sums only through zc -- and debias!, which fits the SNP columns alone, not at all
            def orc_rows(pm):
                try:
                    d = oracle.fit_iht(_rows_permuted(oracle, ox, pm), y[pm], z[pm], k=k, max_iter=40, **okw, **both)
                except RuntimeError:
                    return None
                return {key: d[key] for key in ("iter", "beta", "c", "logl")}
            rows = [orc_rows(pm) for pm in _row_orders(len(y))]
            if any((v is None) != (o is None) or (v is not None and _unstable(strip(o), v, utol, atol=1e-9)) for v in rows):
                tally.set_aside("oracle unstable under another order of its rows", tag)
                continue
            if o is not None and res is not None and o["bt_cond"] < _BT_TIE and not np.array_equal(o["bt"], res.trace["backtracks"][:len(o["bt"])]):
                tally.set_aside("a backtracking decision between loglikelihoods equal to rounding", tag)      # (seeds 9878, 16262)
                continue
            # ... stable by the tolerance, but not by much: the oracle's own answers, re-associated, spread over a good part of it (seed
            # 16276: an effect of 0.008 moves by 8e-7 from one row order to the next, the device's is 1.5e-6 away, the tolerance is 8e-7).
            # The device is held to the tolerance plus four times the oracle's own spread
            if o is not None and res is not None and res.iter == o["iter"] and np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"])):
                own = [v for v in variants + rows if v is not None]
                ltol = 1e-5 if fam in ("negbin_mm", "negbin_newton") else 1e-7
                if _within_own_spread(o, own, dict(beta=res.beta, c=res.c, logl=res.logl), dict(beta=(tol, 1e-9), c=(tol, 1e-9), logl=(ltol, 0.0))):
                    tally.set_aside("within the tolerance plus four times the oracle's own spread under re-association", tag)
                    continue
            # ... debias!'s GLM refit crawling by halved steps: the oracle reports it (orc_result.db_minstep, iht_oracle.h; seed 16330)
            if both.get("debias") and any(halved):
                tally.set_aside("debias!: the GLM refit halves its steps (the oracle's report)", tag)
                continue
            raise
        tally.ok()
    tally.finish()

def test_randomized_genotype_linear_algebra(mih, oracle):
    """Seeded sweep of the genotype linear algebra itself: row counts around every tile boundary of the kernels (the 4-per-byte
    packing, the 128-row MFMA step, the 2^18-row slices), a single SNP up to a few thousand, missing rates up to 30 %, the
    center / scale / impute flags, 1..40 residuals per fused pass with scales from 1e-200 to 1e+200 in ONE pass, every
    residual format -- mu, sigma^-1, X'R and X b against the oracle, the fused pass against the single pass bit for bit."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 9001)))
    edges = np.array([1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 4095, 4097])
    for trial in range(10):
        n = int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(1, 20000))
        if trial == 0 and os.environ.get("MIH_SWEEP_SEED") is None:
            n = (1 << 18) + int(rng.integers(-3, 4))                       # one committed case straddling a row slice
        p = int(rng.choice([1, 2, 3, 15, 16, 17, 31, 33, 64, 100, 257])) if rng.random() < 0.6 else int(rng.integers(1, 3000))
        if n * p > 6e7:
            p = max(1, int(6e7 // n))
        miss = float(rng.choice([0.0, 0.0, 0.01, 0.3])) if n >= 64 else 0.0   # (a SNP with every sample missing has no mean: not a case of the reference)
        flags = dict(center=bool(rng.random() < 0.8), scale=bool(rng.random() < 0.8), impute=bool(rng.random() < 0.8))
        cols = make_bed(rng, n, p, missing_rate=miss, maf_lo=0.0)          # maf 0: monomorphic SNPs (sigma^-1 = 1) included
        x = mih.SnpLinAlg(cols, n=n, **flags)
        ox = oracle.Mat.from_bed_columns(cols, n, **flags)
        tag = (trial, n, p, miss, flags)
        mu, sinv = x.mu_sigma()
        omu, osinv = ox.mu_sinv()
        assert np.array_equal(mu, omu) and np.array_equal(sinv, osinv), tag
        m = int(rng.integers(1, 41))
        R = rng.standard_normal((n, m)) * 10.0 ** rng.integers(-200, 201, m).astype(float) if rng.random() < 0.3 else rng.standard_normal((n, m))
        if rng.random() < 0.3:
            R[:, int(rng.integers(0, m))] = 0.0                            # an all-zero residual among the others
        R = np.asfortranarray(R)
        want = ox.xtv_multi(R)
        scale = np.abs(want).max(axis=0) + np.sqrt(n) * np.abs(R).max(axis=0) * 1e-3 + 1e-300
        for dg in (None, 1316, 428, 4910):
            if dg == 428 and m > 1 and rng.random() < 0.5:
                continue
            got = x.xtv(R, xtv_digits=dg)
            assert np.all(np.isfinite(got)), (tag, dg)
            assert (np.abs(got - want).max(axis=0) / scale).max() < 1e-11, (tag, m, dg)
            j = int(rng.integers(0, m))
            assert np.array_equal(x.xtv(R[:, j].copy(), xtv_digits=dg if dg else 4910), x.xtv(R, xtv_digits=dg if dg else 4910)[:, j]) or dg == 428, (tag, m, dg, j)
        kk = int(rng.integers(0, min(p, 40) + 1))
        idx = np.sort(rng.choice(p, kk, replace=False))
        val = rng.standard_normal(kk)
        mask = np.zeros(p, np.uint8); mask[idx] = 1
        coef = np.zeros(p); coef[idx] = val
        np.testing.assert_allclose(x.xv_sparse(idx, val), ox.xv_masked(mask, coef), rtol=1e-12, atol=1e-12 * (1 + np.abs(val).sum()), err_msg=str(tag))

def test_randomized_projections(mih, oracle):
    """Seeded sweep of the two projections (utilities.jl:553-559, :613-679) on their own: lengths from 1 to a few hundred thousand
    (around the 2 x 11-bit histogram passes of the device top-k; no trial aims at a buffer limit of its finish -- those are the
    cases of tests/test_gpu_select_edges.py), k from 1 to the length,
    heavy ties (values rounded to one or two digits, blocks of equal magnitudes with mixed signs), zeros, +-Inf, denormals;
    group labels dense or sparse with empty groups, J and k (scalar / vector) at random -- bit for bit against the oracle."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 515)))
    for trial in range(16):
        n = int(rng.choice([1, 2, 3, 31, 64, 1000, 2047, 2049, 65535, 65537])) if rng.random() < 0.4 else int(rng.integers(1, 300000))
        v = rng.standard_normal(n) * 10.0 ** float(rng.integers(-3, 4))
        style = int(rng.integers(0, 6))
        if style == 1:
            v = np.round(v, int(rng.integers(0, 3)))                  # many exact ties, many zeros
        elif style == 2:
            v = rng.choice([-2.5, -1.0, 0.0, 1.0, 2.5, 7.0], n)       # six distinct magnitudes
        elif style == 3:
            v[rng.random(n) < 0.01] = np.inf
            v[rng.random(n) < 0.01] = -np.inf
        elif style == 4:
            v *= 1e-310                                               # denormals
        elif style == 5:
            v[rng.random(n) < 0.7] = 0.0
        k = int(rng.choice([1, min(2, n), n, max(1, n - 1), max(1, n // 2)])) if rng.random() < 0.4 else int(rng.integers(1, n + 1))
        tag = (trial, n, style, k)
        assert np.array_equal(mih.project_k(v, k), oracle.project_k(v, k)), tag
        if n < 2:
            continue
        G = int(rng.integers(1, min(n, 3000) + 1))
        if rng.random() < 0.5:
            group = np.sort(rng.integers(1, G + 1, n))                 # contiguous blocks (some labels may not occur)
        else:
            group = rng.integers(1, G + 1, n)                          # scattered labels
        group[rng.integers(0, n)] = G                                  # the largest label occurs: the reference sizes its tables by maximum(group)
        J = int(rng.integers(1, G + 1))
        kg = rng.integers(0, 5, G) if rng.random() < 0.5 else int(rng.integers(1, 5))
        w = v.copy()
        w[~np.isfinite(w)] = 1e6                                       # (the group norms of the reference are sums of squares: keep them finite)
        got, want = mih.project_group_sparse(w, group, J, kg), oracle.project_group_sparse(w, group, J, kg)
        assert np.array_equal(got, want), tag + (G, J, np.ravel(kg)[:8].tolist(), np.flatnonzero(got != want)[:5])

def test_error_paths_nan_loglikelihood_and_bad_arguments(mih, normal_pair, normal_data):
    """fit.jl:259-260 (NaN/Inf loglikelihood aborts), fit.jl:87-94 argument errors, k > p."""
    x, _ = normal_pair
    y = normal_data["y"].copy()
    y[7] = np.nan
    with pytest.raises(mih.MendelIHTError, match="NaN|Inf"):
        mih.fit_iht(y, x, None, k=5, verbose=False)
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(normal_data["y"], x, None, k=5, tol=1e-20, verbose=False)           # tol must exceed eps
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(normal_data["y"], x, None, k=5, max_iter=-1, verbose=False)
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(normal_data["y"], x, None, k=5, est_r="MM", verbose=False)          # est_r needs NegativeBinomial
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(normal_data["y"], x, None, k=x.p + 2, verbose=False)                # cannot project to more than p + q
    with pytest.raises(mih.MendelIHTError):
        mih.fit_iht(np.abs(normal_data["y"]), x, None, k=3, d=mih.Bernoulli(), l=mih.LogitLink(), verbose=False)   # checky
    ok = mih.fit_iht(normal_data["y"], x, None, k=5, verbose=False)                     # the handle survives the failures
    assert np.count_nonzero(ok.beta) == 5

def test_float32_dense_matrix(mih, oracle):
    """`x::Matrix{Float32}` (test/L0_reg_test.jl:245-297 NegBin nuisance parameter on a Float32 matrix;
    test/cv_iht_test.jl:41-78 cross-validation on a Float32 matrix): Float32 storage on the device, Float64
    arithmetic -- identical to the oracle on the exactly-representable upcast of the same matrix."""
    rng = np.random.default_rng(23)
    n, p, k = 802, 350, 6
    X32 = rng.standard_normal((n, p)).astype(np.float32)
    X64 = X32.astype(np.float64)
    xd = mih.DenseMatrix(X32)
    assert xd.dtype == np.float32 and xd.algorithmic_bytes() < 4.2 * n * p + 8 * (n + p) + 1
    od = oracle.Mat.from_dense(X64)
    r = rng.standard_normal(n)
    assert rel(xd.xtv(r), X64.T @ r) < 1e-12
    idx = np.sort(rng.choice(p, 5, replace=False)); val = rng.standard_normal(5)
    assert rel(xd.xv_sparse(idx, val), X64[:, idx] @ val) < 1e-12
    b = np.zeros(p); b[rng.choice(p, k, replace=False)] = rng.standard_normal(k) * 0.5
    y = X64 @ b + 1 + rng.standard_normal(n)
    for kw, okw in ((dict(), dict()), (dict(init_beta=True), dict(init_beta=True)), (dict(debias=True), dict(debias=True))):
        res = mih.fit_iht(y, xd, None, k=k, verbose=False, **kw)
        o = oracle.fit_iht(od, y, None, k=k, **okw)
        assert res.iter == o["iter"] and np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"])), kw
        np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    mu = np.exp(0.3 * (X64 @ b))
    ynb = rng.negative_binomial(5, 5 / (mu + 5)).astype(float)
    res = mih.fit_iht(ynb, xd, None, k=k, d=mih.NegativeBinomial(1.0), l=mih.LogLink(), est_r="Newton", verbose=False)
    o = oracle.fit_iht(od, ynb, None, k=k, dist="negbin", link="log", nb_r=1.0, est_r="newton")
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    assert res.d.r == pytest.approx(o["nb_r"], rel=1e-4)
    folds = hash_folds(n, 3)
    mse = mih.cv_iht(y, X32, None, path=[2, 6, 10], q=3, folds=folds, verbose=False)      # a raw float32 ndarray is accepted
    omse, _ = oracle.cv_iht(od, y, None, path=[2, 6, 10], q=3, folds=folds)
    np.testing.assert_allclose(mse, omse, rtol=1e-5)
    # ragged n (not a multiple of 4): the scalar tail path of the Float32 kernel
    xr = mih.DenseMatrix(X32[:801])
    assert rel(xr.xtv(r[:801]), X64[:801].T @ r[:801]) < 1e-12

@pytest.mark.parametrize("fam", ["normal", "bernoulli", "poisson", "negbin"])
def test_simulate_and_recover(mih, fam):
    """The pattern of test/L0_reg_test.jl:1-102: simulate_random_snparray + simulate_random_response, then fit_iht with
    the true k recovers the large effects and returns exactly k non-zeros."""
    x = mih.simulate_random_snparray(3000, 4000, seed=7)
    d, l = {"normal": (mih.Normal, mih.IdentityLink), "bernoulli": (mih.Bernoulli, mih.LogitLink),
            "poisson": (mih.Poisson, mih.LogLink), "negbin": (mih.NegativeBinomial, mih.LogLink)}[fam]
    k = 10
    y, true_b, pos = mih.simulate_random_response(x, k, d, l(), seed=11)
    assert np.count_nonzero(true_b) == k and np.array_equal(np.flatnonzero(true_b), pos)
    res = mih.fit_iht(y, x, None, k=k, d=d(10.0) if fam == "negbin" else d(), l=l(), verbose=False)
    assert np.count_nonzero(res.beta) == k and res.c[0] != 0                 # L0_reg_test.jl:21-24
    big = pos[np.abs(true_b[pos]) > (0.25 if fam in ("poisson", "negbin") else 0.6)]
    assert np.isin(big, np.flatnonzero(res.beta)).mean() >= 0.7
    with pytest.raises(mih.MendelIHTError):
        mih.simulate_random_response(x, k, mih.NegativeBinomial, mih.IdentityLink())

def _mvfit_case(mih, oracle, rng, trial):
    """One random fit of test_randomized_multivariate_fits_vs_oracle (replayed by tools/repro_fuzz.py)."""
    n = int(rng.integers(150, 1500)); p = int(rng.integers(60, 400)); r = int(rng.integers(2, 6))
    q = int(rng.integers(1, 4)); k = int(rng.integers(2, 14)); miss = float(rng.choice([0.0, 0.03]))
    cols = make_bed(rng, n, p, missing_rate=miss)
    x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    Y, Z = _mv_problem(oracle, ox, rng, r, min(k, 8), q)
    kw = {}
    if q > 1 and rng.random() < 0.6:
        kw["zkeep"] = [1] + [int(v) for v in rng.integers(0, 2, q - 1)]
    if rng.random() < 0.4:
        kw["train"] = (rng.random(n) < 0.8).astype(np.uint8)
    if rng.random() < 0.3:
        kw["init_beta"] = True
    return n, p, r, q, k, miss, x, ox, Y, Z, kw

def test_randomized_multivariate_fits_vs_oracle(mih, oracle):
    """Seeded sweep of multivariate fits: traits r, covariates q (some not kept), k, missingness, train masks,
    init_beta -- against the oracle on every stable trajectory."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 31337)))
    tally = SweepTally("multivariate fits", ceiling=1, floor=9)
    for trial in range(10):
        n, p, r, q, k, miss, x, ox, Y, Z, kw = _mvfit_case(mih, oracle, rng, trial)
        o = oracle.fit_mv(ox, Y, Z, k=k, max_iter=60, **kw)
        res = mih.fit_iht(Y, x, Z, k=k, max_iter=60, verbose=False, **kw)
        tag = (trial, n, p, r, q, k, miss, sorted(kw))
        try:
            assert res.iter == o["iter"], tag
            assert np.array_equal(res.beta != 0, o["B"] != 0), tag
            np.testing.assert_allclose(res.beta, o["B"], rtol=1e-5, atol=1e-10, err_msg=str(tag))
            np.testing.assert_allclose(res.c, o["C"], rtol=1e-5, atol=1e-10, err_msg=str(tag))
            np.testing.assert_allclose(res.Σ, o["Sigma"], rtol=1e-6, err_msg=str(tag))
        except AssertionError:
            pick = lambda d, g=1.0: dict(iter=d["iter"], B=d["B"], C=d["C"] * g, Sigma=d["Sigma"])
            if any(_unstable(pick(o), pick(oracle.fit_mv(ox, Y, Z * g, k=k, max_iter=60, **kw), g), 1e-5) for g in _NUDGES):
                tally.set_aside("oracle unstable under ulp nudges", tag)
                continue
            def orc_rows(pm):                         # the same problem, its samples in another order (_rows_permuted)
                kr = dict(kw, train=kw["train"][pm]) if kw.get("train") is not None else kw
                return oracle.fit_mv(_rows_permuted(oracle, ox, pm), Y[:, pm], Z[:, pm], k=k, max_iter=60, **kr)
            rows = [orc_rows(pm) for pm in _row_orders(n)]
            if any(_unstable(pick(o), pick(v), 1e-5) for v in rows):
                tally.set_aside("oracle unstable under another order of its rows", tag)
                continue
            if res.iter == o["iter"] and np.array_equal(res.beta != 0, o["B"] != 0) and \
               _within_own_spread(o, rows, dict(B=res.beta, C=res.c, Sigma=res.Σ), dict(B=(1e-5, 1e-10), C=(1e-5, 1e-10), Sigma=(1e-6, 0.0))):
                tally.set_aside("within the tolerance plus four times the oracle's own spread under re-association", tag)
                continue
            if kw.get("init_beta"):       # a SNP that is constant over the training rows (ib_cond, iht_oracle.h; seed 10545): the univariate
                one = oracle.fit_iht(ox, Y[0], None, k=1, max_iter=1, train=kw.get("train"), init_beta=True)      # regressions of initialize_beta! see the same predictor
                if one["ib_cond"] < 1e-10:
                    tally.set_aside("init_beta: a constant predictor (rounding residue as Cholesky pivot)", tag)
                    continue
            raise
        tally.ok()
    tally.finish()

def test_gpu_against_committed_oracle_goldens(mih, normal_pair):
    """The GPU path against tests/golden/oracle_goldens.json (oracle results committed as data: the families that no
    reference fixture pins, deterministic inputs from tests/golden/make_oracle_goldens.py) -- no live oracle involved."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_oracle_goldens", os.path.join(GOLD, "make_oracle_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gold = json.load(open(os.path.join(GOLD, "oracle_goldens.json")))["goldens"]
    x, ox = normal_pair
    n, sc, y, z = mod.scenarios(ox)                     # ox only supplies the deterministic linear predictor of the inputs
    fam = {"normal": mih.Normal, "bernoulli": mih.Bernoulli, "poisson": mih.Poisson, "negbin": mih.NegativeBinomial, "gamma": mih.Gamma}
    lnk = {"identity": mih.IdentityLink, "logit": mih.LogitLink, "log": mih.LogLink, "probit": mih.ProbitLink}
    for name, (yy, kw, zz) in sc.items():
        g = gold[name]
        kw = dict(kw)
        dname = kw.pop("dist", "normal")
        d = fam[dname](kw.pop("nb_r")) if dname == "negbin" else fam[dname]()
        l = lnk[kw.pop("link", "identity")]()
        if "est_r" in kw:
            kw["est_r"] = {"newton": "Newton", "mm": "MM"}[kw["est_r"]]
        res = mih.fit_iht(yy, x, zz, d=d, l=l, verbose=False, **kw)
        tol = 1e-5 if dname == "normal" else 1e-4
        assert res.iter == g["iter"] and list(res.trace["backtracks"]) == g["backtracks"], name
        assert list(np.flatnonzero(res.beta)) == g["support"], name
        np.testing.assert_allclose(res.beta[g["support"]], g["beta"], rtol=tol, err_msg=name)
        np.testing.assert_allclose(res.c, g["c"], rtol=tol, err_msg=name)
        assert res.logl == pytest.approx(g["logl"], rel=1e-7), name
    mse = mih.cv_iht(y, x, z, path=range(1, 9), q=3, folds=hash_folds(n, 3), verbose=False)
    np.testing.assert_allclose(mse, gold["cv_normal_path1_8_q3"]["mse"], rtol=1e-5)
    bed = mih.read_bed(os.path.join(FIX, "multivariate.bed"), n)
    xm = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    Y = np.loadtxt(os.path.join(FIX, "multivariate.phen"), delimiter=",").T
    rm = mih.fit_iht(Y, xm, None, k=10, verbose=False)
    gm = gold["multivariate_k10"]
    assert rm.iter == gm["iter"] and [list(map(int, ij)) for ij in np.argwhere(rm.beta != 0)] == gm["support"]
    np.testing.assert_allclose([rm.beta[i, j] for i, j in gm["support"]], gm["B"], rtol=1e-5)
    np.testing.assert_allclose(rm.Σ, gm["Sigma"], rtol=1e-6)

def test_tiny_problems(mih, oracle):
    """Degenerate sizes: a handful of samples, a single SNP, fewer rows than one 128-row tile."""
    rng = np.random.default_rng(0)
    for n, p, k in ((3, 1, 1), (5, 2, 1), (9, 33, 2), (130, 1, 1)):
        cols = make_bed(rng, n, p, maf_lo=0.3)
        x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
        ox = oracle.Mat.from_bed_columns(cols, n)
        r = rng.standard_normal(n)
        np.testing.assert_allclose(x.xtv(r), ox.xtv(r), rtol=1e-10, atol=1e-12)
        y = rng.standard_normal(n)
        res = mih.fit_iht(y, x, None, k=k, verbose=False, max_iter=10)
        o = oracle.fit_iht(ox, y, None, k=k, max_iter=10)
        assert res.iter == o["iter"], (n, p, k)
        np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-6, atol=1e-10)
    x1 = mih.SnpLinAlg(make_bed(rng, 1, 4, maf_lo=0.3), n=1, center=True, scale=True, impute=True)
    with pytest.raises(mih.MendelIHTError, match="NaN|Inf"):             # one sample: zero deviance, NaN loglikelihood
        mih.fit_iht(np.array([0.3]), x1, None, k=1, verbose=False)

def _cv_case(mih, oracle, rng, trial, fams):
    """One random grid of test_randomized_cv_vs_oracle (also replayed by tools/repro_fuzz.py when a seed of tools/fuzz_parity.py fails)."""
    n = int(rng.integers(200, 1600)); p = int(rng.integers(60, 400)); q = int(rng.integers(2, 5))
    od, ol, D, L, tol = fams[int(rng.integers(0, 3))]
    cols = make_bed(rng, n, p, missing_rate=float(rng.choice([0.0, 0.03])))
    x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    eta = 0.5 * _sim(oracle, ox, rng, 4)
    y = {"normal": eta + 1 + rng.standard_normal(n),
         "bernoulli": (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float),
         "poisson": rng.poisson(np.exp(np.clip(0.5 * eta, -3, 3))).astype(float)}[od]
    npath = int(rng.integers(2, 14))                               # up to 13 x 4 = 52 combinations: more than 24 slots
    path = sorted(int(v) for v in rng.choice(np.arange(1, 16), npath, replace=False))
    folds = hash_folds(n, q)
    extra, roll = {}, rng.random()                                 # a third of the grids with one of the options the lock-step driver carries since round 3
    if roll < 0.12 and od == "normal":
        extra["init_beta"] = True
    elif roll < 0.24:
        extra["debias"] = True
    elif roll < 0.36:
        G = int(rng.integers(3, 9))
        group = rng.integers(1, G + 1, p)
        group[:G] = np.arange(1, G + 1)                            # every label occurs; cv_iht fixes J = 1 (cross_validation.jl:91)
        extra["group"] = np.sort(group)
    return n, p, q, od, ol, D, L, tol, x, ox, y, path, folds, extra

def test_randomized_cv_vs_oracle(mih, oracle):
    """Seeded sweep of cross-validations through the rolling lock-step driver (fused FP6 passes, slots refilled as fits
    finish; more combinations than slots in some trials, so two lanes run): losses against the oracle's sequential
    fits, and the same grid split over two ranks must add up to the single-rank result exactly."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 777)))
    fams = [("normal", "identity", mih.Normal, mih.IdentityLink, 1e-6), ("bernoulli", "logit", mih.Bernoulli, mih.LogitLink, 1e-5),
            ("poisson", "log", mih.Poisson, mih.LogLink, 1e-5)]
    tally = SweepTally("cv_iht (entries of the loss matrices)", ceiling=2, floor=125)
    for trial in range(6):
        n, p, q, od, ol, D, L, tol, x, ox, y, path, folds, extra = _cv_case(mih, oracle, rng, trial, fams)
        tag = (trial, n, p, q, od, path, sorted(extra))
        def orc(g=1.0):                                                # None: one of the reference's fits ends in an error (GLM.jl's refit inside debias!)
            try:
                return oracle.cv_iht(ox, y, np.full((n, 1), g), path=path, q=q, folds=folds, dist=od, link=ol, **extra)
            except RuntimeError:
                return None
        first = orc()
        try:
            mse, raw = mih.cv_iht(y, x, None, d=D(), l=L(), path=path, q=q, folds=folds, verbose=False, return_raw=True, **extra)
        except mih.MendelIHTError:
            mse = raw = None
        if first is None or raw is None:
            if (first is None) != (raw is None):                       # only one side failed: a real finding unless the oracle wavers itself
                kinds = {orc(g) is None for g in _NUDGES} | {first is None}
                assert len(kinds) == 2, (tag, "only one side ended in an error", first is None, raw is None)
                tally.set_aside("only one side ends in an error, the oracle wavers under nudges", tag, count=q * len(path))
            else:
                tally.ok(q * len(path))
            continue
        omse, oraw = first
        ok = np.isclose(raw, oraw, rtol=100 * tol, atol=0)
        if not ok.all():                  # entries the oracle itself does not reproduce after ulp-sized nudges of the intercept column are set aside (_unstable)
            stable = np.ones_like(ok)
            for g in _NUDGES:
                again = orc(g)
                stable &= np.isclose(again[1], oraw, rtol=100 * tol, atol=0) if again is not None else False
            if (~ok & stable).any():          # ... the same grid with its samples in another order (_rows_permuted: every sum re-associated; folds, y permuted alike)
                for pm in _row_orders(n):
                    try:
                        again = oracle.cv_iht(_rows_permuted(oracle, ox, pm), y[pm], np.ones((n, 1)), path=path, q=q, folds=folds[pm], dist=od, link=ol, **extra)
                        stable &= np.isclose(again[1], oraw, rtol=100 * tol, atol=0)
                    except RuntimeError:
                        stable[:] = False
            for f, j in np.argwhere(~ok & stable):        # ... and what the oracle REPORTS about the fit behind the entry (round 6: nothing is accepted by argument;
                try:                                      # "a step that used up max_step backtracks" was): a 0/0 step size, init_beta on a SNP that is
                    one = oracle.fit_iht(ox, y, None, k=path[j], dist=od, link=ol, max_iter=100, train=(folds != f + 1).astype(np.uint8), **extra)       # monomorphic in the fold's training rows (seed 9568), a debias! refit that halves its steps
                    flagged = one["eta_cond"] < 1e-18 or one["ib_cond"] < 1e-10 or one["db_minstep"] < 1.0 or one["bt_cond"] < _BT_TIE
                except RuntimeError as e:
                    flagged = e.db_minstep < 1.0
                if flagged:
                    stable[f, j] = False
            assert (ok | ~stable).all() and (~ok).sum() <= max(2, stable.size // 5, len(path) if extra.get("init_beta") else 0), (tag, np.argwhere(~ok & stable))      # (the ceiling counts what is set aside: entries that differ)
            tally.set_aside("entry unstable in the oracle itself", tag, count=int((~ok).sum()))
            tally.ok(int(ok.sum()))
            whole = stable.all(axis=0)                                    # model sizes with every fold stable
            np.testing.assert_allclose(mse[whole], omse[whole], rtol=100 * tol, err_msg=str(tag))
        else:
            tally.ok(ok.size)
            np.testing.assert_allclose(mse, omse, rtol=100 * tol, err_msg=str(tag))
        halves = [mih.cv_iht(y, x, None, d=D(), l=L(), path=path, q=q, folds=folds, verbose=False, return_raw=True,
                             rank=r, world=2, **extra)[1] for r in range(2)]
        assert np.array_equal(halves[0] + halves[1], raw), tag
    tally.finish()

def _mvcv_case(mih, oracle, rng, trial):
    """One random grid of test_randomized_multivariate_cv_vs_oracle (replayed by tools/repro_fuzz.py)."""
    n = int(rng.integers(200, 1200)); p = int(rng.integers(60, 300)); r = int(rng.integers(2, 5))
    qz = int(rng.integers(1, 3)); q = int(rng.integers(2, 4))
    cols = make_bed(rng, n, p, missing_rate=float(rng.choice([0.0, 0.03])))
    x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    Y, Z = _mv_problem(oracle, ox, rng, r, 6, qz)
    path = sorted(int(v) for v in rng.choice(np.arange(1, 13), int(rng.integers(2, 6)), replace=False))
    folds = hash_folds(n, q)
    extra = {}
    if qz > 1 and rng.random() < 0.5:
        extra["zkeep"] = [1] + [int(v) for v in rng.integers(0, 2, qz - 1)]
    if rng.random() < 0.25:
        extra["init_beta"] = True
    return n, p, r, qz, q, x, ox, Y, Z, path, folds, extra

def test_randomized_multivariate_cv_vs_oracle(mih, oracle):
    """Seeded sweep of multivariate cross-validations (mih_cv_mv: the lock-step batches of r-trait fits, one fused X'R pass per
    round): traits, covariates (some not kept), folds, paths, missing genotypes, init_beta -- the held-out losses against the
    oracle's sequential fits, entry by entry; entries the oracle does not reproduce itself (_unstable) are set aside."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 8086)))
    tally = SweepTally("multivariate cv (entries)", ceiling=1, floor=44)
    for trial in range(4):
        n, p, r, qz, q, x, ox, Y, Z, path, folds, extra = _mvcv_case(mih, oracle, rng, trial)
        tag = (trial, n, p, r, qz, q, path, sorted(extra))
        mse, raw = mih.cv_iht(Y, x, Z, path=path, q=q, folds=folds, verbose=False, return_raw=True, **extra)
        omse, oraw = oracle.cv_mv(ox, Y, Z, path=path, q=q, folds=folds, **extra)
        ok = np.isclose(raw, oraw, rtol=1e-5, atol=0)
        if not ok.all():
            stable = np.ones_like(ok)
            for g in _NUDGES:
                stable &= np.isclose(oracle.cv_mv(ox, Y, Z * g, path=path, q=q, folds=folds, **extra)[1], oraw, rtol=1e-5, atol=0)
            mono = np.zeros(q, dtype=bool)
            if extra.get("init_beta"):          # a SNP monomorphic in a fold's training rows (ib_cond, iht_oracle.h; seed 10137): the univariate
                for f in range(q):              # regressions of initialize_beta! (multivariate.jl:519-560) see the same constant predictor
                    one = oracle.fit_iht(ox, Y[0], None, k=1, max_iter=1, train=(folds != f + 1).astype(np.uint8), init_beta=True)
                    mono[f] = one["ib_cond"] < 1e-10
            # (seed 12023, round 5: n = 291 in two folds -- a fold of that class is set aside WHOLE, every model size of it; the ceiling
            # on entries that are merely unstable under nudges applies to the other folds, and one fold at most may be of that class)
            nudged = int((~stable[~mono]).sum())
            stable[mono, :] = False
            assert (ok | ~stable).all() and nudged <= max(2, stable.size // 5) and mono.sum() <= 1, (tag, np.argwhere(~ok & stable), mono, raw, oraw)
            tally.set_aside("entry unstable in the oracle itself", tag, count=int((~ok).sum()))
            tally.ok(int(ok.sum()))
            whole = stable.all(axis=0)
            np.testing.assert_allclose(mse[whole], omse[whole], rtol=1e-5, err_msg=str(tag))
        else:
            tally.ok(ok.size)
            np.testing.assert_allclose(mse, omse, rtol=1e-5, err_msg=str(tag))
    tally.finish()

def _path_case(mih, oracle, rng, trial, fams):
    """One random model path of test_randomized_model_paths_vs_oracle (replayed by tools/repro_fuzz.py)."""
    n = int(rng.integers(150, 1500)); p = int(rng.integers(60, 400)); q = int(rng.integers(1, 4))
    od, ol, D, L = fams[int(rng.integers(0, 4))]
    cols = make_bed(rng, n, p, missing_rate=float(rng.choice([0.0, 0.03])))
    x = mih.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    z = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    eta = 0.5 * _sim(oracle, ox, rng, 4) + z @ np.concatenate([[0.3], rng.standard_normal(q - 1) * 0.2])
    y = {"normal": eta + rng.standard_normal(n),
         "bernoulli": (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float),
         "poisson": rng.poisson(np.exp(np.clip(0.5 * eta, -3, 3))).astype(float),
         "negbin": rng.negative_binomial(4, 4 / (np.exp(0.5 + np.clip(0.5 * eta, -3, 3)) + 4)).astype(float)}[od]
    path = sorted(int(v) for v in rng.choice(np.arange(1, 13), int(rng.integers(2, 8)), replace=False))
    kw, okw = {}, {}
    roll = rng.random()
    if roll < 0.2:
        kw["debias"] = okw["debias"] = True
    elif roll < 0.4:
        G = int(rng.integers(3, 8))
        group = rng.integers(1, G + 1, p); group[:G] = np.arange(1, G + 1)
        kw["group"] = okw["group"] = np.sort(group)
    elif roll < 0.55:
        kw["weight"] = okw["weight"] = rng.uniform(0.5, 2.0, p)
    d = D(float(rng.choice([1.0, 4.0]))) if od == "negbin" else D()
    if od == "negbin":
        okw["nb_r"] = d.r
        est = rng.choice(["None", "MM", "Newton"])
        if est != "None":
            kw["est_r"], okw["est_r"] = str(est), str(est).lower()
    return n, p, q, od, ol, D, L, x, ox, y, z, path, kw, okw, d

def test_randomized_model_paths_vs_oracle(mih, oracle):
    """Seeded sweep of iht_run_many_models (cross_validation.jl:232-273; the lock-step path driver, the sequential branch for
    est_r): families, covariates, groups, prior weights, debias, NegBin est_r -- the loglikelihood of every model size against
    the oracle's fit of that size, and the path split over two ranks adds up exactly."""
    rng = np.random.default_rng(int(os.environ.get("MIH_SWEEP_SEED", 6502)))
    fams = [("normal", "identity", mih.Normal, mih.IdentityLink), ("bernoulli", "logit", mih.Bernoulli, mih.LogitLink),
            ("poisson", "log", mih.Poisson, mih.LogLink), ("negbin", "log", mih.NegativeBinomial, mih.LogLink)]
    tally = SweepTally("model paths (entries)", ceiling=1, floor=26)
    for trial in range(5):
        n, p, q, od, ol, D, L, x, ox, y, z, path, kw, okw, d = _path_case(mih, oracle, rng, trial, fams)
        tag = (trial, n, p, q, od, path, sorted(kw))
        def orc(kk, g=1.0):                            # None: the reference algorithm itself ends in an error (GLM.jl's refit failing inside debias!)
            try:
                return oracle.fit_iht(ox, y, z * g, k=kk, dist=od, link=ol, max_iter=100, **okw)
            except RuntimeError:
                return None
        try:
            ll = np.asarray(mih.iht_run_many_models(y, x, z, path=path, d=d, l=L(), verbose=False, **kw))
        except mih.MendelIHTError as e:
            # (round 6, seed 16136) the LIBRARY ended in the reference's debias! error: a finding unless the oracle does the same on the
            # original input or under a nudge for some size of the path (tests/test_oracle_illconditioned_cpu.py replays the seed)
            assert "debias" in str(e) and kw.get("debias"), (tag, str(e))
            assert any(orc(k, g) is None for k in path for g in [1.0] + _NUDGES), (tag, "only the library ended in the debias! error")
            tally.set_aside("the debias! refit's error comes and goes under ulp nudges", tag, count=len(path))
            continue
        runs = [orc(k) for k in path]
        want = np.array([o["logl"] if o is not None else np.nan for o in runs])
        tol = 1e-5 if "est_r" in kw else 1e-7
        ok = np.isclose(ll, want, rtol=tol, atol=0)
        for j in np.flatnonzero(~ok):                 # the single-fit sweeps' rules for a trajectory nobody can be held to
            o = runs[j]
            if o is None:                             # the device finished the path, the oracle's fit of this size did not: a finding unless the
                # oracle wavers itself (seed 10864: NegBin est_r with debias, r running off to 1e7 .. 6e12 -- the refit's step-halving
                # fails on the original input and not under any of the six nudges)
                assert any(orc(path[j], g) is not None for g in _NUDGES), (tag, path[j], "only the oracle ended in an error")
                tally.set_aside("only the oracle ends in an error, and wavers under nudges", (path[j],) + tag)
                continue
            # (only looked at after the comparison has failed; round 6: "a step used up max_step backtracks" is no longer among the reasons --
            # the oracle's reports, its nudges, then the same problem under other row orders)
            unstable = o["eta_cond"] < 1e-18 or o["bt_cond"] < _BT_TIE or (bool(kw.get("debias")) and o["db_minstep"] < 1.0)
            why = "the oracle's report (0/0 step size, a tie between loglikelihoods, a debias! refit that halves its steps)" if unstable else "oracle unstable under ulp nudges"
            if "est_r" in kw and o["nb_r"] > 1e6:
                # counts without overdispersion: r runs off (1e7 .. 5e10 on seed 10168, from one ulp-sized nudge to the next) and the
                # loglikelihood's lgamma(y + r) - lgamma(r) cancels n * eps * r log r ~ 1e-2 of absolute rounding error
                unstable, why = True, "NegBin r ran off: the loglikelihood is lgamma cancellation noise"
            for g in _NUDGES:
                if unstable:
                    break
                o2 = orc(path[j], g)
                unstable = o2 is None or o2["iter"] != o["iter"] or not np.isclose(o2["logl"], o["logl"], rtol=tol, atol=0)
            for pm in ([] if unstable else _row_orders(n)):
                try:
                    o2 = oracle.fit_iht(_rows_permuted(oracle, ox, pm), y[pm], z[pm], k=path[j], dist=od, link=ol, max_iter=100, **okw)
                except RuntimeError:
                    o2 = None
                if o2 is None or o2["iter"] != o["iter"] or not np.isclose(o2["logl"], o["logl"], rtol=tol, atol=0):
                    unstable, why = True, "oracle unstable under another order of its rows"
                    break
            assert unstable, (tag, path[j], ll[j], want[j])
            tally.set_aside(why, (path[j],) + tag)
        tally.ok(int(ok.sum()))
        halves = [np.asarray(mih.iht_run_many_models(y, x, z, path=path, d=d, l=L(), verbose=False, rank=r, world=2, **kw)) for r in range(2)]
        assert np.array_equal(halves[0] + halves[1], ll), tag
    tally.finish()

def test_more_ranks_than_work_items(mih):
    """Sharding with more ranks than (fold, k) combinations / path entries (8 GPUs, a 2 x 2 grid): the ranks without work return
    zeros and the parts still add up to the single-process result bit for bit -- univariate and multivariate cross-validation,
    model paths."""
    rng = np.random.default_rng(0)
    n, p = 400, 120
    x = mih.SnpLinAlg(make_bed(rng, n, p), n=n, center=True, scale=True, impute=True)
    y, Y = rng.standard_normal(n), rng.standard_normal((2, n))
    folds = hash_folds(n, 2)
    for resp, world in ((y, 8), (Y, 7)):
        full = mih.cv_iht(resp, x, None, path=[1, 2], q=2, folds=folds, verbose=False, return_raw=True)[1]
        parts = [mih.cv_iht(resp, x, None, path=[1, 2], q=2, folds=folds, verbose=False, return_raw=True, rank=r, world=world)[1] for r in range(world)]
        assert np.array_equal(sum(parts), full) and sum(np.count_nonzero(q_) == 0 for q_ in parts) == world - 4
    ll = np.asarray(mih.iht_run_many_models(y, x, None, path=[1, 3], verbose=False))
    pp = [np.asarray(mih.iht_run_many_models(y, x, None, path=[1, 3], verbose=False, rank=r, world=5)) for r in range(5)]
    assert np.array_equal(sum(pp), ll)
    with pytest.raises(mih.MendelIHTError, match="no training samples"):
        mih.cv_iht(y, x, None, path=[1], q=2, folds=np.ones(n, dtype=np.int32), verbose=False)      # every sample in fold 1: nothing to train fold 1's model on

def test_c_abi_refuses_bad_arguments_without_crashing(mih):
    """85 calls with bad arguments straight at the C ABI (tools/abi_edge_probe.py, in a child process so that a crash would be
    seen as one): NULL pointers, zero / negative / oversized dimensions, out-of-range indices, labels, folds, ranks, unknown
    codes -- every one comes back with a status and a message, two documented ones are accepted, and the library fits a model
    afterwards."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_edge_probe.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "probe finished" in r.stdout and "ACCEPTED: []" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.count(": rc=") >= 80

def test_auto_digit_mode_in_the_lockstep_drivers(mih, oracle):
    """ xtv_digits = -1: the lock-step drivers score a residual of a GLM fit in the 43-bit format when ITS
    max |r| / rms(r) <= 128 and in the 54-bit format otherwise -- per residual, so a fit's bits do not depend on its company.
    Bernoulli / Logit (every residual qualifies: |y - mu| < 1): all 40 losses within 1e-9 of the oracle, the eight shards add up
    to the single-rank matrix bit for bit; Poisson with planted count outliers: some residuals qualify and some do not, losses
    within 1e-9 of the oracle; Normal fits and single fits: the default format, bit for bit."""
    n, p = 20_000, 2_000
    x, yb, folds = _config3_problem(mih, n, p)
    ox = oracle.Mat.from_bed_columns(x.export_bed(), n)
    path = list(range(3, 11))
    kw = dict(path=path, q=5, folds=folds, verbose=False, return_raw=True, d=mih.Bernoulli(), l=mih.LogitLink())
    mih.profile_enable(x, True)
    mih.profile_counters(x, reset=True)
    mse_a, raw_a = mih.cv_iht(yb, x, None, xtv_digits=-1, **kw)
    cnt = mih.profile_counters(x, reset=True)
    mse_d, raw_d = mih.cv_iht(yb, x, None, **kw)
    cnt_d = mih.profile_counters(x, reset=True)
    mih.profile_enable(x, False)
    assert cnt["residuals_43bit"] > 200 and cnt_d["residuals_43bit"] == 0
    assert not np.array_equal(raw_a, raw_d)                               # it really is the other arithmetic ...
    np.testing.assert_allclose(raw_a, raw_d, rtol=1e-10)                  # ... to ~1e-12
    omse, oraw = oracle.cv_iht(ox, yb, None, path=path, q=5, folds=folds, dist="bernoulli", link="logit")
    np.testing.assert_allclose(raw_a, oraw, rtol=1e-9)
    np.testing.assert_allclose(mse_a, omse, rtol=1e-9)
    tot = np.zeros_like(raw_a)
    for r in range(8):
        tot += mih.cv_iht(yb, x, None, xtv_digits=-1, rank=r, world=8, **kw)[1]
    assert np.array_equal(tot, raw_a)                                     # a fit's bits do not depend on which fits it rides with
    # heavy tails: Poisson counts with planted outliers -- those fits' residuals fail the test and keep 54 bits
    rng = np.random.default_rng(8)
    supp = np.sort(rng.choice(p, 6, replace=False))
    eta = x.xv_sparse(supp, rng.standard_normal(6) * 0.3)
    yp = rng.poisson(np.exp(eta)).astype(float)
    yp[rng.choice(n, 3, replace=False)] = 4000.0
    kwp = dict(path=[2, 4, 6], q=3, folds=hash_folds(n, 3), verbose=False, return_raw=True, d=mih.Poisson(), l=mih.LogLink())
    mih.profile_enable(x, True)
    mih.profile_counters(x, reset=True)
    _, raw_p = mih.cv_iht(yp, x, None, xtv_digits=-1, **kwp)
    cntp = mih.profile_counters(x, reset=True)
    passes = mih.profile_passes(x, reset=True)
    mih.profile_enable(x, False)
    scored = sum(q["residuals"] for q in passes)
    assert 0 <= cntp["residuals_43bit"] < scored                          # (the outliers' residuals are 54-bit ones)
    _, oraw_p = oracle.cv_iht(ox, yp, None, path=[2, 4, 6], q=3, folds=hash_folds(n, 3), dist="poisson", link="log")
    np.testing.assert_allclose(raw_p, oraw_p, rtol=1e-6)
    # Normal / Identity and single fits: -1 is the default format
    yn = eta + 1.0 + rng.standard_normal(n)
    kn = dict(path=[3, 6], q=3, folds=hash_folds(n, 3), verbose=False, return_raw=True)
    assert np.array_equal(mih.cv_iht(yn, x, None, xtv_digits=-1, **kn)[1], mih.cv_iht(yn, x, None, **kn)[1])
    a = mih.fit_iht(yb, x, None, k=6, d=mih.Bernoulli(), l=mih.LogitLink(), verbose=False, xtv_digits=-1)
    b = mih.fit_iht(yb, x, None, k=6, d=mih.Bernoulli(), l=mih.LogitLink(), verbose=False)
    assert np.array_equal(a.beta, b.beta) and a.iter == b.iter
    # the multivariate fit (round 5): per pass, all r rows of T1 = Gamma * resid must pass the guard -- Gaussian traits do: every
    # pass in the 43-bit format, the oracle's support / iterations / backtracks, B to 1e-9; one trait with a planted outlier of 10^6
    # standard deviations: its passes keep 54 bits and the fit is the default fit bit for bit
    Ym, Zm = _mv_problem(oracle, ox, rng, 4, 9, 2)
    mih.profile_enable(x, True)
    mih.profile_counters(x, reset=True)
    ma = mih.fit_iht(Ym, x, Zm, k=9, verbose=False, xtv_digits=-1)
    cm = mih.profile_counters(x, reset=True)
    md = mih.fit_iht(Ym, x, Zm, k=9, verbose=False)
    om = oracle.fit_mv(ox, Ym, Zm, k=9)
    assert cm["residuals_43bit"] >= 4 * (ma.iter - 1) > 0 and mih.profile_counters(x, reset=True)["residuals_43bit"] == 0
    assert ma.iter == md.iter == om["iter"] and list(ma.trace["backtracks"]) == list(om["bt_trace"])
    assert np.array_equal(ma.beta != 0, om["B"] != 0) and not np.array_equal(ma.beta, md.beta)
    np.testing.assert_allclose(ma.beta, md.beta, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(ma.beta, om["B"], rtol=1e-5, atol=1e-12)
    Yo = Ym.copy(); Yo[2, 17] += 1e6 * Ym[2].std()
    oa = mih.fit_iht(Yo, x, Zm, k=9, verbose=False, xtv_digits=-1, max_iter=8)
    co = mih.profile_counters(x, reset=True)
    od = mih.fit_iht(Yo, x, Zm, k=9, verbose=False, max_iter=8)
    mih.profile_enable(x, False)
    assert co["residuals_43bit"] == 0 and np.array_equal(oa.beta, od.beta) and oa.iter == od.iter

# ---- BASELINE.json configs at their own sizes / trait counts ("configs_untested") -------------------------
def test_config0_normal_bed_k9_against_g1b(mih, normal_pair, normal_data):
    """configs[0]: fit_iht on data/normal.bed, k = 9, Normal, intercept only (README.md:104) on the GPU against the
    G1b numbers (an independent numpy probe of the reference algorithm; tests/test_oracle_golden.py pins the
    oracle to the same numbers)."""
    x, ox = normal_pair
    res = mih.fit_iht(normal_data["y"], x, None, k=9, verbose=False)
    assert res.iter == 10
    assert res.logl == pytest.approx(-1612.734968, abs=1e-5)
    assert list(np.flatnonzero(res.beta) + 1) == [1266, 3137, 4246, 4717, 6290, 7629, 7755, 8375, 9415]
    assert res.c[0] == pytest.approx(1.65222721, abs=1e-7)

def test_bench_workload_fewer_columns_against_oracle(mih, oracle):
    """The bench.py workload (configs[2]: n = 500 000, k = 200, Normal) with 60 000 of its 1 000 000 columns, GPU against
    the oracle on the same matrix (tools/validate_large.py as a test): same iterations and support, beta to 1e-12."""
    n, p, k = 500_000, 60_000, 200
    x = mih.SnpLinAlg.synthetic(n, p, seed=2024)
    rng = np.random.default_rng(2025)
    supp = np.sort(rng.choice(p, size=k, replace=False))
    y = x.xv_sparse(supp, rng.standard_normal(k)) + 1.0 + rng.standard_normal(n)
    res = mih.fit_iht(y, x, None, k=k, verbose=False)
    ox = oracle.Mat.from_bed_columns(x.export_bed(), n)
    o = oracle.fit_iht(ox, y, None, k=k)
    assert res.iter == o["iter"] and list(res.trace["backtracks"]) == list(o["bt_trace"])
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=0, atol=1e-12)
    assert res.logl == pytest.approx(o["logl"], rel=1e-12)

def test_c_abi_harness_reproduces_the_recorded_run(mih, tmp_path):
    """tests/abi_harness.c (plain C, dlopen, no ctypes mirrors) runs the reference's recorded fit (G1) and a small
    cross-validation through mih_snp_create / mih_fit_iht / mih_cv_iht -- the calls a Julia ccall binding makes."""
    import subprocess
    from test_abi_cpu import _build_harness
    exe = _build_harness(tmp_path)
    r = subprocess.run([str(exe), mih.library_path(), FIX], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout and "5 iterations" in r.stdout

def test_native_rccl_communicator_world1(mih, normal_pair, normal_data):
    """mih_comm_create_rccl: the library's own RCCL communicator behind the `mih_comm` of a column-sharded fit.  The test
    box has one GPU (RCCL refuses two ranks on one device), so this drives the whole native path -- dlopen of librccl,
    unique id, ncclCommInitRank, device and host all-reduce, all-gather -- with a one-rank communicator: the fit must equal
    the plain single-process fit bit for bit, and the recorded G1 log."""
    from mendeliht_amd import dist as D
    x, _ = normal_pair
    y, z = normal_data["y"], normal_data["z"]
    one = mih.fit_iht(y, x, z, k=7, verbose=False)
    sh = D.fit_iht_sharded(y, x, z, col_offset=0, p_global=x.p, native=True, k=7, verbose=False)
    assert sh.iter == one.iter == 5
    assert np.array_equal(sh.beta, one.beta) and np.array_equal(sh.c, one.c) and sh.logl == one.logl
    g = json.load(open(os.path.join(GOLD, "golden_normal_k7.json")))
    np.testing.assert_allclose(sh.trace["logl"], g["logl"], rtol=1e-11)
    # logistic with prior weights and a covariate competing in the projection: every exchange kind is exercised
    rng = np.random.default_rng(5)
    yb = (rng.random(x.n) < 0.5).astype(float)
    w = rng.uniform(0.5, 2.0, x.p)
    kw = dict(k=6, d=mih.Bernoulli(), l=mih.LogitLink(), weight=w, zkeep=[True, False], verbose=False)
    one = mih.fit_iht(yb, x, z, **kw)
    sh = D.fit_iht_sharded(yb, x, z, col_offset=0, p_global=x.p, native=True, **kw)
    assert sh.iter == one.iter and np.array_equal(sh.beta, one.beta) and sh.logl == one.logl

def test_config3_full_grid_against_oracle(mih, oracle):
    """The EXACT driver shape of BASELINE configs[3]: cv_iht Bernoulli/Logit, path = 1:20, q = 5 = 100
    (fold, k) fits on one rank -- two lock-step lanes of 19 slots (38 fits in flight: 19 ten-digit residuals fill the 192 digit columns of a six-operand pass), the tail hand-over from lane 1 to lane 0
    and the 20 fits of a fold sharing one initial score all fire (asserted from the driver's own counters) -- with ALL 100
    held-out losses against oracle.cv_iht (cross_validation.jl:98-131), and the eight `rank = r, world = 8` shards of the same
    grid summing bit-exactly to the single-rank matrix (each rank: 12 or 13 fits in one lane, as one GPU of 8 runs it)."""
    n, p = 20_000, 4_000
    x, yb, folds = _config3_problem(mih, n, p)
    path = range(1, 21)
    mih.profile_counters(x, reset=True)
    mih.profile_read(x, reset=True)
    mih.profile_enable(x, True)
    mse, raw = mih.cv_iht(yb, x, None, path=path, q=5, folds=folds, verbose=False, return_raw=True,
                          d=mih.Bernoulli(), l=mih.LogitLink())
    mih.profile_enable(x, False)
    cnt = mih.profile_counters(x, reset=True)
    passes = mih.profile_passes(x, reset=True)
    # the driver shape of the full-size run
    assert cnt["fits"] == 100 and cnt["lanes"] == 2
    assert cnt["max_lane_slots"] == 19 and cnt["max_in_flight"] == 38          # two lanes x floor(6 operands x 32 columns / 10 digits)
    assert cnt["handovers"] == 1                                                # lane 1 handed its tail to lane 0
    assert cnt["shared_init"] >= 80                                             # at most 2 lanes x 5 folds ride their own initial score
    assert cnt["scores"] >= 100 * 5 and cnt["rounds"] >= 10
    assert {q["stream_tag"] for q in passes} == {1, 2}
    assert max(q["residuals"] for q in passes) == 19 and all(q["kernel"].startswith("k_xtv_dma16<") for q in passes)
    assert all(q["operands"] == (10 * q["residuals"] + 31) // 32 for q in passes)                # flat packing of the digit columns
    assert cnt["init_scores"] == 100                                            # one initial score per fit, counted apart from the steps' 
    # (round 5) a fit that converges is finished BEFORE the pass of its last step (the convergence test needs b and b0 only; the
    # reference computes that score and never reads it): every iteration but those ends with a scored residual
    assert cnt["skipped_last_scores"] >= 90                                     # (a fit may also end on max_iter)
    assert sum(q["residuals"] for q in passes) == cnt["scores"] - cnt["skipped_last_scores"] + cnt["init_scores"] - cnt["shared_init"]
    assert sum(q["residuals"] for q in passes) / len(passes) >= 15.0            # residuals per fused pass (19 slots), ramp-up and tail included
    assert np.count_nonzero(raw) == 100
    # all 100 losses against the oracle
    ox = oracle.Mat.from_bed_columns(x.export_bed(), n)
    omse, oraw = oracle.cv_iht(ox, yb, None, path=path, q=5, folds=folds, dist="bernoulli", link="logit")
    np.testing.assert_allclose(raw, oraw, rtol=1e-4)                            # north_star: 1e-4 for GLM links
    np.testing.assert_allclose(raw, oraw, rtol=1e-9)                            # what it actually is
    np.testing.assert_allclose(mse, omse, rtol=1e-9)
    assert int(np.argmin(mse)) == int(np.argmin(omse))
    # eight shards, as 8 GPUs would run them (here one after the other on this GPU)
    rank_of = mih.cv_assignment(path, 5, 8)
    tot = np.zeros_like(raw)
    for r in range(8):
        mih.profile_enable(x, True)
        _, part = mih.cv_iht(yb, x, None, path=path, q=5, folds=folds, verbose=False, return_raw=True, rank=r, world=8,
                             d=mih.Bernoulli(), l=mih.LogitLink())
        mih.profile_enable(x, False)
        c = mih.profile_counters(x, reset=True)
        mih.profile_read(x, reset=True)
        assert np.array_equal(part != 0, rank_of == r)
        assert c["fits"] == int((rank_of == r).sum()) and c["fits"] in (12, 13) and c["lanes"] == 1
        tot += part
    assert np.array_equal(tot.view(np.uint64), raw.view(np.uint64))             # bit-exact: a fit does not depend on its rank

def test_snplinalg_float32_callers(mih, normal_data):
    """T = Float32 (src/MendelIHT.jl:39: Float = Union{Float64, Float32}): SnpLinAlg{Float32} on the 2-bit path.  The device
    arithmetic does not depend on T, so the Float32 caller gets the Float64 fit, cast: same support, same iterations, beta equal
    to the Float64 beta rounded to Float32 -- at least as accurate as an all-Float32 run."""
    n = normal_data["n"]
    bed = mih.read_bed(normal_data["bed"], n)
    y, z = normal_data["y"], normal_data["z"]
    x64 = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    x32 = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True, dtype=np.float32)
    r64 = mih.fit_iht(y, x64, z, k=7, verbose=False)
    r32 = mih.fit_iht(y.astype(np.float32).astype(np.float64), x32, z.astype(np.float32).astype(np.float64), k=7, verbose=False)
    assert r32.beta.dtype == np.float32 and r32.c.dtype == np.float32
    assert np.array_equal(np.flatnonzero(r32.beta), np.flatnonzero(r64.beta)) and r32.iter == r64.iter
    np.testing.assert_allclose(r32.beta, r64.beta, rtol=2e-5, atol=1e-7)        # y, z themselves were rounded to Float32
    with pytest.raises(mih.MendelIHTError):
        mih.SnpLinAlg(bed, n, dtype=np.float16)

@pytest.mark.parametrize("fam", ["normal", "bernoulli", "poisson"])
def test_wrapper_three_input_routes_agree(mih, tmp_path, fam):
    """test/wrapper_test.jl:44-77: `iht` / `cross_validate` on a PLINK trio give the same result whether the phenotype comes
    from the .fam file or a phenotype file and whether the intercept comes from a covariate file of ones or the default."""
    n, p = 800, 1500
    x = mih.SnpLinAlg.synthetic(n, p, seed=12)
    rng = np.random.default_rng(13)
    supp = np.sort(rng.choice(p, 6, replace=False))
    eta = x.xv_sparse(supp, rng.standard_normal(6) * 0.5)
    d = {"normal": mih.Normal, "bernoulli": mih.Bernoulli, "poisson": mih.Poisson}[fam]
    y = {"normal": eta + rng.standard_normal(n), "bernoulli": (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float),
         "poisson": rng.poisson(np.exp(0.5 * eta)).astype(float)}[fam]
    prefix = str(tmp_path / f"uni{fam}")
    with open(prefix + ".bed", "wb") as f:
        f.write(b"\x6c\x1b\x01")
        f.write(x.export_bed().tobytes())
    with open(prefix + ".bim", "w") as f:
        for j in range(p):
            f.write(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n")
    with open(prefix + ".fam", "w") as f:
        for i in range(n):
            f.write(f"{i + 1}\t1\t0\t0\t1\t{float(y[i])!r}\n")
    (tmp_path / "cov.txt").write_text("".join("1.0\n" for _ in range(n)))
    (tmp_path / "phen.txt").write_text("".join(f"{float(v)!r}\n" for v in y))
    kw = dict(verbose=False, summaryfile=str(tmp_path / "s.txt"), betafile=str(tmp_path / "b.txt"), max_iter=5)
    r1 = mih.iht(prefix, 11, d, **kw)
    r2 = mih.iht(prefix, 11, d, covariates=str(tmp_path / "cov.txt"), **kw)
    r3 = mih.iht(prefix, 11, d, covariates=str(tmp_path / "cov.txt"), phenotypes=str(tmp_path / "phen.txt"), **kw)
    for r in (r2, r3):
        assert np.array_equal(r.beta, r1.beta) and r.logl == r1.logl and r.iter == r1.iter and r.σg == r1.σg
    assert np.count_nonzero(r1.beta) == 11 and r1.c[0] != 0
    folds = hash_folds(n, 3)
    ckw = dict(verbose=False, max_iter=5, q=3, folds=folds, path=range(0, 8), cv_summaryfile=str(tmp_path / "cv.txt"))
    m1 = mih.cross_validate(prefix, d, **ckw)
    m2 = mih.cross_validate(prefix, d, covariates=str(tmp_path / "cov.txt"), **ckw)
    m3 = mih.cross_validate(prefix, d, covariates=str(tmp_path / "cov.txt"), phenotypes=str(tmp_path / "phen.txt"), **ckw)
    assert np.array_equal(m1, m2) and np.array_equal(m1, m3) and np.all(m1 > 0)           # test/cv_iht_test.jl: all(mses .> 0), path = 0:..

def test_cv_init_beta_full_grid_against_oracle(mih, oracle):
    """cv_iht(init_beta = true) -- the setting of the reference's large real runs (manuscript/UKBB_hyptertension/ukbb.jl:16-18) --
    on the LOCK-STEP driver (round 3): path = 1:20, q = 5, Normal, two lanes; the p univariate regressions of initialize_beta!
    (utilities.jl:776-812) are computed once per fold and lane and shared by the fold's fits (IbShared).  All 100 losses against
    the oracle's sequential cv_iht, and far fewer passes than 100 fits x 2 regressions."""
    n, p = 6000, 2000
    x = mih.SnpLinAlg.synthetic(n, p, seed=91)
    rng = np.random.default_rng(92)
    supp = np.sort(rng.choice(p, 9, replace=False))
    z = np.column_stack([np.ones(n), rng.standard_normal(n)])
    y = x.xv_sparse(supp, rng.standard_normal(9) * 0.5) + 0.7 + 0.3 * z[:, 1] + rng.standard_normal(n)
    folds = hash_folds(n, 5)
    mih.profile_read(x, reset=True); mih.profile_counters(x, reset=True)
    mih.profile_enable(x, True)
    mse, raw = mih.cv_iht(y, x, z, path=range(1, 21), q=5, folds=folds, init_beta=True, verbose=False, return_raw=True)
    mih.profile_enable(x, False)
    cnt = mih.profile_counters(x, reset=True)
    passes = mih.profile_passes(x, reset=True)
    assert cnt["fits"] == 100 and cnt["lanes"] == 2
    two_rhs = [q for q in passes if q["stream_tag"] == 0 and q["residuals"] == 2]       # the fused 2-RHS pass of initialize_beta!
    assert 5 <= len(two_rhs) <= 10                                                       # once per fold and lane, not once per fit
    ox = oracle.Mat.from_bed_columns(x.export_bed(), n)
    omse, oraw = oracle.cv_iht(ox, y, z, path=range(1, 21), q=5, folds=folds, init_beta=True)
    np.testing.assert_allclose(raw, oraw, rtol=1e-9)
    np.testing.assert_allclose(mse, omse, rtol=1e-9)
    logl = mih.iht_run_many_models(y, x, z, path=range(1, 9), verbose=False)            # model path on the same driver
    assert np.all(np.diff(logl) > 0)

def test_lockstep_error_paths_leave_the_library_usable(mih):
    """A fit that fails inside a lock-step round (NaN loglikelihood, fit.jl:259) fails the whole cross-validation with the
    reference's error -- from a coroutine of a lane, with the other fits of both lanes in flight -- and leaves nothing behind: the
    next call on the same matrix gives the bits of the call before (pool blocks returned, streams drained, no stuck flag)."""
    n, p = 5000, 1200
    x = mih.SnpLinAlg.synthetic(n, p, seed=21)
    rng = np.random.default_rng(22)
    supp = np.sort(rng.choice(p, 6, replace=False))
    y = x.xv_sparse(supp, rng.standard_normal(6)) + rng.standard_normal(n)
    folds = hash_folds(n, 4)
    kw = dict(path=range(1, 11), q=4, folds=folds, verbose=False, return_raw=True)
    before = mih.cv_iht(y, x, None, **kw)[1]
    bad = y.copy()
    bad[17] = np.nan
    for _ in range(3):
        with pytest.raises(mih.MendelIHTError, match="NaN"):
            mih.cv_iht(bad, x, None, **kw)
        with pytest.raises(mih.MendelIHTError, match="NaN"):
            mih.iht_run_many_models(bad, x, None, path=range(1, 9), verbose=False)
    after = mih.cv_iht(y, x, None, **kw)[1]
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))

def test_choose_callback_makes_the_references_random_draw(mih, oracle):
    """_choose! (src/utilities.jl:444-458, src/multivariate.jl:310-351): the one place on the path where the reference draws
    from the caller's RNG.  mih_fit_params::choose hands the draw to the caller (the Julia glue answers with the reference's own
    `sample` / `shuffle!`); the restatement has the same hook.  Given the same stand-in RNG the library and the restatement ask
    the same questions in the same order and return the same model; without a callback both apply the same deterministic rule
    and flag it; a bad draw is an ArgumentError."""
    from conftest import seeded_draw, tied_case
    m = mih
    cols, y, tied = tied_case()
    n = 1000
    x = m.SnpLinAlg(cols, n=n, center=True, scale=True, impute=True)
    xo = oracle.Mat.from_bed_columns(cols, n)
    z = np.ones((n, 1))
    for k in (2, 1):
        for seed in (11, 12, 13):
            lh, lo = [], []
            rh = m.fit_iht(y, x, z, k=k, verbose=False, choose=seeded_draw(seed, lh))
            ro = oracle.fit_iht(xo, y, None, k=k, choose=seeded_draw(seed, lo))
            assert lh == lo and len(lh) >= 1 and rh.choose_fired and ro["choose_fired"]
            assert sorted(np.flatnonzero(rh.beta)) == sorted(np.flatnonzero(ro["beta"]))
            assert rh.iter == ro["iter"]
            np.testing.assert_allclose(rh.beta, ro["beta"], rtol=0, atol=1e-10)
            np.testing.assert_allclose(rh.trace["logl"], ro["logl_trace"], rtol=1e-11)      # (flat after the first step: one true effect,
            # interchangeable copies -- whether a step "lowers" the loglikelihood is decided in its last bit, so the backtrack counts are not compared)
        plain_h, plain_o = m.fit_iht(y, x, z, k=k, verbose=False), oracle.fit_iht(xo, y, None, k=k)
        assert plain_h.choose_fired and sorted(np.flatnonzero(plain_h.beta)) == sorted(np.flatnonzero(plain_o["beta"]))
    supports = {tuple(np.flatnonzero(m.fit_iht(y, x, z, k=2, verbose=False, choose=seeded_draw(s, [])).beta)) for s in range(8)}
    assert len(supports) > 1                                   # the draw decides which of the interchangeable copies stay
    with pytest.raises(m.MendelIHTError):
        m.fit_iht(y, x, z, k=2, verbose=False, choose=lambda kind, lst, excess: np.array([5]))            # not in the list
    with pytest.raises(m.MendelIHTError):
        m.fit_iht(y, x, z, k=1, verbose=False, choose=lambda kind, lst, excess: lst[:1].repeat(excess))   # one SNP twice
    with pytest.raises(m.MendelIHTError):
        m.fit_iht(y, x, z, k=2, verbose=False, choose=lambda kind, lst, excess: 1 / 0)                     # the callback fails
    # Bernoulli with a second, unprotected covariate (three collinear copies in the model converge slowly: 19 steps are enough here)
    rng = np.random.default_rng(8)
    z2 = np.column_stack([np.ones(n), rng.standard_normal(n)])
    yb = (y > np.median(y)).astype(float)
    lh, lo = [], []
    rh = m.fit_iht(yb, x, z2, k=2, d=m.Bernoulli(), l=m.LogitLink(), zkeep=[1, 0], verbose=False, max_iter=20, choose=seeded_draw(21, lh))
    ro = oracle.fit_iht(xo, yb, z2, k=2, dist="bernoulli", link="logit", zkeep=[1, 0], max_iter=20, choose=seeded_draw(21, lo))
    assert lh == lo and lh and rh.iter == ro["iter"]
    np.testing.assert_allclose(rh.beta, ro["beta"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(rh.c, ro["c"], rtol=0, atol=1e-9)
    # multivariate: shuffle!(B_nz_idx), shuffle!(C_nz_idx), then the first `excess` entries go
    Y = np.vstack([y, np.random.default_rng(5).standard_normal(n)])
    for seed in (12, 14):
        lh, lo = [], []
        rh = m.fit_iht(Y, x, None, k=1, verbose=False, choose=seeded_draw(seed, lh))
        ro = oracle.fit_mv(xo, Y, None, k=1, choose=seeded_draw(seed, lo))
        assert lh == lo and len(lh) >= 1 and rh.choose_fired           # (an empty C_nz_idx is not handed over: shuffle! of it draws nothing)
        assert all(len(call[1]) > 0 for call in lh)
        np.testing.assert_allclose(rh.beta, ro["B"], rtol=0, atol=1e-10)
        assert rh.iter == ro["iter"]
    # the lock-step drivers apply the deterministic rule (their fits run on the library's own threads): equal to the restatement's
    folds = hash_folds(n, 3)
    a = m.cv_iht(y, x, z, path=[1, 2, 3], q=3, folds=folds, verbose=False)
    b, _ = oracle.cv_iht(xo, y, None, path=[1, 2, 3], q=3, folds=folds)
    np.testing.assert_allclose(a, b, rtol=1e-9)
