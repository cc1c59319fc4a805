"""The 16-bit dosage matrix (mih_dosage_*, DosageMatrix) on the GPU: X'r against exact rational arithmetic, bit-reproducible
and fused = single; every fit against the oracle on the same standardized matrix; the reference's "read BGEN and VCF" testset
(test/wrapper_test.jl:184-202) and recorded run through VCF / BGEN files; the full-size synthetic matrix."""
import json
import os
import shutil
from fractions import Fraction

import numpy as np
import pytest

from conftest import FIX, GOLD, hash_folds
from gpu_helpers import edge_matrix, exact_xtv, standardized
from test_genotype_readers_cpu import bed_codes, write_bgen, write_vcf

pytestmark = pytest.mark.gpu


def test_xtv_exact_bound_bits_and_fusion(mih):
    n, den = 997, 255
    num = edge_matrix(n, den, 1)
    x = mih.DosageMatrix(num, den)
    mu, sinv = x.mu_sigma()
    for j in range(num.shape[1]):                        # mu: the mean of the non-missing dosages, correctly rounded
        ok = num[:, j] != 0xFFFF
        want = Fraction(int(num[ok, j].astype(np.int64).sum()), int(ok.sum()) * den) if ok.any() else Fraction(0)
        assert mu[j] == float(want)
        s = np.sqrt(mu[j] * (1 - mu[j] / 2))
        assert sinv[j] == (1 / s if s > 0 else 1.0)
    X = standardized(num, den, mu, sinv)
    rng = np.random.default_rng(2)
    R = rng.standard_normal((n, 16))
    single = np.stack([x.xtv(R[:, v]) for v in range(16)], axis=1)
    for v in (0, 7):
        ex = exact_xtv(num, den, mu, sinv, R[:, v])
        bound = np.abs(X).T @ np.abs(R[:, v])
        for j in range(num.shape[1]):
            assert abs(single[j, v] - float(ex[j])) <= 1e-12 * bound[j], (j, single[j, v], float(ex[j]))
    sigma0 = [j for j in range(num.shape[1]) if not np.any(X[:, j])]
    assert len(sigma0) >= 4 and np.all(single[sigma0] == 0.0)             # monomorphic at 0 / 2, all missing
    assert np.array_equal(x.xtv(R[:, 3]), single[:, 3])                   # run to run
    for m in (2, 5, 16):
        fused = x.xtv(R[:, :m])
        assert np.array_equal(fused, single[:, :m]), m                      # fused = single, bit for bit
    assert x.algorithmic_bytes(1) == 2.0 * n * x.p + 8.0 * (n + x.p)
    assert x.algorithmic_bytes(8) == 2.0 * n * x.p + 64.0 * (n + x.p)
    idx = np.array([0, 5, 12, 19]); val = rng.standard_normal(4)
    np.testing.assert_allclose(x.xv_sparse(idx, val), X[:, idx] @ val, rtol=1e-13, atol=1e-13)


def test_create_refusals(mih):
    with pytest.raises(mih.MendelIHTError):
        mih.DosageMatrix(np.full((10, 2), 11, np.uint16), 5)              # num > 2 denom
    with pytest.raises(mih.MendelIHTError):
        mih.DosageMatrix(np.zeros((10, 2), np.uint16), 40000)
    with pytest.raises(mih.MendelIHTError):
        mih.SnpLinAlg.mu_sigma(mih.DenseMatrix(np.ones((4, 3))))           # dense handles have no statistics


@pytest.fixture(scope="module")
def frac_pair(mih, oracle):
    rng = np.random.default_rng(7)
    n, p, den = 600, 900, 255
    rho = rng.uniform(0, 0.5, p)
    num = (rng.binomial(2, rho, (n, p)) * den + rng.integers(-25, 26, (n, p))).clip(0, 2 * den)
    num[rng.random((n, p)) < 0.01] = 0xFFFF
    num = num.astype(np.uint16)
    x = mih.DosageMatrix(num, den)
    X = standardized(num, den, *x.mu_sigma())
    return x, oracle.Mat.from_dense(np.asfortranarray(X)), X


def test_fits_match_oracle_on_fractional_dosages(mih, oracle, frac_pair):
    x, ox, X = frac_pair
    n, p = X.shape
    rng = np.random.default_rng(8)
    b = np.zeros(p); b[rng.choice(p, 6, replace=False)] = rng.standard_normal(6) * 0.6
    eta = X @ b
    cases = [(eta + 0.5 + rng.standard_normal(n), {}, {}, 1e-5),
             ((rng.random(n) < 1 / (1 + np.exp(-eta))).astype(float), dict(d=mih.Bernoulli(), l=mih.LogitLink()),
              dict(dist="bernoulli", link="logit"), 1e-4),
             (rng.poisson(np.exp(0.3 * eta)).astype(float), dict(d=mih.Poisson(), l=mih.LogLink()), dict(dist="poisson", link="log"), 1e-4)]
    for y, kw, okw, tol in cases:
        res = mih.fit_iht(y, x, None, k=6, verbose=False, **kw)
        o = oracle.fit_iht(ox, y, None, k=6, **okw)
        assert res.iter == o["iter"]
        assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
        np.testing.assert_allclose(res.beta, o["beta"], rtol=tol, atol=1e-12)
    y = cases[0][0]
    for extra in (dict(init_beta=True), dict(debias=True)):
        res = mih.fit_iht(y, x, None, k=6, verbose=False, **extra)
        o = oracle.fit_iht(ox, y, None, k=6, **extra)
        assert res.iter == o["iter"] and np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
        np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    folds = hash_folds(n, 3)
    mse = mih.cv_iht(y, x, None, path=list(range(1, 8)), q=3, folds=folds, verbose=False)
    omse, _ = oracle.cv_iht(ox, y, None, path=list(range(1, 8)), q=3, folds=folds)
    np.testing.assert_allclose(mse, omse, rtol=1e-5)
    Y = np.stack([eta + rng.standard_normal(n), 0.5 * eta + rng.standard_normal(n)])
    res = mih.fit_iht(Y, x, None, k=6, verbose=False)
    o = oracle.fit_mv(ox, Y, None, k=6)
    assert res.iter == o["iter"] and np.array_equal(res.beta != 0, o["B"] != 0)
    np.testing.assert_allclose(res.beta, o["B"], rtol=1e-5, atol=1e-12)


@pytest.fixture(scope="module")
def normal_files(tmp_path_factory):
    """data/normal as a PLINK trio, a GT VCF and an 8-bit BGEN with hard calls, all 10 000 variants (written from normal.bed)."""
    d = tmp_path_factory.mktemp("normal")
    n = 1000
    codes = bed_codes(os.path.join(FIX, "normal.bed"), n)                   # n x p ALT allele counts, -1 missing
    shutil.copyfile(os.path.join(FIX, "normal.bed"), d / "normal.bed")
    y = np.loadtxt(os.path.join(FIX, "normal_y_fam6.txt"))
    with open(d / "normal.fam", "w") as f:
        for i, v in enumerate(y):
            f.write(f"{i + 1}\t{i + 1}\t0\t0\t1\t{float(v)!r}\n")
    with open(d / "normal.bim", "w") as f:
        for j in range(codes.shape[1]):
            f.write(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n")
    np.savetxt(d / "phenotypes.txt", y)
    write_vcf(d / "normal.vcf.gz", codes, 1)
    write_bgen(d / "normal.bgen", codes, 1, nbits=8)
    return d


def test_read_bgen_and_vcf_testset(mih, normal_files):
    """test/wrapper_test.jl:184-202: PLINK, VCF and BGEN inputs give the same fit."""
    d = normal_files
    kw = dict(phenotypes=str(d / "phenotypes.txt"), summaryfile=str(d / "s.txt"))
    ref = mih.iht(str(d / "normal"), 10, mih.Normal, betafile=str(d / "b0.txt"), **kw)
    for src in ("normal.vcf.gz", "normal.bgen"):
        res = mih.iht(str(d / src), 10, mih.Normal, betafile=str(d / "b1.txt"), **kw)
        assert res.iter == ref.iter
        assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(ref.beta))
        np.testing.assert_allclose(res.beta, ref.beta, rtol=1e-10, atol=1e-14)
        assert res.logl == pytest.approx(ref.logl, rel=1e-10)
        assert res.σg == pytest.approx(ref.σg, rel=1e-10)
        rows = open(d / "b1.txt").read().splitlines()
        assert rows[0] == "chr\tpos\tSNPid\tref\talt\tEstimated_beta" and len(rows) == 10_001
    x = mih.parse_genotypes(str(d / "normal.vcf.gz"))[0]
    assert isinstance(x, mih.DosageMatrix) and x.denom == 1
    with pytest.raises(mih.MendelIHTError):
        mih.iht(str(d / "normal.vcf.gz"), 10, mih.Normal, phenotypes=6, summaryfile=str(d / "s.txt"))
    mse = mih.cross_validate(str(d / "normal.bgen"), mih.Normal, path=range(8, 12), q=3, phenotypes=str(d / "phenotypes.txt"),
                             cv_summaryfile=str(d / "cv.txt"), folds=hash_folds(1000, 3), verbose=False)
    assert np.all(np.isfinite(mse)) and len(mse) == 4


def test_golden_k7_through_vcf(mih, normal_files):
    """The reference's recorded run (docs/src/man/examples.md:230-267) reproduced from a VCF input."""
    d = normal_files
    g = json.load(open(os.path.join(GOLD, "golden_normal_k7.json")))
    res = mih.iht(str(d / "normal.vcf.gz"), 7, mih.Normal, phenotypes=str(d / "phenotypes.txt"),
                  covariates=os.path.join(FIX, "covariates.txt"), summaryfile=str(d / "s.txt"), betafile=str(d / "b.txt"))
    assert res.iter == g["iterations"]
    assert list(np.flatnonzero(res.beta) + 1) == g["positions_1based"]
    np.testing.assert_allclose(res.trace["logl"], g["logl"], rtol=1e-9)


def test_golden_excerpts_on_device(mih):
    """The committed excerpts of data/normal.{vcf.gz,bgen} on the device equal normal.bed's first 200 columns."""
    codes = bed_codes(os.path.join(FIX, "normal.bed"), 1000)[:, :200]
    for path in ("normal_head.vcf.gz", "normal_head.bgen"):
        x, ids = mih.parse_genotypes(os.path.join(GOLD, path))[:2]
        assert x.denom == 1 and x.shape == (1000, 200) and len(ids) == 1000
        assert np.array_equal(x.export().astype(np.int64), np.where(codes < 0, 0xFFFF, codes))


def test_fullsize_synthetic(mih):
    """500 000 x 100 000 (a 100 GB image; 400 GB as Float64): exported columns against the oracle's dense X'r."""
    n, p = 500_000, 100_000
    x = mih.DosageMatrix.synthetic(n, p, seed=11, denom=255, missing_rate=0.01)
    mu, sinv = x.mu_sigma()
    r = np.random.default_rng(3).standard_normal(n)
    out = x.xtv(r)
    cols = np.array([0, 1, 4097, 55_555, p - 1])
    for j in cols:
        num = x.export(int(j), 1)
        assert num.shape == (n, 1)
        ok = num[:, 0] != 0xFFFF
        assert ok.mean() == pytest.approx(0.99, abs=0.002)
        assert num[ok, 0].max() <= 510
        xj = standardized(num, 255, mu[j:j + 1], sinv[j:j + 1])[:, 0]
        assert mu[j] == pytest.approx(num[ok, 0].astype(np.float64).mean() / 255, rel=1e-14)
        assert abs(out[j] - xj @ r) <= 1e-11 * (np.abs(xj) @ np.abs(r))
    again = mih.DosageMatrix.synthetic(1000, 3, seed=11, denom=255, missing_rate=0.01)
    assert np.array_equal(again.export(), mih.DosageMatrix.synthetic(1000, 3, seed=11, denom=255, missing_rate=0.01).export())
