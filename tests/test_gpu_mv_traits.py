"""The multivariate fit and its cross-validation over the WHOLE accepted trait range, 13 <= r <= 32 (csrc/mv.hip: kMaxR = 32,
kMaxRQ = 256), on the product library.  tests/test_gpu_mv.py stops at r = 12; what the library does differently above that, and
which case here is there for it:

  launch_mv_apply (T1 = Gamma * resid, and the step size's denominator with the upper-triangular factor and the weights)
      r = 13, 14, 15, 16      the templates k_mv_apply_t<13 .. 16>, which no other test instantiates
      r = 17, 24, 31, 32      the runtime-r kernel k_mv_apply (a dynamically indexed local array), launched by no other test
  k_mv_full (vec(B) in the reference's order, 257 * 8 * r bytes of dynamic LDS)
      r = 31                  63 736 bytes, the last size below 64 KiB
      r = 32                  65 792 bytes, 256 above 64 KiB (a workgroup of the MI355X may take up to 160 KiB)
      the small matrix        p = 300: the second block holds 44 columns
  CMat, r * q entries by value
      (r, q) = (32, 8)        r * q = 256: full; (32, 9) and r = 33 are refused, and the handle fits a model afterwards
  the r-trait X'R pass of a fit (flat packing of the ten-digit format: at most 19 residuals a pass)
      r = 13 .. 17            one pass; r = 24, 31, 32: two passes of 12, 16 + 15, 16 residuals
  the multi-trait X beta kernel k_xv_snp_cached_mt, chunks of at most 12 traits
      r = 13 .. 24            two chunks; r = 31: 12 + 12 + 7, coefficient records of 32 with one padding entry; r = 32: 12 + 12 + 8
                              (tests/test_gpu_xv_paths.py holds the kernel alone to the direct path's bits at m = 16, 17, 31, 32)
      the small matrix        2 % missing genotypes: the per-trait fix-up path behind it
  init_beta for MvNormal      1 + r right-hand sides in one fused X'R call: 18 at r = 17, 33 at r = 32 (two passes of 17 + 16)
  mih_cv_mv                   per_batch = max(1, xtv_lockstep_width / r) fits per fused call; see test_cross_validation_*
  xtv_digits = -1             k_r_guard r times per pass, r flags read back: all traits take the 43-bit format or none
  DenseMatrix, DosageMatrix   xtv_dense_device with 17 residuals: k_xtv_dosage_lds<4> four times and <1> once; the f64 dense matrix
                              of 517 rows (odd: not the LDS kernel's shape) takes k_xtv_dense once per residual; their own X beta

Every check is against oracle.fit_mv / oracle.cv_mv (the f64 restatement of the reference, no device code), with the assertions
and tolerances of test_multivariate_trait_counts_of_every_product_kernel_shape: the same iteration count and backtrack trace,
bit-exact support, B and C to rtol 1e-5 / atol 1e-12, Sigma to 1e-6, the loglikelihood to 1e-9; cross-validation losses to 1e-6
as in test_config4_multivariate_r10.  No case is set aside: for every input below the oracle agrees with itself under the six
ulp-sized nudges of gpu_helpers._NUDGES (fits: not _unstable at 1e-5; losses: within 6e-16), so a disagreement is the device's.

Two matrices: the shipped 1000 x 10000 normal.bed, and a ragged 517 x 300 one with 2 % missing genotypes.  An oracle fit is
computed once per problem and shared (the plain fit, the xtv_digits = -1 fit and the fit after the refusals read the same one)."""
import numpy as np
import pytest

from conftest import hash_folds, make_bed
from gpu_helpers import _dosages, _mv_problem, standardized

pytestmark = pytest.mark.gpu

_SMALL_N, _SMALL_P = 517, 300


@pytest.fixture(scope="module")
def small_cols():
    cols = make_bed(np.random.default_rng(5170), _SMALL_N, _SMALL_P, 0.02)
    cols.flags.writeable = False
    return cols


@pytest.fixture(scope="module")
def small_pair(mih, oracle, small_cols):
    x = mih.SnpLinAlg(small_cols, _SMALL_N, center=True, scale=True, impute=True)      # (what the oracle's matrix defaults to)
    return x, oracle.Mat.from_bed_columns(small_cols, _SMALL_N)


_MEMO = {}


def _problem(oracle, ox, name, seed, r, q, zkeep=None):
    """Y, Z, k and the oracle's fit of one problem on the matrix `name`, computed once per module and left unchanged."""
    key = (name, seed, r, q, None if zkeep is None else tuple(zkeep))
    if key not in _MEMO:
        Y, Z = _mv_problem(oracle, ox, np.random.default_rng(seed), r, 2 * r, q)
        k = 2 * r + 3
        o = oracle.fit_mv(ox, Y, Z, k=k, zkeep=zkeep, max_iter=30)
        for a in (Y, Z, *[v for v in o.values() if isinstance(v, np.ndarray)]):
            a.flags.writeable = False
        _MEMO[key] = (Y, Z, k, o)
    return _MEMO[key]


def _hold(res, o, r, p, k):
    assert res.iter == o["iter"] and res.iter >= 4
    assert list(res.trace["backtracks"]) == list(o["bt_trace"])
    assert np.array_equal(res.beta != 0, o["B"] != 0)                         # bit-exact support
    np.testing.assert_allclose(res.beta, o["B"], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(res.c, o["C"], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(res.Σ, o["Sigma"], rtol=1e-6)
    assert res.logl == pytest.approx(o["logl"], rel=1e-9)
    assert res.beta.shape == (r, p) and 0 < np.count_nonzero(res.beta) <= k


_NORMAL_FITS = [(713, 13, 2, None), (714, 14, 1, None), (715, 15, 3, [1, 1, 0]), (716, 16, 2, None), (717, 17, 2, None),
                (724, 24, 3, [1, 0, 1]), (731, 31, 8, None), (732, 32, 8, None), (732, 32, 1, None)]


@pytest.mark.parametrize("seed,r,q,zkeep", _NORMAL_FITS, ids=[f"r{r}q{q}" for _, r, q, _ in _NORMAL_FITS])
def test_fit_on_the_shipped_matrix(mih, oracle, normal_pair, seed, r, q, zkeep):
    """1000 x 10000, r = 13 .. 16 (k_mv_apply_t<r>), 17 .. 32 (k_mv_apply), covariates kept and not kept; (32, 8) fills CMat and
    launches k_mv_full with 65 792 bytes of LDS, (31, 8) with 63 736."""
    x, ox = normal_pair
    Y, Z, k, o = _problem(oracle, ox, "normal", seed, r, q, zkeep)
    res = mih.fit_iht(Y, x, Z, k=k, zkeep=zkeep, verbose=False, max_iter=30)
    _hold(res, o, r, x.p, k)


@pytest.mark.parametrize("r,q", [(17, 2), (32, 8)])
def test_fit_on_a_ragged_matrix_with_missing_genotypes(mih, oracle, small_pair, r, q):
    """517 rows (a last dword of 5 rows, an odd row pair), p = 300 (k_mv_full's last block holds 44 columns), 2 % missing
    genotypes (the multi-trait X beta takes its per-trait fix-up path)."""
    x, ox = small_pair
    Y, Z, k, o = _problem(oracle, ox, "small", 900 + r, r, q)
    res = mih.fit_iht(Y, x, Z, k=k, verbose=False, max_iter=30)
    _hold(res, o, r, x.p, k)


@pytest.mark.parametrize("r,q,seed", [(17, 2, 1700), (32, 3, 3200)])
def test_init_beta_with_a_train_mask(mih, oracle, normal_pair, r, q, seed):
    """initialize_beta!(::mIHTVariable) regresses every trait on every SNP: 1 + r right-hand sides (the weights and the r masked
    traits) in one fused X'R call, 18 and 33 of them -- the latter in two passes of 17 and 16 -- over the training rows only."""
    x, ox = normal_pair
    Y, Z = _mv_problem(oracle, ox, np.random.default_rng(seed), r, 2 * r, q)
    k = 2 * r + 3
    train = (np.arange(x.n) % 4 != 1).astype(np.uint8)
    res = mih.fit_iht(Y, x, Z, k=k, init_beta=True, train=train, verbose=False, max_iter=30)
    o = oracle.fit_mv(ox, Y, Z, k=k, init_beta=True, train=train, max_iter=30)
    plain = oracle.fit_mv(ox, Y, Z, k=k, train=train, max_iter=30)
    _hold(res, o, r, x.p, k)
    assert o["logl"] != plain["logl"] and o["logl_trace"][0] != plain["logl_trace"][0]        # the start really differs


@pytest.mark.parametrize("r", [13, 24, 32])
def test_cross_validation_with_one_or_two_fits_per_round(mih, oracle, small_pair, r):
    """mih_cv_mv keeps per_batch = max(1, xtv_lockstep_width / r) fits in flight and scores them in ONE fused X'R call per round.
    For the default residual format (ten base-49 digits packed flat: 19 residuals in the six operands of a pass)
    xtv_lockstep_width is 2 * 19 = 38, so r never exceeds it; the batch falls to ONE fit from r = 20 on:

        r = 13    two fits per round, 26 residuals in two passes of 13 (test_config4_multivariate_r10: two fits, 20 in 10 + 10)
        r = 24    one fit per round, its own 24 residuals in two passes of 12
        r = 32    one fit per round, two passes of 16

    Three folds, path [r, 2 r + 3]: six fits, the two of a fold share the fold's initial score."""
    x, ox = small_pair
    Y, Z = _mv_problem(oracle, ox, np.random.default_rng(2400 + r), r, 2 * r, 2)
    path = [r, 2 * r + 3]
    folds = hash_folds(_SMALL_N, 3)
    mse, raw = mih.cv_iht(Y, x, Z, path=path, q=3, folds=folds, verbose=False, return_raw=True)
    omse, oraw = oracle.cv_mv(ox, Y, Z, path=path, q=3, folds=folds)
    assert raw.shape == (3, 2) and np.all(raw > 0)
    np.testing.assert_allclose(raw, oraw, rtol=1e-6)
    np.testing.assert_allclose(mse, omse, rtol=1e-6)


@pytest.mark.parametrize("seed,r,q", [(717, 17, 2), (732, 32, 8)])
def test_auto_digit_mode_guards_every_trait(mih, oracle, normal_pair, seed, r, q):
    """xtv_digits = -1: k_r_guard runs on each of the r rows of T1 = Gamma * resid and r flags come home; the pass takes the 43-bit
    format for all traits or for none, so the counter of 43-bit residuals moves in steps of r.  The traits are Gaussian (the largest
    of 1000 normal deviates is about 4 rms, the guard asks for 128): passes do qualify.  Against the same oracle fit as the
    default format, at the same tolerances."""
    x, ox = normal_pair
    Y, Z, k, o = _problem(oracle, ox, "normal", seed, r, q)
    mih.profile_enable(x, True)
    try:
        mih.profile_counters(x, reset=True)
        res = mih.fit_iht(Y, x, Z, k=k, verbose=False, max_iter=30, xtv_digits=-1)
        cnt = mih.profile_counters(x, reset=True)
    finally:
        mih.profile_enable(x, False)
    assert cnt["residuals_43bit"] > 0 and cnt["residuals_43bit"] % r == 0, cnt
    assert cnt["residuals_43bit"] <= r * (res.iter + 1), cnt                  # one pass for the initial score, at most one per step
    _hold(res, o, r, x.p, k)


def test_refusals_beyond_the_range_leave_the_handle_usable(mih, oracle, small_pair):
    """r = 33 and r * q = 288 are refused with the library's messages by the fit, r = 33 by the cross-validation too; the same
    handle then fits the (17, 2) problem as before."""
    x, ox = small_pair
    rng = np.random.default_rng(33)
    n = _SMALL_N
    ones = np.ones((1, n))
    with pytest.raises(mih.MendelIHTError, match=r"r=33 must be in 1\.\.32"):
        mih.fit_iht(rng.standard_normal((33, n)), x, ones, k=10, verbose=False)
    with pytest.raises(mih.MendelIHTError, match=r"r\*q = 288 exceeds 256"):
        mih.fit_iht(rng.standard_normal((32, n)), x, np.vstack([ones, rng.standard_normal((8, n))]), k=10, verbose=False)
    with pytest.raises(mih.MendelIHTError, match=r"r=33 must be in 1\.\.32"):
        mih.cv_iht(rng.standard_normal((33, n)), x, ones, path=[5], q=3, folds=hash_folds(n, 3), verbose=False)
    Y, Z, k, o = _problem(oracle, ox, "small", 917, 17, 2)
    res = mih.fit_iht(Y, x, Z, k=k, verbose=False, max_iter=30)
    _hold(res, o, 17, x.p, k)


_DENSE_SEED, _DOSAGE_SEED = 1117, 1217


def test_dense_matrix_with_17_traits(mih, oracle):
    """A 517 x 300 Matrix{Float64}: 17 residuals through xtv_dense_device (517 rows are odd, so k_xtv_dense once per residual) and
    the dense kind's X beta."""
    X = np.asfortranarray(np.random.default_rng(_DENSE_SEED).standard_normal((_SMALL_N, _SMALL_P)))
    x, ox = mih.DenseMatrix(X), oracle.Mat.from_dense(X)
    r, k = 17, 37
    Y, Z = _mv_problem(oracle, ox, np.random.default_rng(_DENSE_SEED + 1), r, 2 * r, 2)
    res = mih.fit_iht(Y, x, Z, k=k, verbose=False, max_iter=30)
    _hold(res, oracle.fit_mv(ox, Y, Z, k=k, max_iter=30), r, x.p, k)


def test_dosage_matrix_with_17_traits(mih, oracle, small_cols):
    """The small matrix's genotypes as 16-bit dosages (denominator 1, 0xFFFF where missing): 17 residuals through
    k_xtv_dosage_lds<4> four times and <1> once, X beta through k_xv_dosage.  The oracle fits the dense matrix standardized with the
    handle's own mu and 1 / sigma, as tests/test_gpu_dosage.py does."""
    n = _SMALL_N
    code = np.unpackbits(small_cols, axis=1, bitorder="little").reshape(_SMALL_P, -1, 2)[:, :n, :]
    missing = (code[:, :, 0] + 2 * code[:, :, 1] == 1).T
    num = np.where(missing, 0xFFFF, _dosages(small_cols, n).T).astype(np.uint16)
    assert 0.01 < missing.mean() < 0.03
    x = mih.DosageMatrix(num, 1)
    ox = oracle.Mat.from_dense(np.asfortranarray(standardized(num, 1, *x.mu_sigma())))
    r, k = 17, 37
    Y, Z = _mv_problem(oracle, ox, np.random.default_rng(_DOSAGE_SEED), r, 2 * r, 2)
    res = mih.fit_iht(Y, x, Z, k=k, verbose=False, max_iter=30)
    _hold(res, oracle.fit_mv(ox, Y, Z, k=k, max_iter=30), r, x.p, k)
