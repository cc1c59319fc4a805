"""The arithmetic kernels of the 16-bit dosage matrix at the shapes where they can break: X'r (k_xtv_dosage_lds, every NRHS
instantiation, one step and many, ragged tails, pad rows) against exact rational arithmetic within an error bound counted from
the kernel's source; X beta (k_xv_dosage) likewise; init_beta, debias, cross-validation and multivariate fits on a matrix
with pad rows and numerators up to 65534 against the oracle; the strided upload, regrid and the range check of the storage.

Nothing here is chaotic: every X'r / X beta check is one kernel call against an exact value, so no case is set aside."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from conftest import hash_folds
from gpu_helpers import (dosage_host_stats, dosage_xtv_tol, dosage_xv_tol, edge_matrix, exact_xtv, exact_xv, standardized)

pytestmark = pytest.mark.gpu

# Row counts around everything the kernel steps by: a 16-byte load is 8 rows, a wave-load 512, a step 1024; the staging of
# residual pairs needs `i + 1 < n` on odd n.
NS = (1, 2, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 4100, 9001)
PS = (1, 2, 15, 16, 17, 33)                         # around the 16-column block and the 2-column wave
DENS = (1, 2, 255, 10000, 32767)
# edge_matrix's columns by class: near 0, near 2, monomorphic at 0 / 1 / 2, all missing, sparse missing -- then the rest
SPECIAL = (0, 1, 6, 7, 8, 9, 10)
REST = (2, 3, 4, 5, 11, 12, 13, 14, 15, 16, 17, 18, 19)


def cases():
    """The covering set of (n, p, denom, rot): two cases per row count, case A with p = PS[i % 6], denom = DENS[i % 5] and case B
    with p = PS[(i + 3) % 6], denom = DENS[(i + 2) % 5] for the i-th row count, so every n meets two denominators and two column
    counts; the one-step row counts (i < 10) and the many-step ones (i >= 10) each run through all six p; every denominator
    meets one-step and many-step row counts.  Every case calls X'r with 9 residuals (4 + 4 + 1) and with 7 (4 + 2 + 1), so every
    n meets NRHS = 4, 2 and 1.  rot rotates which special column comes first (column_order): in the k-th case with p = 1, 17 or 33
    it is chosen so that the last column, the odd one whose wave-mate is idle, is special column k mod 7."""
    out, k = [], 0
    for i, n in enumerate(NS):
        for p, den in ((PS[i % 6], DENS[i % 5]), (PS[(i + 3) % 6], DENS[(i + 2) % 5])):
            rot = (i + den) % 7
            if p in (1, 17, 33):
                rot, k = (k - 3 * (p // 16)) % 7, k + 1
            out.append((n, p, den, rot))
    return out


def column_order(p, rot):
    """Which edge_matrix column sits at each of the p positions: L = the special columns rotated by rot, then the rest; block b
    (16 columns) holds L[3 b], L[3 b + 1], ... cyclically.  So a full block holds all seven special columns, the ragged last block
    of p = 15 does too, and the last column of p = 1, 17, 33 -- the odd one whose wave-mate is idle -- is the special column
    L[0], L[3], L[6]: over the rotations of the covering set every class gets there (test_covering_set checks it)."""
    L = [SPECIAL[(k + rot) % 7] for k in range(7)] + list(REST)
    return [L[(k % 16 + 3 * (k // 16)) % 20] for k in range(p)]


def shape_matrix(n, p, den, rot, seed):
    num = edge_matrix(n, den, seed)
    if n >= 4:                                           # the top numerator 2 den next to the missing marker, in both halves of
        num[0:4, 10] = (0xFFFF, 2 * den, 2 * den, 0xFFFF)  # a 32-bit word (at den = 32767: 0xFFFE beside 0xFFFF)
    return np.ascontiguousarray(num[:, column_order(p, rot)])


def residuals(n, m, seed):
    """Column v: standard normal (v % 3 == 0); normal times 10^U{-8..8} per row (1); |normal| + 1, no cancellation in sum r, the
    worst case for the rounding of the mean (2)."""
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((n, m))
    for v in range(m):
        if v % 3 == 1:
            R[:, v] *= 10.0 ** rng.integers(-8, 9, n)
        elif v % 3 == 2:
            R[:, v] = np.abs(R[:, v]) + 1.0
    return R


def check_stats(num, den, mu, sinv):
    """mu_j the correctly rounded exact mean of the non-missing dosages, sinv_j = 1 / sqrt(mu (1 - mu / 2)) (1 where that is 0)."""
    for j in range(num.shape[1]):
        ok = num[:, j] != 0xFFFF
        want = Fraction(int(num[ok, j].astype(np.int64).sum()), int(ok.sum()) * den) if ok.any() else Fraction(0)
        assert mu[j] == float(want), (j, mu[j], float(want))
        s = np.sqrt(mu[j] * (1 - mu[j] / 2))
        assert sinv[j] == (1 / s if s > 0 else 1.0), j


def check_exact(got, num, den, mu, sinv, R, tag):
    """Every entry of got (p x m) against the exact value within dosage_xtv_tol; exactly 0 where the bound is 0.  Returns the
    largest error in units of the bound."""
    tol = dosage_xtv_tol(num, den, R)
    worst = 0.0
    assert np.all(np.isfinite(got)), tag
    for v in range(R.shape[1]):
        ex = exact_xtv(num, den, mu, sinv, R[:, v])
        for j in range(num.shape[1]):
            err = abs(Fraction(float(got[j, v])) - ex[j])
            if tol[j, v] == 0.0:
                assert got[j, v] == 0.0 and ex[j] == 0, (tag, j, v, got[j, v])
            else:
                assert err <= Fraction(float(tol[j, v])), (tag, "column", j, "residual", v, float(got[j, v]), float(ex[j]),
                                                            float(err) / tol[j, v])
                worst = max(worst, float(err) / tol[j, v])
    return worst


def test_covering_set():
    cs = cases()
    for i, n in enumerate(NS):
        mine = [c for c in cs if c[0] == n]
        assert len({c[2] for c in mine}) >= 2 and len({c[1] for c in mine}) >= 2
    for p in PS:
        assert any(c[1] == p and c[0] <= 1024 for c in cs) and any(c[1] == p and c[0] > 1024 for c in cs)
    for den in DENS:
        assert any(c[2] == den and c[0] <= 1024 for c in cs) and any(c[2] == den and c[0] > 1024 for c in cs)
    idle_mate = {column_order(p, rot)[-1] for _, p, _, rot in cs if p % 2}
    assert set(SPECIAL) <= idle_mate, idle_mate           # every class once as the odd column whose wave-mate is idle
    for rot in range(7):
        assert set(SPECIAL) <= set(column_order(16, rot)) and set(SPECIAL) <= set(column_order(15, rot))
    ragged = {c for _, p, _, rot in cs if p > 16 for c in column_order(p, rot)[16 * ((p - 1) // 16):]}
    assert set(SPECIAL) <= ragged | {c for rot in range(7) for c in column_order(15, rot)}


@pytest.mark.parametrize("n,p,den,rot", cases())
def test_xtv_shapes(mih, n, p, den, rot):
    """X'r at the covering set of cases(): exact within the counted bound for 9 residuals of three kinds, the statistics, exact
    zeros, fused = single and run to run bit for bit, every split of launch_dosage_lds around n = 1024 and 2048, and column
    independence: the bits of a column's result depend neither on p nor on where the column sits.  At p = 1 and 2 the special
    columns alone may all be zero columns, which any sum gets right: the case runs a second time on ordinary fractional columns."""
    num = shape_matrix(n, p, den, rot, seed=100 + n)
    if den == 32767:                                                      # (every such case has n >= 4 and the sparse-missing column)
        w = num[:, column_order(p, rot).index(10)]
        assert (w[0], w[1]) == (0xFFFF, 0xFFFE) and (w[2], w[3]) == (0xFFFE, 0xFFFF)
    xtv_case(mih, num, den)
    if p <= 2:
        xtv_case(mih, np.ascontiguousarray(edge_matrix(n, den, 150 + n)[:, [11 + rot, 12 + rot][:p]]), den)


def xtv_case(mih, num, den):
    n, p = num.shape
    x = mih.DosageMatrix(num, den)
    assert np.array_equal(x.export(), num)
    mu, sinv = x.mu_sigma()
    check_stats(num, den, mu, sinv)
    _, _, hmu, hsinv = dosage_host_stats(num, den)
    assert np.array_equal(mu, hmu) and np.array_equal(sinv, hsinv)       # the host restatement the tolerance is computed from
    R = residuals(n, 9, seed=200 + n)
    got = x.xtv(R)
    worst = check_exact(got, num, den, mu, sinv, R, (n, p, den))
    print(f"n={n} p={p} denom={den}: largest error {worst:.3f} of the bound")
    X = standardized(num, den, mu, sinv)
    zero = [j for j in range(p) if not np.any(X[:, j])]
    assert np.all(got[zero] == 0.0)                                       # monomorphic, all missing
    single = np.stack([x.xtv(R[:, v]) for v in range(9)], axis=1)
    assert np.array_equal(got, single)                                    # fused (4 + 4 + 1) = single, bit for bit
    assert np.array_equal(x.xtv(R), got) and np.array_equal(x.xtv(R[:, 4]), single[:, 4])          # run to run
    splits = (7, 2, 3, 5, 6) if 1023 <= n <= 1025 or 2047 <= n <= 2049 else (7,)
    for m in splits:                                                      # 4+2+1, 2, 2+1, 4+1, 4+2: every NRHS at every offset
        assert np.array_equal(x.xtv(R[:, :m]), single[:, :m]), m
        assert np.array_equal(x.xtv(R[:, 9 - m:]), single[:, 9 - m:]), m
    # column independence: reversed (every column in another block / wave / slot when p > 1), and one column dropped so that
    # every later column changes block, wave and wave-mate
    rev = mih.DosageMatrix(np.ascontiguousarray(num[:, ::-1]), den)
    assert np.array_equal(rev.xtv(R)[::-1], got)
    assert np.array_equal(rev.xtv(R[:, :7])[::-1], got[:, :7])
    if p > 1:
        for drop in (0, p // 2):
            keep = [j for j in range(p) if j != drop]
            sub = mih.DosageMatrix(np.ascontiguousarray(num[:, keep]), den)
            assert np.array_equal(sub.xtv(R), got[keep]), drop


@pytest.mark.parametrize("n,den", [(9, 255), (1025, 32767), (2049, 10000), (9001, 2)])
def test_xtv_scaling_and_nonfinite(mih, n, den):
    """Two properties of the f64 FMA design: a residual scaled by a power of two scales the result bit for bit (no overflow, no
    subnormals at these sizes); a residual with one inf or nan row gives a non-finite value in exactly the columns where numpy's
    plain standardized(...).T r does (a stored missing entry is 0, and 0 * nan is nan there too), and nothing sticks: the next
    call with a finite residual gives the bits it gave before."""
    p = 17
    num = shape_matrix(n, p, den, 2, seed=300 + n)
    x = mih.DosageMatrix(num, den)
    X = standardized(num, den, *x.mu_sigma())
    rng = np.random.default_rng(301 + n)
    R = rng.standard_normal((n, 4))
    base = x.xtv(R)
    for k in (-200, 200):
        assert np.array_equal(x.xtv(R * 2.0 ** k), base * 2.0 ** k), k
        assert np.array_equal(x.xtv(R[:, 0] * 2.0 ** k), base[:, 0] * 2.0 ** k), k
    for bad in (np.inf, -np.inf, np.nan):
        for row in (0, n // 2, n - 1):
            Rb = R.copy()
            Rb[row, 1] = bad
            with np.errstate(invalid="ignore", over="ignore"):
                want = (X * Rb[:, 1][:, None]).sum(axis=0)                # X' r, every product formed
            got = x.xtv(Rb)
            assert np.array_equal(np.isfinite(got[:, 1]), np.isfinite(want)), (bad, row)
            assert np.array_equal(np.isnan(got[:, 1]), np.isnan(want)), (bad, row)
            assert np.array_equal(got[:, [0, 2, 3]], base[:, [0, 2, 3]])  # the other residuals of the fused pass are untouched
            one = x.xtv(Rb[:, 1])
            assert np.array_equal(np.isfinite(one), np.isfinite(want)) and np.array_equal(np.isnan(one), np.isnan(want))
            assert np.array_equal(x.xtv(R), base) and np.array_equal(x.xtv(R[:, 1]), base[:, 1])


def test_xtv_tall_fused(mih):
    """The fused instantiations over many steps: n = 100 003 (98 steps, the last one ragged), p = 17, denom = 32767, 4 residuals
    in one NRHS = 4 pass, 2 in one NRHS = 2 pass, all 17 columns exact within the counted bound."""
    n, p, den = 100_003, 17, 32767
    num = shape_matrix(n, p, den, 3, seed=400)
    x = mih.DosageMatrix(num, den)
    mu, sinv = x.mu_sigma()
    check_stats(num, den, mu, sinv)
    R = residuals(n, 4, seed=401)
    got = x.xtv(R)
    worst = check_exact(got, num, den, mu, sinv, R, "tall")
    print(f"n={n}: largest error {worst:.3f} of the bound")
    single = np.stack([x.xtv(R[:, v]) for v in range(4)], axis=1)
    assert np.array_equal(got, single)
    assert np.array_equal(x.xtv(R[:, 1:3]), single[:, 1:3]) and np.array_equal(x.xtv(R[:, :3]), single[:, :3])
    assert np.array_equal(x.xtv(R), got)


@pytest.mark.parametrize("n", [9, 1027])
def test_xv_sparse_exact(mih, n):
    """X beta on a dosage handle against the exact rational X[:, idx] val within dosage_xv_tol.  The launcher splits the support
    into G = min(nnz, 16) groups (XvWork::groups = kXvGroups = 16) of ceil(nnz / G) columns: counts on both sides of 16, and 17
    (two columns per group: the last seven groups get none), 63 / 64 / 65, 300; unsorted indices with repeats."""
    den, p = 32767, 33
    num = shape_matrix(n, p, den, 1, seed=500 + n)
    x = mih.DosageMatrix(num, den)
    mu, sinv = x.mu_sigma()
    rng = np.random.default_rng(501 + n)
    for nnz in (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300):
        idx = rng.integers(0, p, nnz)
        if nnz >= 2:
            idx[-1] = idx[0]                                              # a repeated index for certain
        val = rng.standard_normal(nnz) * 10.0 ** rng.integers(-3, 4, nnz)
        got = x.xv_sparse(idx, val)
        if nnz == 0:
            assert got.shape == (n,) and np.all(got == 0.0)
            continue
        ex = exact_xv(num, den, mu, sinv, idx, val)
        tol = dosage_xv_tol(num, den, idx, val)
        assert np.all(np.isfinite(got))
        worst = 0.0
        for i in range(n):
            err = abs(Fraction(float(got[i])) - ex[i])
            if tol[i] == 0.0:
                assert got[i] == 0.0 and ex[i] == 0, (nnz, i)
            else:
                assert err <= Fraction(float(tol[i])), (nnz, i, float(got[i]), float(ex[i]), float(err) / tol[i])
                worst = max(worst, float(err) / tol[i])
        print(f"n={n} nnz={nnz}: largest error {worst:.3f} of the bound")
        assert np.array_equal(x.xv_sparse(idx, val), got)


@pytest.fixture(scope="module")
def wide_pair(mih, oracle):
    """n = 1027 (five pad rows; ragged against every block size), p = 333, denom = 32767: numerators over the whole 16-bit range,
    1 % missing, one all-missing and one monomorphic-at-2 column."""
    rng = np.random.default_rng(17)
    n, p, den = 1027, 333, 32767
    rho = rng.uniform(0.05, 0.5, p)
    num = (rng.binomial(2, rho, (n, p)) * den + rng.integers(-den // 2, den // 2 + 1, (n, p))).clip(0, 2 * den)
    num[rng.random((n, p)) < 0.01] = 0xFFFF
    num[:, 100] = 0xFFFF
    num[:, 200] = 2 * den
    num[n - 1, p - 1] = 2 * den                                           # the top numerator in the last real row
    num = num.astype(np.uint16)
    assert num[num != 0xFFFF].max() == 65534 and num.min() == 0
    x = mih.DosageMatrix(num, den)
    X = standardized(num, den, *x.mu_sigma())
    return x, oracle.Mat.from_dense(np.asfortranarray(X)), X


def planted(X, seed):
    rng = np.random.default_rng(seed)
    n, p = X.shape
    b = np.zeros(p)
    b[rng.choice(np.setdiff1d(np.arange(p), [100, 200]), 6, replace=False)] = rng.choice([-1.0, 1.0], 6) * rng.uniform(0.4, 0.8, 6)
    eta = X @ b
    return eta, eta + 0.5 + rng.standard_normal(n), rng


def test_fits_on_pad_rows_and_large_numerators(mih, oracle, wide_pair):
    """fit_iht, init_beta, debias, cv_iht and a multivariate fit on wide_pair against the oracle on the standardized dense matrix,
    with the asserts of test_fits_match_oracle_on_fractional_dosages: same iterations, same support, rtol = 1e-5."""
    x, ox, X = wide_pair
    n, p = X.shape
    eta, y, rng = planted(X, 18)
    for extra in ({}, dict(init_beta=True), dict(debias=True)):
        res = mih.fit_iht(y, x, None, k=6, verbose=False, **extra)
        o = oracle.fit_iht(ox, y, None, k=6, **extra)
        assert res.iter == o["iter"] and np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"])), extra
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


def test_cv_init_beta_on_ragged_folds(mih, oracle, wide_pair):
    """cv_iht(init_beta = true) on wide_pair: k_ib_dosage_sxx weights every row by the fold's training mask, and with n = 1027 the
    folds are ragged against every block size.  Against the oracle's cv_iht as test_cv_init_beta_full_grid_against_oracle holds
    the 2-bit matrix to it: every fold's loss and the mean, rtol = 1e-9."""
    x, ox, X = wide_pair
    n = X.shape[0]
    _, y, _ = planted(X, 18)
    folds = hash_folds(n, 3)
    mse, raw = mih.cv_iht(y, x, None, path=range(1, 8), q=3, folds=folds, init_beta=True, verbose=False, return_raw=True)
    omse, oraw = oracle.cv_iht(ox, y, None, path=range(1, 8), q=3, folds=folds, init_beta=True)
    print("cv init_beta: largest relative difference", float(np.max(np.abs(np.asarray(raw) - oraw) / np.abs(oraw))))
    np.testing.assert_allclose(raw, oraw, rtol=1e-9)
    np.testing.assert_allclose(mse, omse, rtol=1e-9)
    plain = mih.cv_iht(y, x, None, path=range(1, 8), q=3, folds=folds, verbose=False)
    assert not np.array_equal(plain, mse)                                 # init_beta did change the fits


def _create_strided(mih, buf, n, p, stride, den):
    h = C.c_void_p(None)
    rc = mih.lib().mih_dosage_create(buf.ctypes.data_as(C.c_void_p), n, p, stride, den, 0, C.byref(h))
    return rc, h


def test_strided_upload(mih):
    """mih_dosage_create with col_stride = n + 5 and junk in the gap (0xFFFF, values above 2 denom): the handle holds the n x p
    block, its statistics and X'r are those of the contiguous upload, the junk does not trip the range check; col_stride < n is
    MIH_BAD_DIM."""
    n, p, den = 1027, 17, 255
    num = shape_matrix(n, p, den, 0, seed=600)
    buf = np.empty((p, n + 5), np.uint16)
    buf[:, :n] = num.T
    buf[:, n:] = np.array([0xFFFF, 2 * den + 1, 0xFFFE, 40000, 0xFFFF], np.uint16)[None, :]
    rc, h = _create_strided(mih, buf, n, p, n + 5, den)
    assert rc == 0
    xs = mih.DosageMatrix(None, den, _handle=h)
    xc = mih.DosageMatrix(num, den)
    assert xs.shape == (n, p) and np.array_equal(xs.export(), num)
    for a, b in zip(xs.mu_sigma(), xc.mu_sigma()):
        assert np.array_equal(a, b)
    R = residuals(n, 7, seed=601)
    assert np.array_equal(xs.xtv(R), xc.xtv(R))
    rc, h = _create_strided(mih, buf, n, p, n - 1, den)
    assert rc == 1 and not h.value                                        # MIH_BAD_DIM
    with pytest.raises(mih.MendelIHTError):                               # the junk IS out of range where it is part of the matrix
        rc, h = _create_strided(mih, buf, n + 2, p, n + 5, den)
        mih.api._check(rc)


@pytest.mark.parametrize("den,new", [(5, 32765), (1, 32767)])
def test_regrid(mih, den, new):
    """regrid onto a finer grid: the numerators times new / den, 0xFFFF kept, mu_j and sinv_j BITWISE what they were (S m and
    N denom m are exact in a double, so the quotient rounds the same), X'r within the counted bound of the same exact value.  A
    multiple above 32767 and a non-multiple refuse and leave the handle as it was."""
    n = 1025
    num = edge_matrix(n, den, 700 + den)
    x = mih.DosageMatrix(num, den)
    mu, sinv = x.mu_sigma()
    R = residuals(n, 4, seed=701)
    before = x.xtv(R)
    check_exact(before, num, den, mu, sinv, R, "before")
    for refuse in (32770 if den == 5 else 32768, 32767 if den == 5 else 0, 7 if den == 5 else -1):
        with pytest.raises(mih.MendelIHTError):
            x.regrid(refuse)
        assert x.denom == den and np.array_equal(x.export(), num)
        assert np.array_equal(x.xtv(R), before)
    assert x.regrid(new) is x and x.denom == new
    fine = np.where(num == 0xFFFF, 0xFFFF, num.astype(np.int64) * (new // den)).astype(np.uint16)
    assert np.array_equal(x.export(), fine)
    mu2, sinv2 = x.mu_sigma()
    assert np.array_equal(mu2, mu) and np.array_equal(sinv2, sinv)
    after = x.xtv(R)
    check_exact(after, fine, new, mu, sinv, R, "after")                   # the exact value is the same one: fine / new = num / den
    ex = exact_xtv(num, den, mu, sinv, R[:, 0])
    assert ex == exact_xtv(fine, new, mu, sinv, R[:, 0])
    y = mih.DosageMatrix(fine, new)                                       # the regridded handle is the one created on that grid
    assert np.array_equal(y.xtv(R), after)
    assert np.array_equal(x.xv_sparse(np.array([3, 12, 0]), np.array([0.5, -2.0, 3.0])),
                          y.xv_sparse(np.array([3, 12, 0]), np.array([0.5, -2.0, 3.0])))


def test_range_check_and_pad_rows(mih):
    """n = 1025: seven pad rows follow the last real row in the same 16-byte load.  One numerator of 2 denom + 1 there, in the last
    column, is refused and counted once; without missing entries mu_j is the exact mean over exactly n rows (the pad rows the
    library writes are not counted), and X'r is exact within the bound: it sees them as missing."""
    n, den = 1025, 10000                                                  # (at 32767, 2 denom + 1 is the missing marker itself)
    rng = np.random.default_rng(800)
    num = rng.integers(0, 2 * den + 1, (n, 19)).astype(np.uint16)
    num[n - 1, :] = 2 * den
    bad = num.copy()
    bad[n - 1, 18] = 2 * den + 1
    with pytest.raises(mih.MendelIHTError, match=r"\b1 dosage numerators exceed 2 \* denom = 20000"):
        mih.DosageMatrix(bad, den)
    x = mih.DosageMatrix(num, den)
    mu, sinv = x.mu_sigma()
    for j in range(19):
        assert mu[j] == float(Fraction(int(num[:, j].astype(np.int64).sum()), n * den)), j
    R = residuals(n, 3, seed=801)
    check_exact(x.xtv(R), num, den, mu, sinv, R, "pad rows")
