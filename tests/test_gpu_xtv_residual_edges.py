"""The residual front end of X'r over the 2-bit matrix at its edges (csrc/xtv_digits.hip k_r_stats / k_digits, csrc/peel.h, k_xtv_finalize;
k_res_stats + k_res_peel in a resident step): the guard's block quartile on ragged, few and all-zero blocks, the 64-row limit and
the strict `>` of its threshold, where the peeled row sits, company in fused passes, the power-of-two scale at powers of two, below
them, for denormals and in the short formats, finite residuals up to 2^1022, and fits whose training mask holds out whole blocks.

Every result on a raw-dosage matrix is held to EXACT dot products (integers over one power of two) at a bound that is derived, not
measured (gpu_helpers.xtv_edge_exact):  |out_j - exact_j| <= (q / 2) sum_i g_ij [row i not peeled] + 8 x 2^-53 sum_i g_ij |r_i|,
q = 2^-e the quantum of the scale rule's restatement (gpu_helpers.xtv_quantum); a peeled residual also to 2 x 2^-53 sum_i g_ij |r_i|, the
figure test_xtv_fixed_point_under_adversarial_dynamic_range asserts.  The counter of peeled residuals is read beside every result
and compared with the guard's restatement (gpu_helpers.peel_rule).  tests/test_xtv_residual_edges_cpu.py shows that the inputs are
what their names say.

What the tests establish about the guard on small n (peel.h): with a single-row or an all-zero block among four or fewer
the threshold is tiny or 0 and the guard FIRES on ordinary residuals ("ragged" a and d, every "zero_blocks" case) -- it rescans the
rows, peels up to 64 of them or none, and the result keeps the accuracy above either way.

Two findings of these tests, both fixed with them: (1) a finite residual with max|r| >= 1e300 kept the scale 2^0, its entries
saturated the conversion to integers and the row came out finite and wrong (max|r| = 1e300: 2e14 x the bound) -- the scale rule now
takes every finite maximum; (2) with all 64 non-zero rows of a residual peeled, the plain chain of 64 additions in k_xtv_finalize was
2.5 x 2^-53 sum_i g_ij |r_i| off in two columns (n = 1025), over the 2 ulp-sums a peeled residual is held to -- the side channel now
adds its terms in a compensated sum."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from gpu_helpers import _same_fit, peel_rule, xtv_edge_exact, xtv_edge_problem

pytestmark = pytest.mark.gpu

FORMATS = (None, 428, 1316)
RAGGED_N = (255, 256, 257, 513, 769, 1023, 1025, 4097, 16383, 16385, 16640)
FLAGS = [(1, 1, 1), (1, 1, 0), (0, 0, 1), (1, 0, 1)]


@functools.lru_cache(maxsize=None)
def _problem(group, n):
    return xtv_edge_problem(group, n)


@functools.lru_cache(maxsize=None)
def _exact(group, n, t, ebits_of):
    """(exact, bound, ulp-sum) of case t of a problem, computed once per quantum (formats with the same ebits share it)."""
    cols, cases = _problem(group, n)
    return xtv_edge_exact(cols, n, cases[t], ebits_of)


def _raw(mih, group, n):
    cols, cases = _problem(group, n)
    return mih.SnpLinAlg(cols, n=n, center=False, scale=False, impute=False), cases


def _xtv_counted(mih, x, R, dg):
    """x.xtv of the columns of R in the fused workspace (format None = the library default of every multi-residual context, 4910) and
    how many residuals of the call had rows peeled."""
    mih.profile_counters(x, reset=True)
    got = x.xtv(np.asfortranarray(R.reshape(x.n, -1)), xtv_digits=dg)
    return got, mih.profile_counters(x, reset=True)["peeled_residuals"]


def _misses(got, exact, bound, ulp, peeled):
    """Columns outside the derived bound (and, for a peeled residual, outside 2 ulp-sums): [(column, err / bound, err / ulp-sum)]."""
    bad = []
    for j in range(len(exact)):
        if not math.isfinite(got[j]):
            bad.append((j, float(got[j]), None))
            continue
        err = abs(Fraction(float(got[j])) - exact[j])
        if err > bound[j] or (peeled and err > 2 * ulp[j]):
            bad.append((j, float(err / bound[j]) if bound[j] else math.inf, float(err / ulp[j]) if ulp[j] else math.inf))
    return bad


def _check_case(mih, x, group, n, t, case, dg, report):
    got, cnt = _xtv_counted(mih, x, case.r, dg)
    got = got[:, 0]
    want = 1 if case.rows.size else 0
    assert peel_rule(case.r).tolist() == case.rows.tolist()
    assert cnt == want, (group, n, case.name, dg, "peeled residuals", cnt, "restatement", case.rows.tolist())
    exact, bound, ulp = _exact(group, n, t, 428 if dg is None else dg)                   # (None = 4910 and 428 share ebits = 53)
    if case.expect == "nan" or (case.expect == "bound_or_nan" and np.isnan(got).all()):
        assert np.isnan(got).all(), (group, n, case.name, dg, got)
        report.append((case.name, dg, "NaN in every column"))
        return got
    bad = _misses(got, exact, bound, ulp, bool(want))
    worst = max((float(abs(Fraction(float(v)) - e) / b) for v, e, b in zip(got, exact, bound) if b and math.isfinite(v)), default=0.0)
    report.append((case.name, dg, f"max err / bound {worst:.3g}"))
    print(group, n, case.name, dg, f"peeled {cnt}", f"max err / bound {worst:.3g}")
    assert not bad, (group, n, case.name, dg, bad[:5])
    return got


@pytest.fixture()
def counted(mih):
    """Matrices whose measurement hook is on for the test."""
    on = []

    def enable(x):
        mih.profile_enable(x, True)
        on.append(x)
        return x
    yield enable
    for x in on:
        mih.profile_enable(x, False)


@pytest.mark.parametrize("n", RAGGED_N)
def test_ragged_guard_blocks(mih, counted, n):
    """(case 1) The guard's blocks at n around the block size, the quartile's steps (4 -> 5 blocks) and the first wrap of the strided
    blocks (16385, 16640): a: Gaussian with a 2^-20 last row (tau = 2^-14 where that row is a block of its own among <= 4: the guard fires
    and finds a heavy tail); b: Gaussian; c: every entry +-1 (all maxima tie); d: a clipped Gaussian of which the guard peels ten rows
    at n = 257, 513, 769 because the last block is one small row."""
    x, cases = _raw(mih, "ragged", n)
    counted(x)
    report = []
    for dg in FORMATS:
        for t, case in enumerate(cases):
            _check_case(mih, x, "ragged", n, t, case, dg, report)


@pytest.mark.parametrize("n", [769, 1025])
def test_all_zero_blocks(mih, counted, n):
    """(case 2) What a contiguous held-out fold leaves: whole 256-row blocks of zeros, tau = 0.  More than 64 non-zero rows: no peel;
    64, 10, 1 non-zero rows: every one of them rides the f64 side channel, the fixed point is all zeros and its scale comes from
    rest = 0 -- the result is the plain f64 sum of those rows."""
    x, cases = _raw(mih, "zero_blocks", n)
    counted(x)
    report = []
    for dg in FORMATS:
        for t, case in enumerate(cases):
            got = _check_case(mih, x, "zero_blocks", n, t, case, dg, report)
            if case.name == "nz1":                                   # a unit vector: the row of X itself, exactly
                assert [Fraction(float(v)) for v in got] == _exact("zero_blocks", n, t, 428 if dg is None else dg)[0]


@pytest.mark.parametrize("flags", FLAGS)
def test_unit_vector_gives_the_standardized_row(mih, oracle, counted, flags):
    """(case 2) The unit vector on a matrix with flags and 2 % missing entries: the only non-zero row is peeled and X'e_i is row i of the
    standardized matrix, to the bound test_ragged_missing_flags holds X'r to."""
    n = 1025
    cols, _ = _problem("company", n)                                # (2 % missing)
    _, cases = _problem("zero_blocks", n)
    case = cases[-1]
    c, s, i = flags
    x = counted(mih.SnpLinAlg(cols, n, center=c, scale=s, impute=i))
    ref = oracle.Mat.from_bed_columns(cols, n, center=c, scale=s, impute=i).xtv(case.r)
    for dg in FORMATS:
        got, cnt = _xtv_counted(mih, x, case.r, dg)
        assert cnt == 1, (flags, dg, cnt)
        assert np.max(np.abs(got[:, 0] - ref)) < 1e-11 * max(np.max(np.abs(ref)), np.sum(np.abs(case.r))), (flags, dg)


def test_the_sixty_four_row_limit_and_the_threshold_tie(mih, counted):
    """(case 3) 64 rows 2^30 x the rest are peeled (columns that carry none of them: within 1e-13 of their own value), 65 are not
    (the plain quantum); max|r| == 64 bq exactly peels nothing (the guard's `>` is strict), one ulp more peels that row."""
    n = 3000
    x, cases = _raw(mih, "limit", n)
    counted(x)
    report = []
    for dg in FORMATS:
        for t, case in enumerate(cases):
            got = _check_case(mih, x, "limit", n, t, case, dg, report)
            if case.name == "lim64":
                exact = _exact("limit", n, t, 428 if dg is None else dg)[0][:8]           # columns 0 .. 7 carry none of the 64 rows
                rel = np.array([float(abs(Fraction(float(v)) - e) / abs(e)) for v, e in zip(got[:8], exact) if abs(e) >= 1])
                assert rel.size >= 4 and rel.max() <= 1e-13, (dg, rel)


@pytest.mark.parametrize("flags", FLAGS)
def test_where_the_peeled_row_sits(mih, oracle, counted, flags):
    """(case 4) n = 1027 (no multiple of 4, 16 or 64): the outlier on the last row, on row 0 and on a row where a column's genotype is
    missing, every flag combination of test_ragged_missing_flags, against the oracle at that test's bound."""
    n = 1027
    cols, cases = _problem("where", n)
    c, s, i = flags
    x = counted(mih.SnpLinAlg(cols, n, center=c, scale=s, impute=i))
    ox = oracle.Mat.from_bed_columns(cols, n, center=c, scale=s, impute=i)
    for case in cases:
        ref = ox.xtv(case.r)
        for dg in FORMATS:
            got, cnt = _xtv_counted(mih, x, case.r, dg)
            assert cnt == 1 and peel_rule(case.r).tolist() == case.rows.tolist(), (flags, case.name, dg, cnt)
            err = np.max(np.abs(got[:, 0] - ref)) / max(np.max(np.abs(ref)), np.sum(np.abs(case.r)))
            print("where", flags, case.name, dg, f"err {err:.3g}")
            assert err < 1e-11, (flags, case.name, dg, err)


def test_where_the_peeled_row_sits_exactly(mih, counted):
    """(case 4) The same three residuals on the raw dosages (2 % missing entries stored as 0), against exact values."""
    n = 1027
    x, cases = _raw(mih, "where", n)
    counted(x)
    for dg in FORMATS:
        for t, case in enumerate(cases):
            _check_case(mih, x, "where", n, t, case, dg, [])


def test_company_in_fused_passes(mih, counted):
    """(case 5) 23 residuals of every kind above and plain Gaussians in ONE call (two passes of the flat packing in the default
    format): each to its derived bound, the counter equal to the number the restatement peels, and every residual's row bit for
    bit what it gives alone and among the first 1, 4 and 19.  (428 rides one residual per operand, and a single residual takes another
    kernel than two or more: its fused call is held to the bounds and to itself, not to the single call.)"""
    n = 1025
    x, cases = _raw(mih, "company", n)
    counted(x)
    R = np.asfortranarray(np.stack([c.r for c in cases], axis=1))
    want = sum(1 for c in cases if c.rows.size)
    assert want == sum(1 for c in cases if peel_rule(c.r).size) and 7 <= want < 23
    for dg in FORMATS:
        got, cnt = _xtv_counted(mih, x, R, dg)
        assert cnt == want, (dg, cnt, want)
        for t, case in enumerate(cases):
            exact, bound, ulp = _exact("company", n, t, 428 if dg is None else dg)
            bad = _misses(got[:, t], exact, bound, ulp, bool(case.rows.size))
            assert not bad, (dg, case.name, bad[:5])
        again, _ = _xtv_counted(mih, x, R, dg)
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64)), dg
        if dg == 428:
            continue
        for m in (1, 4, 19):
            part, cnt = _xtv_counted(mih, x, R[:, :m], dg)
            assert cnt == sum(1 for c in cases[:m] if c.rows.size), (dg, m, cnt)
            assert np.array_equal(part.view(np.uint64), got[:, :m].view(np.uint64)), (dg, m)
        for t, case in enumerate(cases):
            alone, cnt = _xtv_counted(mih, x, case.r, dg)
            assert cnt == (1 if case.rows.size else 0), (dg, case.name, cnt)
            assert np.array_equal(alone[:, 0].view(np.uint64), got[:, t].view(np.uint64)), (dg, case.name)


@pytest.mark.parametrize("dg", [None, 4908, 1316, 1308, 428])
def test_scale_rule_at_powers_of_two(mih, counted, dg):
    """(case 6) e = ebits - ilogb(top), capped at 1000: max|r| = 2^k and the double below it, k = -1022, -600, 0, 1, 600, the extreme
    entry positive and negative (the base-4 digits are asymmetric: -2 .. 1), a residual of denormals only; all five formats (in the two
    short ones the quantum term of the bound dominates)."""
    n = 513
    x, cases = _raw(mih, "scale", n)
    counted(x)
    report = []
    for t, case in enumerate(cases):
        got, cnt = _xtv_counted(mih, x, case.r, dg)
        assert cnt == 0, (dg, case.name, cnt)
        exact, bound, ulp = _exact("scale", n, t, dg)
        bad = _misses(got[:, 0], exact, bound, ulp, False)
        worst = max(float(abs(Fraction(float(v)) - e) / b) for v, e, b in zip(got[:, 0], exact, bound) if math.isfinite(v))
        print("scale", dg, case.name, f"max err / bound {worst:.3g}")
        assert not bad, (dg, case.name, bad[:5])


def test_huge_finite_residuals(mih, counted):
    """(case 7) Finite residuals with max|r| >= 1e300 (9.9e299 for the other side of the old limit) up to 2^1022: the scale rule gives
    every finite maximum its exponent, so the values are correct to the derived bound -- or NaN in every column, never a finite wrong
    number.  Two entries of 1.5e308: sum r overflows, NaN in every column as for an Inf entry.  The other residuals of the call keep
    their bits."""
    n = 513
    x, cases = _raw(mih, "huge", n)
    counted(x)
    rng = np.random.default_rng(8)
    plain = rng.standard_normal((n, 4))
    report = []
    for dg in FORMATS:
        for t, case in enumerate(cases):
            _check_case(mih, x, "huge", n, t, case, dg, report)
        calm, _ = _xtv_counted(mih, x, plain, dg)                        # four Gaussians ...
        for t, case in enumerate(cases):
            mixed = plain.copy()
            mixed[:, 1] = case.r                                          # ... and the same call with a huge one in their midst
            got, cnt = _xtv_counted(mih, x, mixed, dg)
            assert cnt == (1 if case.rows.size else 0), (dg, case.name, cnt)
            for v in (0, 2, 3):
                assert np.array_equal(got[:, v].view(np.uint64), calm[:, v].view(np.uint64)), (dg, case.name, v)
            alone, _ = _xtv_counted(mih, x, case.r, dg)
            if dg != 428:
                assert np.array_equal(got[:, 1].view(np.uint64), alone[:, 0].view(np.uint64)), (dg, case.name)
    print(report)
    assert all(what != "NaN in every column" for name, dg, what in report if name != "sum_overflows"), report      # the values are correct


def _blocks_mask(n, held):
    train = np.ones(n, np.uint8)
    for b in held:
        train[256 * b:256 * (b + 1)] = 0
    return train


@pytest.mark.parametrize("n", [769, 16640])
def test_resident_fits_with_whole_blocks_held_out(mih, oracle, n):
    """(case 8) The guard inside a resident step (k_res_stats + k_res_peel make the decision there) on the residuals a training mask
    that holds out whole 256-row blocks leaves -- zeros over whole blocks, tau = 0 at n = 769 -- and on a Poisson fit with a planted count
    in the last, single-row block: step_mode 0 against step_mode 1 bit for bit, and both against the oracle at the tolerances of
    test_fit_iht_families_vs_oracle."""
    p = 64
    x = mih.SnpLinAlg.synthetic(n, p, seed=31)
    ox = oracle.Mat.from_bed_columns(x.export_bed(), n)
    rng = np.random.default_rng(5 + n)
    supp = np.sort(rng.choice(p, 4, replace=False))
    eta = x.xv_sparse(supp, np.array([0.6, -0.5, 0.4, 0.5]))
    held = (1,) if n == 769 else (0, 7, 8, 30, 63)
    train = _blocks_mask(n, held)
    if n == 769:
        train[768] = 0                                      # the single-row last block is held out too
    yn = eta + 1.0 + rng.standard_normal(n)
    yp = rng.poisson(np.exp(0.3 * eta)).astype(float)
    runs = [("normal", yn, dict(train=train), dict(), dict(), 1e-5),
            ("poisson", yp, dict(train=train), dict(d=mih.Poisson(), l=mih.LogLink()), dict(dist="poisson", link="log"), 1e-4)]
    if n == 769:
        yo = yp.copy()
        yo[768] = 400.0                                     # a count the model has not caught up with, alone in its block
        runs.append(("poisson, planted count", yo, dict(), dict(d=mih.Poisson(), l=mih.LogLink()), dict(dist="poisson", link="log"), 1e-4))
    mih.profile_enable(x, True)
    try:
        for what, y, tkw, kw, okw, tol in runs:
            mih.profile_counters(x, reset=True)
            a = mih.fit_iht(y, x, None, k=4, verbose=False, step_mode=0, **tkw, **kw)
            cnt = mih.profile_counters(x, reset=True)
            b = mih.fit_iht(y, x, None, k=4, verbose=False, step_mode=1, **tkw, **kw)
            host = mih.profile_counters(x, reset=True)
            _same_fit(a, b, (n, what))
            assert cnt["resident_steps"] > 0 and host["resident_steps"] == 0, (n, what, cnt, host)
            assert cnt["peeled_residuals"] == host["peeled_residuals"], (n, what, cnt, host)          # the same decisions in either kernel
            if "planted" in what:
                assert cnt["peeled_residuals"] >= 1, (n, what, cnt)
            o = oracle.fit_iht(ox, y, None, k=4, **tkw, **okw)
            print("resident", n, what, "iter", a.iter, "peeled", cnt["peeled_residuals"])
            assert a.iter == o["iter"], (n, what, a.iter, o["iter"])
            assert list(a.trace["backtracks"]) == list(o["bt_trace"]), (n, what)
            nz = np.flatnonzero(o["beta"])
            assert np.array_equal(np.flatnonzero(a.beta), nz), (n, what)
            np.testing.assert_allclose(a.beta[nz], o["beta"][nz], rtol=tol, err_msg=str((n, what)))
            np.testing.assert_allclose(a.c, o["c"], rtol=tol, err_msg=str((n, what)))
            assert a.logl == pytest.approx(o["logl"], rel=1e-9), (n, what)
    finally:
        mih.profile_enable(x, False)


def test_cv_with_contiguous_folds(mih, oracle):
    """(case 8) cv_iht at n = 769 with CONTIGUOUS folds: every training residual is zero over a run of whole blocks, in every pass of
    the lock-step lanes.  Both lock-step drivers (resident and host-driven steps) give the same losses bit for bit, and the
    oracle's at the tolerance of test_cv_iht_vs_oracle_and_sharding."""
    n, p, q = 769, 64, 3
    x = mih.SnpLinAlg.synthetic(n, p, seed=31)
    ox = oracle.Mat.from_bed_columns(x.export_bed(), n)
    rng = np.random.default_rng(774)
    supp = np.sort(rng.choice(p, 4, replace=False))
    y = x.xv_sparse(supp, np.array([0.6, -0.5, 0.4, 0.5])) + 1.0 + rng.standard_normal(n)
    folds = (np.arange(n) * q // n + 1).astype(np.int32)
    raws = []
    for mode in (0, 1):
        mih.set_step_mode(mode)
        try:
            mse, raw = mih.cv_iht(y, x, None, path=[2, 4], q=q, folds=folds, verbose=False, return_raw=True)
        finally:
            mih.set_step_mode(0)
        raws.append(np.asarray(raw))
    assert np.array_equal(raws[0].view(np.uint64), raws[1].view(np.uint64))
    omse, oraw = oracle.cv_iht(ox, y, None, path=[2, 4], q=q, folds=folds)
    np.testing.assert_allclose(raws[0].reshape(oraw.shape), oraw, rtol=1e-5)
    np.testing.assert_allclose(mse, omse, rtol=1e-5)
