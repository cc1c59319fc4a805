"""The matrix side of X'r over the 2-bit matrix at its edges (csrc/xtv.hip dispatch_xtv / auto_splits / plan_passes, csrc/xtv_kernels.h
row_slice, the ring prologue of k_xtv_dma / k_xtv_dma16, k_xtv_mfma_lds, the epilogues, k_xtv_finalize): all 16 kernel instantiations
of the release library, row slices of 1 .. 15 blocks (below, at and above the ring depths 3, 4 and 8), 2 .. 16 slices with short,
single-row and empty last slices, ragged column groups and idle waves around 32, 64, 256 and 512 columns, every pass plan up to the
per-operand FP6 layout beyond 304 residuals, and the missing-entry fix-up under every flag combination.

Every result is held to EXACT values (integers over one power of two; rationals over the handle's own mu and sinv for a standardized
matrix) at a bound that is counted from the source, not measured (gpu_helpers.xtv_matrix_exact / xtv_recombine_count / xtv_std_exact):
    |out_j - exact_j| <= (q / 2) sum_i g_ij [row i not peeled] + C x 2^-53 sum_i g_ij |r_i|,   C = 18 .. 48 by format and slice count.
After each call the pass records are compared with the restated plan (gpu_helpers.xtv_plan: kernel name, residuals and operands of
every pass) and the counter of peeled residuals with the guard's restatement.  A unit vector that the guard peels (n > 256) must
give the column's entry times its value EXACTLY: the fixed point is all zeros and the side channel adds one exact product.
tests/test_xtv_matrix_edges_cpu.py shows that the inputs, slice patterns and plans are what the case names say.

Each test prints its worst err / bound.  Measured on an MI355X: rows 0.65 .. 0.98, columns 0.03 (p = 1) .. 0.98, pass plans 0.09 .. 0.99,
flags 0.009 .. 0.16 -- the quantum term is sharp: on a column with a single entry err / bound is the rounding of ONE residual entry over
half its quantum, anything in [0, 1).  The whole file takes 20 s, the slowest case 2 s."""
import math
from fractions import Fraction

import numpy as np
import pytest

from gpu_helpers import (XTV_COL_N, XTV_COL_P, XTV_FLAG_MISS, XTV_FLAG_RUNS, XTV_FLAG_SHAPES, XTV_FLAGS, XTV_KERNELS, XTV_PLAN_M,
                         XTV_PLAN_SHAPES, XTV_ROW_N, XTV_RUNS, xtv_matrix_problem, xtv_plan, xtv_run_calls)

pytestmark = pytest.mark.gpu

_SEEN = set()          # kernel names in the pass records of this file's calls


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


def _call(mih, x, prob, idx, dg):
    """x.xtv of the residuals idx of the problem in format dg (None: the library default of every fused context); the pass records must
    be the restated plan, the peeled-residual counter the restatement's."""
    mih.profile_passes(x, reset=True)
    mih.profile_counters(x, reset=True)
    got = x.xtv(np.asfortranarray(prob.R[:, idx]), xtv_digits=dg)
    passes = [(q["kernel"], q["residuals"], q["operands"]) for q in mih.profile_passes(x, reset=True)]
    peeled = mih.profile_counters(x, reset=True)["peeled_residuals"]
    what = (prob.n, prob.p, dg, len(idx))
    assert passes == [(k, r, o) for r, o, _, k in xtv_plan(dg, len(idx))], what
    assert peeled == sum(1 for t in idx if prob.cases[t].rows.size), what + ("peeled residuals", peeled)
    _SEEN.update(k for k, _, _ in passes)
    return got


def _hold(got, exact, bound, what, case, bad):
    """Column by column: |got - exact| <= bound in rationals (NaN where the reference has no value); returns the worst err / bound."""
    worst = 0.0
    for j, (v, e, b) in enumerate(zip(got, exact, bound)):
        if e is None:
            if not math.isnan(v):
                bad.append(what + (case.name, j, float(v), "NaN expected"))
            continue
        if not math.isfinite(v):
            bad.append(what + (case.name, j, float(v), "not finite"))
            continue
        err = abs(Fraction(float(v)) - e)
        if b:
            worst = max(worst, float(err / b))
        if err > b:
            bad.append(what + (case.name, j, f"err / bound {float(err / b) if b else math.inf:.3g}"))
    return worst


def _check_raw(mih, x, prob, idx, dg, bad):
    got = _call(mih, x, prob, idx, dg)
    what = (prob.n, prob.p, dg, len(idx))
    worst = 0.0
    for v, t in enumerate(idx):
        case = prob.cases[t]
        exact, bounds, _ = prob.raw(t)
        worst = max(worst, _hold(got[:, v], exact, bounds[dg], what, case, bad))
        if case.name.startswith("unit") and case.rows.size:
            wrong = [j for j in range(prob.p) if Fraction(float(got[j, v])) != exact[j]]
            if wrong:
                bad.append(what + (case.name, wrong[:5], "a peeled unit vector gives the entry times its value exactly"))
    return got, worst


def _raw_matrix(mih, counted, prob):
    return counted(mih.SnpLinAlg(prob.cols, n=prob.n, center=False, scale=False, impute=False))


def _runs(mih, counted, n, p, tag):
    prob = xtv_matrix_problem(n, p)
    x = _raw_matrix(mih, counted, prob)
    bad, worst = [], 0.0
    for dg, m in XTV_RUNS:
        for idx in xtv_run_calls(m):
            _, w = _check_raw(mih, x, prob, idx, dg, bad)
            worst = max(worst, w)
    print(tag, n, p, "slices", prob.slices, f"worst err / bound {worst:.3g}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("n", XTV_ROW_N)
def test_row_slices(mih, counted, n):
    """p = 70 (three column groups: one half-idle wave and six idle ones).  One slice of 1 .. 15 blocks -- below, at and above the ring
    depths, odd and even; 2048: 8 + 8; 2049: 9 + 8; 4095: 4 x 8; 4225: 9, 9, 9, 7; 8321: 8 slices, the last of 3 blocks; 16400: 16 slices,
    slice 14 short, slice 15 empty; 28800: slice 15 empty behind a full slice 14; 28801: slice 15 is one block of one row.  The default
    format with 1 and 19 residuals, 428 with 1, 1316 with 4, 6 and 8 (the three k_xtv_mfma_lds shapes), 4908 with 5."""
    _runs(mih, counted, n, 70, "rows")


@pytest.mark.parametrize("p", XTV_COL_P)
@pytest.mark.parametrize("n", XTV_COL_N)
def test_column_groups(mih, counted, n, p):
    """p around 32 SNPs per group, 2 groups per wave and 256 / 512 SNPs per workgroup, at one slice (n = 385) and at two (n = 2049:
    a second workgroup per slice writes into the same `partial` layout).  The formats and residual counts of test_row_slices."""
    _runs(mih, counted, n, p, "cols")


@pytest.mark.parametrize("dg", list(XTV_PLAN_M))
@pytest.mark.parametrize("shape", XTV_PLAN_SHAPES)
def test_pass_plans(mih, counted, shape, dg):
    """Every pass plan: the default format with 1 .. 19 residuals (all twelve k_xtv_dma16<NR, .., half?>), 20, 38, 39, 304 (the last flat
    plan), 305 and 307 (the per-operand FP6 layout, 307 with a half pass); 4908, 1316, 428 and 1308 around every change of the operand
    count.  Column v of a fused result is, bit for bit, the same residual scored alone in the same format."""
    n, p = shape
    prob = xtv_matrix_problem(n, p, count=307)
    x = _raw_matrix(mih, counted, prob)
    bad, worst, alone = [], 0.0, {}
    for m in XTV_PLAN_M[dg]:
        got, w = _check_raw(mih, x, prob, list(range(m)), dg, bad)
        worst = max(worst, w)
        for v in range(m):
            if v not in alone:
                alone[v] = _call(mih, x, prob, [v], dg)[:, 0]
            if not np.array_equal(got[:, v].view(np.uint64), alone[v].view(np.uint64)):
                bad.append((n, p, dg, m, prob.cases[v].name, int(np.flatnonzero(got[:, v].view(np.uint64) != alone[v].view(np.uint64))[0]),
                            "fused differs from the residual scored alone"))
    print("plans", n, p, dg, f"worst err / bound {worst:.3g}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("miss", XTV_FLAG_MISS)
@pytest.mark.parametrize("flags", XTV_FLAGS)
@pytest.mark.parametrize("shape", XTV_FLAG_SHAPES)
def test_flags_and_missing_entries(mih, counted, shape, flags, miss):
    """(center, scale, impute) with 2 % and 30 % missing entries at one slice, two and sixteen, against the standardized reference in
    rationals over the handle's own mu and sinv: the column with every entry missing (NaN, as the reference's mean over no
    observation), a column missing only in row n - 1, monomorphic columns; the default format with 3 residuals, 428 with 1."""
    n, p = shape
    prob = xtv_matrix_problem(n, p, miss, 4, True)
    c, s, i = flags
    x = counted(mih.SnpLinAlg(prob.cols, n=n, center=c, scale=s, impute=i))
    mu, sinv = x.mu_sigma()
    bad, worst = [], 0.0
    for dg, m in XTV_FLAG_RUNS:
        for idx in xtv_run_calls(m, flags=True):
            got = _call(mih, x, prob, idx, dg)
            for v, t in enumerate(idx):
                exact, bounds = prob.std(t, mu, sinv, flags)
                worst = max(worst, _hold(got[:, v], exact, bounds[dg], (n, p, dg, len(idx), flags, miss), prob.cases[t], bad))
    print("flags", n, p, flags, miss, f"worst err / bound {worst:.3g}")
    assert not bad, bad[:8]


def test_all_sixteen_kernels_ran(mih, counted):
    """The union of the kernel names in this file's pass records is the release library's full set: twelve k_xtv_dma16, k_xtv_dma and
    three k_xtv_mfma_lds.  (Run alone, the test makes the calls that name them itself.)"""
    prob = xtv_matrix_problem(385, 70, count=307)
    x = _raw_matrix(mih, counted, prob)
    for dg, m in [(None, m) for m in range(1, 20)] + [(428, 1), (1316, 4), (1316, 6), (1316, 8)]:
        _call(mih, x, prob, list(range(m)), dg)
    assert _SEEN == set(XTV_KERNELS) and len(_SEEN) == 16, sorted(_SEEN ^ set(XTV_KERNELS))
