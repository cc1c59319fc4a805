"""The inputs, exact values, bounds and plan restatements of tests/test_gpu_xtv_matrix_edges.py, checked without a GPU: the exact
functions against brute-force rational sums, the slice patterns and pass plans the GPU file's case names promise, and that every
(case, column) of the GPU file has a finite reference and a positive bound -- nothing is left unchecked there."""
from fractions import Fraction

import numpy as np
import pytest

from gpu_helpers import (XTV_COL_N, XTV_COL_P, XTV_FLAG_MISS, XTV_FLAG_RUNS, XTV_FLAG_SHAPES, XTV_FLAGS, XTV_KERNELS, XTV_PLAN_M,
                         XTV_PLAN_SHAPES, XTV_ROW_N, XTV_RUNS, EdgeCase, _codes, _dosages, peel_rule, snp_host_stats, xtv_matrix_cols,
                         xtv_matrix_exact, xtv_matrix_problem, xtv_plan, xtv_quantum, xtv_recombine_count, xtv_run_calls, xtv_slices,
                         xtv_std_exact)

FORMATS = (None, 4908, 1316, 1308, 428)


@pytest.mark.parametrize("n,p,miss", [(1, 9, 0.0), (5, 12, 0.3), (130, 10, 0.1), (259, 11, 0.02)])
def test_exact_functions_against_brute_force(n, p, miss):
    cols = xtv_matrix_cols(n, p, miss, last_row_missing=p >= 10)
    g, code = _dosages(cols, n), _codes(cols, n)
    mu, sinv = snp_host_stats(cols, n)
    assert np.isnan(mu[7]) and sinv[7] == 1.0 and mu[0] == 0.0 and mu[1] == 2.0 and sinv[0] == sinv[1] == 1.0
    rng = np.random.default_rng(n)
    for r in (rng.standard_normal(n) * 3.0, np.ones(n), np.eye(n)[n - 1] * 0.3):
        case = EdgeCase("r", r, rows=peel_rule(r))
        rf = [Fraction(float(v)) for v in r]
        for splits in (1, 16):
            raw = xtv_matrix_exact(cols, n, case, splits)
            exact, bounds, ulp = raw
            for j in range(p):
                dot = sum((int(g[j, i]) * rf[i] for i in range(n)), Fraction(0))
                dab = sum((int(g[j, i]) * abs(rf[i]) for i in range(n)), Fraction(0))
                cnt = sum(int(g[j, i]) for i in range(n) if i not in set(case.rows.tolist()))
                assert exact[j] == dot and ulp[j] == dab / 2 ** 53
                for dg in FORMATS:
                    want = Fraction(xtv_quantum(r, dg)) / 2 * cnt + xtv_recombine_count(dg, splits) * dab / 2 ** 53
                    assert bounds[dg][j] == want, (j, dg)
            for c, s, i in XTV_FLAGS:
                ex, bd = xtv_std_exact(cols, n, case, mu, sinv, c, s, i, raw)
                for j in range(p):
                    miss_rows = [t for t in range(n) if code[j, t] == 1]
                    if np.isnan(mu[j]) and (c or (i and miss_rows)):
                        assert ex[j] is None
                        continue
                    m, si = Fraction(float(mu[j])), Fraction(float(sinv[j])) if s else Fraction(1)
                    val = exact[j] + (m * sum((rf[t] for t in miss_rows), Fraction(0)) if i else 0) - (m * sum(rf, Fraction(0)) if c else 0)
                    assert ex[j] == si * val, (j, (c, s, i))
                    M = abs(m) * sum((abs(rf[t]) for t in miss_rows), Fraction(0)) if i else 0
                    S = abs(m) * sum((abs(v) for v in rf), Fraction(0)) if c else 0
                    dab = ulp[j] * 2 ** 53
                    tail = (max(len(miss_rows) - 1, 0) * M + (1 + 70) * S + 6 * (dab + M + S)) / 2 ** 53
                    assert bd[None][j] == abs(si) * (bounds[None][j] + tail), (j, (c, s, i))


SLICES = {2048: [8, 8], 2049: [9, 8], 4095: [8, 8, 8, 8], 4225: [9, 9, 9, 7], 8321: [9] * 7 + [3], 16400: [9] * 14 + [3, 0],
          28800: [15] * 15 + [0], 28801: [15] * 15 + [1]}


def test_slice_patterns():
    """The row cases are what their names say: one slice of 1 .. 15 blocks, then the named multi-slice patterns; the column and
    pass-plan shapes have one slice (385 rows) and 9 + 8 blocks (2049) at every p."""
    single = [n for n in XTV_ROW_N if n <= 1920]
    assert len(single) == 16 and len(XTV_ROW_N) == 16 + len(SLICES)
    nbs = [xtv_slices(n, 70) for n in single]
    assert all(len(s) == 1 for s in nbs)
    assert sorted({s[0] for s in nbs}) == [1, 2, 3, 4, 5, 8, 9, 15] and {-(-n // 128) for n in single} == {s[0] for s in nbs}
    for n, want in SLICES.items():
        assert xtv_slices(n, 70) == want, n
    assert 28801 - 128 * 15 * 15 == 1 and 16400 - 128 * 128 == 16
    for p in XTV_COL_P + (65, 70):
        assert xtv_slices(385, p) == [4] and xtv_slices(2049, p) == [9, 8]


def test_pass_plans_cover_every_kernel():
    seen = set()
    for dg, ms in XTV_PLAN_M.items():
        for m in ms:
            plan = xtv_plan(dg, m)
            assert sum(q[0] for q in plan) == m and all(1 <= q[1] <= 6 for q in plan), (dg, m)
            seen |= {q[3] for q in plan}
    assert seen == set(XTV_KERNELS) and len(XTV_KERNELS) == 16
    assert {q[3] for m in range(1, 20) for q in xtv_plan(None, m)} == {k for k in XTV_KERNELS if "dma16" in k}
    assert [xtv_plan(None, m)[0][1:3] for m in (1, 2, 4, 7, 10, 13, 17, 19)] == [(1, True), (1, False), (2, True), (3, True), (4, True), (5, True), (6, True), (6, False)]
    assert [q[:3] for q in xtv_plan(None, 304)] == [(19, 6, False)] * 16               # the last flat plan
    for m in (305, 307):                                                                  # per-operand layout: three residuals an operand
        plan = xtv_plan(None, m)
        assert all("k_xtv_dma16" in q[3] for q in plan)
        assert all(q[0] == 3 * q[1] for q in plan[:-1]) and plan[-1][0] == m - sum(q[0] for q in plan[:-1])
        assert 3 * (plan[-1][1] - 1) < plan[-1][0] <= 3 * plan[-1][1]
    assert not any(q[2] for q in xtv_plan(None, 305)) and xtv_plan(None, 307)[-1][2] and not any(q[2] for q in xtv_plan(None, 307)[:-1])
    assert [q[3] for q in xtv_plan(1316, 4)] == ["k_xtv_mfma_lds<2,4,1,4,fp4>"] and [q[3] for q in xtv_plan(1316, 6)] == ["k_xtv_mfma_lds<3,2,2,8,fp4>"]
    assert [q[3] for q in xtv_plan(1316, 8)] == ["k_xtv_mfma_lds<4,2,2,8,fp4>"] and [q[3] for q in xtv_plan(428, 1)] == ["k_xtv_dma<1,2,4,8,fp4>"]
    assert [q[:2] for q in xtv_plan(428, 9)] == [(4, 4), (3, 3), (2, 2)] and [q[:2] for q in xtv_plan(1316, 18)] == [(8, 4), (6, 3), (4, 2)]
    assert [q[:3] for q in xtv_plan(4908, 25)] == [(16, 4, False), (9, 3, True)] and [q[:3] for q in xtv_plan(4908, 5)] == [(5, 2, True)]


def test_recombination_counts():
    assert [xtv_recombine_count(dg, 1) for dg in FORMATS] == [18, 23, 33, 23, 28]
    assert xtv_recombine_count(None, 16) == 33 and xtv_recombine_count(None, 4) - xtv_recombine_count(None, 1) == 3


def _columns_checked(exact, bounds, g_nonzero, what):
    """Every column has a value to be held to: a positive bound where it has a non-zero entry; exact == bound == 0 otherwise (the
    GPU file's comparison |got - exact| <= bound then demands exactly 0)."""
    pairs = 0
    for dg, bd in bounds.items():
        for j, (e, b) in enumerate(zip(exact, bd)):
            if e is None:
                continue
            assert b > 0 or (b == 0 and e == 0 and not g_nonzero[j]), (what, dg, j)
            assert not g_nonzero[j] or b > 0, (what, dg, j)
            assert np.isfinite(float(e)) and np.isfinite(float(b)), (what, dg, j)
            pairs += 1
    return pairs


def _raw_inputs():
    for n in XTV_ROW_N:
        yield ("rows", n, 70, 19, sorted({t for dg, m in XTV_RUNS for call in xtv_run_calls(m) for t in call}))
    for n in XTV_COL_N:
        for p in XTV_COL_P:
            yield ("cols", n, p, 19, sorted({t for dg, m in XTV_RUNS for call in xtv_run_calls(m) for t in call}))
    for n, p in XTV_PLAN_SHAPES:
        yield ("plans", n, p, 307, list(range(307)))


def test_every_raw_input_has_a_reference_and_a_bound():
    pairs = 0
    for group, n, p, count, used in _raw_inputs():
        prob = xtv_matrix_problem(n, p, count=count)
        assert used == list(range(len(used))) and len(prob.cases) >= len(used)
        nz = (_dosages(prob.cols, n) != 0).any(axis=1)
        if p >= 9:
            assert not nz[0] and not nz[7] and nz[1] and nz[2] and nz[3] and nz[4] and (nz[6] == (len(prob.slices) > 1))
        kinds = [c.name.rstrip("0123456789") for c in prob.cases[:19]]
        assert kinds[0] == "gauss" and kinds[1] == "one" and kinds[2] == "unit" and (n < 2 or prob.cases[4].name == f"unit{n - 1}")
        for t in used:
            case = prob.cases[t]
            assert np.isfinite(case.r).all() and case.rows.tolist() == peel_rule(case.r).tolist()
            if case.name.startswith("unit"):
                assert np.count_nonzero(case.r) == 1 and case.rows.size == (1 if n > 256 else 0)       # more than one guard block: it rides the side channel
            exact, bounds, _ = prob.raw(t)
            pairs += _columns_checked(exact, bounds, nz, (group, n, p, case.name))
    assert pairs > 0


def test_every_standardized_input_has_a_reference_and_a_bound():
    for n, p in XTV_FLAG_SHAPES:
        for miss in XTV_FLAG_MISS:
            prob = xtv_matrix_problem(n, p, miss, 4, True)
            code = _codes(prob.cols, n)
            mu, sinv = snp_host_stats(prob.cols, n)
            assert (code[7] == 1).all() and np.isnan(mu[7])                                   # every entry missing
            assert np.flatnonzero(code[8] == 1).tolist() == [n - 1]                           # missing only in row n - 1
            assert mu[0] == 0.0 and mu[1] == 2.0 and sinv[0] == sinv[1] == 1.0                # monomorphic
            assert abs((code[9:] == 1).mean() - miss) < 0.25 * miss + 0.01
            nz = (_dosages(prob.cols, n) != 0).any(axis=1)
            for flags in XTV_FLAGS:
                for dg, m in XTV_FLAG_RUNS:
                    for call in xtv_run_calls(m, flags=True):
                        for t in call:
                            exact, bounds = prob.std(t, mu, sinv, flags)
                            assert [j for j, e in enumerate(exact) if e is None] == [7], (n, p, miss, flags)
                            _columns_checked(exact, bounds, nz, (n, p, miss, flags, prob.cases[t].name))
