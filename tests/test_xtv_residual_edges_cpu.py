"""The inputs of tests/test_gpu_xtv_residual_edges.py are what their names say (no GPU): for every residual of
gpu_helpers.xtv_edge_problem the guard's restatement (peel_rule, peel_threshold) gives the rows the case is MEANT to have peeled,
the tie sits on the threshold exactly, the exact dot products and the derived bounds are finite -- so a failure of the GPU file is
the kernels', not the inputs'."""
import math
from fractions import Fraction

import numpy as np
import pytest

from gpu_helpers import XTV_EBITS, _codes, _dosages, peel_rule, peel_threshold, xtv_edge_exact, xtv_edge_problem, xtv_quantum

RAGGED_N = (255, 256, 257, 513, 769, 1023, 1025, 4097, 16383, 16385, 16640)
PROBLEMS = [("ragged", n) for n in RAGGED_N] + [("zero_blocks", 769), ("zero_blocks", 1025), ("limit", 3000), ("where", 1027),
                                                  ("company", 1025), ("scale", 513), ("huge", 513)]


@pytest.mark.parametrize("group,n", PROBLEMS)
def test_every_residual_is_what_its_name_says(group, n):
    cols, cases = xtv_edge_problem(group, n)
    cols2, cases2 = xtv_edge_problem(group, n)
    assert np.array_equal(cols, cols2) and all(np.array_equal(a.r, b.r, equal_nan=True) for a, b in zip(cases, cases2))       # deterministic
    assert 33 <= cols.shape[0] <= 70 and cols.shape[1] == (n + 3) // 4 and n <= 16640
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.r.shape == (n,) and np.all(np.isfinite(c.r)), c.name
        rows = peel_rule(c.r)
        assert rows.tolist() == c.rows.tolist(), (group, n, c.name, rows, c.rows)
        tau, fmx = peel_threshold(c.r)
        if c.fires is not None:
            assert (fmx > tau) == c.fires, (group, n, c.name, tau, fmx)
        if c.rows.size:
            assert c.rows.size <= 64 and np.all(np.abs(c.r[c.rows]) > tau)
            rest = np.delete(np.abs(c.r), c.rows)
            assert rest.size == 0 or rest.max() <= tau
        elif fmx > tau:
            assert np.count_nonzero(np.abs(c.r) > tau) > 64, (group, n, c.name)          # the guard fired and found a heavy tail
        if c.expect == "nan":
            with np.errstate(over="ignore"):
                assert not math.isfinite(float(np.sum(c.r)))
            continue
        assert math.isfinite(float(np.sum(np.abs(c.r))))                                  # no order of the sum overflows
        for dg in (None, 4908, 1308):
            exact, bound, ulp = xtv_edge_exact(cols, n, c, dg)
            assert all(math.isfinite(float(v)) for v in exact), (group, n, c.name)
            assert all(math.isfinite(float(v)) and v >= 0 for v in bound), (group, n, c.name)
            assert all(b >= 8 * u for b, u in zip(bound, ulp))


def test_named_properties_of_the_cases():
    _, cases = xtv_edge_problem("limit", 3000)
    by = {c.name: c for c in cases}
    assert by["lim64"].rows.size == 64 and by["lim65"].rows.size == 0
    assert np.count_nonzero(np.abs(by["lim65"].r) > peel_threshold(by["lim65"].r)[0]) == 65
    cols, _ = xtv_edge_problem("limit", 3000)
    g = _dosages(cols, 3000)
    assert np.all(g[:8][:, by["lim64"].rows] == 0) and np.all(g[8:][:, by["lim64"].rows].sum(axis=1) > 0)
    # the tie: max|r| == 64 bq exactly (both powers of two); its neighbour is one ulp above
    tau, fmx = peel_threshold(by["tie"].r)
    assert tau == fmx == 64.0 and by["tie"].rows.size == 0
    tau, fmx = peel_threshold(by["tie_up"].r)
    assert tau == 64.0 and fmx == np.nextafter(64.0, np.inf) and by["tie_up"].rows.size == 1
    assert np.array_equal(np.flatnonzero(by["tie"].r != by["tie_up"].r), by["tie_up"].rows)
    # tau = 0: every non-zero row is peeled when there are at most 64, none when there are more
    for n in (769, 1025):
        _, cases = xtv_edge_problem("zero_blocks", n)
        for c in cases:
            assert peel_threshold(c.r)[0] == 0.0, (n, c.name)
            nz = np.flatnonzero(c.r)
            assert c.rows.tolist() == (nz.tolist() if nz.size <= 64 else []), (n, c.name)
        assert [np.count_nonzero(c.r) for c in cases[2:]] == [64, 10, 1] and all(np.count_nonzero(c.r) > 64 for c in cases[:2])
    # ragged d: an ORDINARY residual the guard peels ten rows of, because the last block is one small row
    for n in RAGGED_N:
        _, cases = xtv_edge_problem("ragged", n)
        assert cases[3].rows.size == (10 if n in (257, 513, 769) else 0), n
        assert np.all(np.abs(cases[2].r) == 1.0)
    # where: the third outlier sits on a row where a column's genotype is missing
    cols, cases = xtv_edge_problem("where", 1027)
    code = _codes(cols, 1027)
    assert [c.rows.tolist() for c in cases[:2]] == [[1026], [0]] and (code[:, cases[2].rows[0]] == 1).any()
    _, cases = xtv_edge_problem("company", 1025)
    assert len(cases) == 23 and sum(c.rows.size > 0 for c in cases) >= 7 and sum(c.name.startswith("gauss") for c in cases) == 8


def test_scale_rule_restated():
    """xtv_quantum: 2^-(ebits - ilogb(top)), at powers of two, just below them, for denormals (capped at 2^-1000) and huge entries."""
    one = np.array([0.5, -1.0, 0.25])
    for dg, eb in XTV_EBITS.items():
        assert xtv_quantum(one, dg) == 2.0 ** -eb
        assert xtv_quantum(np.array([np.nextafter(1.0, 0.0), 0.1]), dg) == 2.0 ** -(eb + 1)
        assert xtv_quantum(np.array([-2.0 ** 600, 1.0]), dg) == 2.0 ** (600 - eb)
        assert xtv_quantum(np.array([2.0 ** -1022, 0.0]), dg) == 2.0 ** -1000 == xtv_quantum(np.array([2.0 ** -1074]), dg)
        assert xtv_quantum(np.array([2.0 ** 1022]), dg) == 2.0 ** (1022 - eb)
        assert xtv_quantum(np.zeros(5), dg) == 1.0
    # the rows the guard takes out do not set the scale
    r = np.random.default_rng(1).standard_normal(3000)
    r[np.argmax(np.abs(r))] = 3.5
    r[2000] = 1e9
    assert peel_rule(r).tolist() == [2000] and xtv_quantum(r) == 2.0 ** -52
    _, cases = xtv_edge_problem("scale", 513)
    assert len(cases) == 21
    for c in cases[:-1]:
        k = int(c.name.split("_k")[1].split("_")[0])
        top = np.abs(c.r).max()
        assert top == (2.0 ** k if c.name.startswith("pow2") else np.nextafter(2.0 ** k, 0.0)), c.name
        assert (c.r[np.argmax(np.abs(c.r))] > 0) == c.name.endswith("pos")
        e = 53 - (k if c.name.startswith("pow2") else k - 1)
        assert Fraction(xtv_quantum(c.r)) == Fraction(2) ** -min(e, 1000), c.name
    assert 0 < np.abs(cases[-1].r).max() < 2.0 ** -1022 and xtv_quantum(cases[-1].r) == 2.0 ** -1000
    _, cases = xtv_edge_problem("huge", 513)
    assert [np.abs(c.r).max() for c in cases] == [9.9e299, 1e300, 1e305, 1e305, 2.0 ** 1022, 2.0 ** 1022, 1.5e308]
