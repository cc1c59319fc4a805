"""tests/init_beta_spec.py without a GPU: the statement against np.linalg.lstsq, its failure branch, its three evaluations against
each other, and -- for every case tests/test_gpu_init_beta.py runs -- the conditions that test relies on, in exact arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import assoc_spec as A
import init_beta_spec as S

ALL_CASES = S.snp_cases() + S.dense_cases()


def _x_of(inp):
    return A.xtilde(inp.codes, inp.case.flags) if inp.case.kind == "snp" else inp.X


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c.n <= 8320 and not c.one_training_row], ids=lambda c: c.id)
def test_the_statement_is_least_squares_on_the_training_rows(case):
    """(b0, b1) = argmin |y - b0 - b1 x_j| over T, to 1e-9 of the pair's size, on the columns with d / Sxx >= 0.1."""
    inp = S.inputs(case)
    ex, X, T = inp.exact, _x_of(inp), inp.w != 0
    skip = set(S.undetermined(inp)) | ({inp.planted["a"]} if "a" in inp.planted else set())
    for j in range(case.p):
        if j in skip:
            continue
        assert ex.d[j] >= Fraction(1, 10) * ex.Sxx[j]
        ls = np.linalg.lstsq(np.column_stack([np.ones(int(T.sum())), X[T, j]]), inp.Y[T], rcond=None)[0]       # 2 x m
        for t in range(case.m):
            got = np.array([float(ex.b0[t][j]), float(ex.b1[t][j])])
            assert np.max(np.abs(got - ls[:, t])) <= 1e-9 * np.max(np.abs(ls[:, t])), (case.id, j, t, got, ls[:, t])


def test_the_failure_branch_returns_the_unsolved_right_hand_side():
    Sy, Sxy = Fraction(7, 3), Fraction(-5, 8)
    assert S.solve_exact(0, Fraction(0), Sxy, Fraction(0), Sy)[:2] == (Sy, Sxy)                       # no training row
    assert S.solve_exact(4, Fraction(6), Sxy, Fraction(9), Sy) == (Sy, Sxy, Fraction(0))              # constant column: d = 9 - 36 / 4
    assert S.solve_exact(4, Fraction(6), Sxy, Fraction(8), Sy)[:2] == (Sy, Sxy)                       # d < 0 (as rounding can leave it)
    b0, b1, d = S.solve_mp(4, 6.0, -0.625, 9.0, 2.5)
    assert (float(b0), float(b1), float(d)) == (2.5, -0.625, 0.0)
    assert S.clamp(Fraction(5, 2)) == 2.0 and S.clamp(Fraction(-9, 2)) == -2.0 and S.clamp(Fraction(1, 4)) == 0.25
    # the planted columns of a committed case take it: (a) gives (Sy, 0) exactly, (c) (Sy, Sxy)
    inp = S.inputs(next(c for c in S.snp_cases() if c.p == 33 and c.mask == "random80" and c.n == 129))
    ex = inp.exact
    a, c = inp.planted["a"], inp.planted["c"]
    assert ex.d[a] == 0 and ex.Sx[a] == 0 and ex.Sxx[a] == 0 and (ex.b0[0][a], ex.b1[0][a]) == (ex.Sy[0], 0)
    assert ex.d[c] == 0 and (ex.b0[0][c], ex.b1[0][c]) == (ex.Sy[0], ex.Sxy[0][c])


def test_the_three_evaluations_agree():
    """solve_mp on the exact sums gives the rational solution; the class-sum route equals the row-by-row route of exact_dense on
    the same rational entries; solve_bound is positive and small."""
    inp = S.inputs(next(c for c in S.snp_cases() if (c.n, c.p, c.m) == (129, 33, 2)))
    ex, case = inp.exact, inp.case
    for j in range(case.p):
        if j in S.undetermined(inp) or j == inp.planted["a"]:
            continue
        for t in range(case.m):
            b0, b1, d = S.solve_mp(ex.N, ex.Sx[j], ex.Sxy[t][j], ex.Sxx[j], ex.Sy[t])
            assert abs(float(b1) - float(ex.b1[t][j])) <= 1e-15 * abs(float(b1)) and abs(float(b0) - float(ex.b0[t][j])) <= 1e-15 * abs(float(b0))
            db0, db1 = S.solve_bound(ex.N, ex.Sx[j], ex.Sxy[t][j], ex.Sxx[j], ex.Sy[t], b0, b1, d, S.E_XX_SNP)
            assert 0 < db1 <= 1e-12 * max(abs(float(b1)), 1.0) and 0 < db0 <= 1e-12 * max(abs(float(b0)), 1.0)
    # uncentred, unscaled: the entries are the allele counts themselves, doubles, so exact_dense must give the same rationals
    raw = next(c for c in S.snp_cases() if c.flags == (0, 0, 1) and c.missing == 0.0 and c.n == 129)
    inp = S.inputs(raw)
    X = A.xtilde(inp.codes, raw.flags)
    dn = S.exact_dense(X, inp.w, inp.Y)
    keep = [j for j in range(raw.p) if (inp.codes[:, j] >= 0).all()]           # (planted (b) columns carry the rounded mean)
    assert keep and all(dn.Sx[j] == inp.exact.Sx[j] and dn.Sxx[j] == inp.exact.Sxx[j] and dn.Sxy[0][j] == inp.exact.Sxy[0][j] for j in keep)
    assert dn.N == inp.exact.N and dn.Sy == inp.exact.Sy


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_conditions_of_the_device_test(case):
    inp = S.inputs(case)
    assert S.conditions(inp) == []
    T = inp.w != 0
    assert set(np.unique(inp.w)) <= {0.0, 1.0} and int(T.sum()) == inp.exact.N and (case.one_training_row or inp.exact.N >= 8)
    Yi = inp.Y * S.YQ
    assert np.array_equal(Yi, np.rint(Yi)) and np.abs(inp.Y).max() < 2 ** 10
    if case.kind == "snp":
        assert np.array_equal(inp.exact.cnt, S.train_counts(inp.codes, inp.w))
        if case.p >= S.PLANT_MIN_P:
            want = {"a", "b_in", "jstar"} | ({"b_out", "c"} if case.mask != "all" else set())
            assert set(inp.planted) == want and len(set(inp.planted.values())) == len(want)
            assert S.undetermined(inp) == (list(range(case.p)) if case.one_training_row else ([inp.planted["c"]] if "c" in inp.planted else []))
        else:
            assert inp.planted == {} and S.undetermined(inp) == []
    if case.mask == "blocks":
        B = S.COUNT_BLOCK_ROWS
        assert not T[:B].any() and all(T[B + 16 * k:B + 16 * k + 16].all() == (k % 2 == 0) for k in range(8) if B + 16 * k < case.n)
        assert case.n < B + 7 * 128 or (not T[B + 6 * 128:B + 7 * 128].any() and T[B + 5 * 128:B + 6 * 128].all() and T[B + 7 * 128:].all())
    if case.mask == "one_out":
        assert not T[-1] and T[:-1].all()


def test_the_case_list_is_the_one_asked_for():
    snp, dense = S.snp_cases(), S.dense_cases()
    one = [c for c in snp if c.m == 1]
    assert {(c.n, c.p) for c in one} == set(S.SNP_SHAPES) and len(S.SNP_SHAPES) == 17
    assert {c.n for c in one if c.p == 33} == set(S.SNP_N) and all({c.p for c in one if c.n == n} == set(S.SNP_P) for n in (129, 8320))
    assert {(17, 1), (17, 65), (16500, 1), (16500, 65)} <= set(S.SNP_SHAPES)
    for n, p in S.SNP_SHAPES:
        assert {c.mask for c in one if (c.n, c.p) == (n, p)} == set(S.SNP_MASKS) - (set() if n > S.COUNT_BLOCK_ROWS else {"blocks"})
    for mask in S.SNP_MASKS:
        assert {c.flags for c in snp if c.mask == mask} == set(A.EDGE_FLAGS) and {c.missing for c in snp if c.mask == mask} == set(S.SNP_MISSING)
    assert {(c.n, c.p, c.m) for c in snp if c.m > 1} == {(n, p, m) for n, p in S.TRAIT_SHAPES for m in S.TRAIT_M}
    assert [c for c in snp if c.one_training_row] and all(c.n == 8193 for c in snp if c.one_training_row)
    assert {(c.kind, c.n, c.m, c.mask) for c in dense} == {(k, n, m, mk) for k in S.DENSE_KINDS for n in S.DENSE_N for m in (1, 3) for mk in ("all", "random80")}
    assert all(c.p == 5 for c in dense) and len({c.id for c in snp + dense}) == len(snp + dense)
