"""The numpy statement of `filter` (tests/qc_spec.py) on the crafted matrix: the thresholds are float64 products compared with
`<`, and the counts of a round are taken before either mask changes.  An implementation that rounds the thresholds, uses `<=`
or updates one mask before counting for the other gives other answers here (no GPU needed)."""
import numpy as np

import qc_spec as Q


def dropped(mask):
    return list(np.flatnonzero(~mask))


def test_thresholds_are_the_float64_products():
    assert (1 - 0.98) * 200 > 4 and (1 - 0.98) * 1000 > 20           # 4.0000000000000036, 20.000000000000018
    assert 20 >= (1 - 0.98) * 900 and 4 >= (1 - 0.98) * 178           # 18.000000000000014, 3.56...


def test_counts_statement():
    codes = Q.crafted_codes()
    cc, rm = Q.counts(codes)
    assert cc.dtype == np.int32 and rm.dtype == np.int32
    assert np.array_equal(cc.sum(axis=1), np.full(200, 1000))
    assert cc[50, 3] == 20 and rm[500] == 4 and np.all(rm[:100] == 20)
    assert list(cc[90]) == [1000, 0, 0, 0] and list(cc[91]) == [997, 3, 0, 0]
    rows = np.arange(100, 1000)
    cc, rm = Q.counts(codes, rows, np.arange(200) != 50)
    assert np.all(cc[:20, 3] == 0) and list(cc[50]) == [0, 0, 0, 0] and rm[500] == 3 and np.all(rm[:100] == 0)
    assert np.array_equal(cc.sum(axis=1), np.where(np.arange(200) == 50, 0, 900))


def test_defaults_converge_in_three_rounds():
    codes = Q.crafted_codes()
    rmask, cmask, rounds, converged = Q.filter(codes)
    assert converged and rounds == 3
    assert dropped(rmask) == list(range(100)) + [500]
    assert dropped(cmask) == list(range(20)) + [50, 90, 91]
    # round 1 alone keeps row 500 (4 < 4.0000000000000036) and column 50 (20 < 20.000000000000018); both fall in round 2
    r1, c1, _, conv1 = Q.filter(codes, maxiters=1)
    assert not conv1 and dropped(r1) == list(range(100)) and dropped(c1) == list(range(20)) + [90, 91]


def test_maxiters_two_is_not_converged():
    codes = Q.crafted_codes()
    rmask, cmask, rounds, converged = Q.filter(codes, maxiters=2)
    assert not converged and rounds == 2
    assert (~rmask).sum() == 101 and (~cmask).sum() == 23
    full = Q.filter(codes)
    assert np.array_equal(rmask, full[0]) and np.array_equal(cmask, full[1])


def test_without_the_maf_test_the_monomorphic_columns_stay():
    codes = Q.crafted_codes()
    rmask, cmask, rounds, converged = Q.filter(codes, min_maf=0)
    assert converged and rounds == 3
    assert cmask[90] and cmask[91] and (~cmask).sum() == 21 and (~rmask).sum() == 101
