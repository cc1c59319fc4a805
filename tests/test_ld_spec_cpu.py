"""tests/ld_spec.py against the definitions it states, without a device: the formula of r against the correlation of the
mean-imputed columns computed as such, the integer statistics against loops over their definitions, the properties of the
greedy pass, and the margin condition of the device tests -- no band pair of any input they use has r^2 within 1e-9 of a
threshold they use, so that a pair list or a mask can be compared exactly.  That is a condition on the inputs, not a tolerance:
no pair is excused.  (On these planted-LD inputs 0.2, 0.3 and 0.5 ARE hit exactly at n = 15 and n = 16, where r^2 is a small
rational number; 0.1999 and 0.4999 keep their distance at every shape.)"""
import os
import re

import numpy as np
import pytest

import ld_spec as S
from conftest import ROOT


def all_inputs():
    for n, p, window, missing, seed in S.edge_cases():
        yield S.planted(n, p, seed, missing), window
    for n, p, missing, seed in S.list_cases():
        codes = S.planted(n, p, seed, missing)
        for w in S.PAIR_WINDOWS:
            yield codes, S.window_of(w, p)


def test_the_case_list_covers_every_edge_value():
    cases = S.edge_cases()
    assert {c[0] for c in cases} == set(S.EDGE_N) and {c[1] for c in cases} == set(S.EDGE_P)
    assert {(c[1], c[2]) for c in cases} == {(p, S.window_of(w, p)) for p in S.EDGE_P for w in S.EDGE_W}
    assert sum(c[3] == 0.0 for c in cases) * 4 == len(cases)
    plain = [c for c in cases if c[3] == 0.0]                        # the one-product kernel meets every window and every p
    assert {c[1] for c in plain} == set(S.EDGE_P)
    assert {w for w in S.EDGE_W if any(c[2] == S.window_of(w, c[1]) for c in plain)} == set(S.EDGE_W)
    for miss in (True, False):                                       # several row slices with several panels, both kernels
        assert sum(1 for c in cases if c[0] >= 257 and c[1] >= 65 and (c[3] > 0) == miss) >= 3
    for n, p, window, missing, seed in cases:
        codes = S.planted(n, p, seed, missing)
        assert (codes < 0).any() == (missing > 0) or n * p < 200
        if p >= 31:
            deg = S.degenerate(codes)
            assert deg[3] and deg[17] and (missing == 0 or deg[p - 2])


def test_r_is_the_correlation_of_the_mean_imputed_columns():
    seen = 0
    for codes, window in all_inputs():
        got, want = S.r(codes, window), S.brute_r(codes, window)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12), (codes.shape, window, float(np.abs(got[ok] - want[ok]).max()))
        assert np.all(np.abs(got[ok]) <= 1.0 + 1e-12)
        seen += int(ok.sum())
    assert seen > 50_000


@pytest.mark.parametrize("case", [(17, 33, 34, 0.03, 1), (65, 5, 3, 0.2, 2), (16, 40, 50, 0.0, 3)])
def test_the_integer_statistics_are_their_definitions(case):
    n, p, window, missing, seed = case
    codes = S.planted(n, p, seed, missing)
    st, diag = S.stats(codes, window)
    w = min(window, p)
    assert st.shape == (p, w - 1, 4) and st.dtype == np.int64
    for j in range(p):
        assert diag[j] == sum(int(g) ** 2 for g in codes[:, j] if g >= 0)
        for d in range(1, w):
            k = j + d
            if k >= p:
                assert not st[j, d - 1].any()
                continue
            D = sum(int(a) * int(b) for a, b in zip(codes[:, j], codes[:, k]) if a >= 0 and b >= 0)
            Ajk = sum(int(b) for a, b in zip(codes[:, j], codes[:, k]) if a < 0 and b >= 0)
            Akj = sum(int(a) for a, b in zip(codes[:, j], codes[:, k]) if b < 0 and a >= 0)
            M = sum(1 for a, b in zip(codes[:, j], codes[:, k]) if a < 0 and b < 0)
            assert st[j, d - 1].tolist() == [D, Ajk, Akj, M], (j, k)


def test_the_bound_is_small_and_zero_only_where_r_is_exact():
    for codes, window in all_inputs():
        b, rb = S.bound(codes, window), S.r(codes, window)
        ok = ~np.isnan(rb)
        assert np.all(np.isfinite(b[ok])) and np.all(b[ok] < 1e-9), (codes.shape, window)
        assert np.all(rb[ok & (b == 0.0)] == 0.0)


@pytest.mark.parametrize("case", S.list_cases())
def test_prune(case):
    n, p, missing, seed = case
    codes = S.planted(n, p, seed, missing)
    deg = S.degenerate(codes)
    for window, step in S.PRUNE_SHAPES:
        window, step = S.window_of(window, p), S.window_of(step, p)
        rb = S.r(codes, window)
        for thr in S.THRESHOLDS:
            keep = S.prune(codes, window, step, thr)
            assert not keep[deg].any()                                           # every degenerate column is dropped
            w = min(window, p)
            for s in range(0, p, step):                                          # no pair above the threshold inside a window position
                kept = [j for j in range(s, min(s + w, p)) if keep[j]]
                for a, i in enumerate(kept):
                    for j in kept[a + 1:]:
                        assert not rb[i, j - i - 1] ** 2 > thr, (window, step, thr, i, j)
        keep = S.prune(codes, window, step, 1.0 + 1e-9)
        assert np.array_equal(keep, ~deg)                                         # nothing but the degenerate columns goes
        if not np.nanmax(rb * rb) > 1.0:                                          # (identical columns may round to 1 + an ulp)
            assert np.array_equal(S.prune(codes, window, step, 1.0), ~deg)
    some = S.prune(codes, 50, 5, S.THRESHOLDS[0])
    assert 0 < some.sum() < (~deg).sum()                                          # the planted runs are thinned, not emptied


def test_margin_condition_of_the_device_tests():
    """Every input and threshold tests/test_gpu_ld.py compares a list or a mask on: no band pair within 1e-9 of the threshold."""
    worst = np.inf
    for n, p, missing, seed in S.list_cases():
        codes = S.planted(n, p, seed, missing)
        windows = {S.window_of(w, p) for w in S.PAIR_WINDOWS} | {S.window_of(w, p) for w, _ in S.PRUNE_SHAPES}
        for window in sorted(windows):
            for thr in S.THRESHOLDS:
                m = S.min_margin(codes, window, thr)
                assert m >= S.MARGIN, (n, p, window, thr, m)
                worst = min(worst, m)
    assert worst >= 1e-9
    # and the reason for the two thresholds: the round ones are hit exactly by small rational r^2
    hit = [thr for thr in (0.2, 0.3, 0.5) for n in (15, 16) for seed in range(40)
           if S.min_margin(S.planted(n, 64, seed, 0.0), 64, thr) < S.MARGIN]
    assert hit


def test_pairs_are_in_order_and_strict():
    codes = S.planted(129, 150, 11, 0.03)
    rb = S.r(codes, 33)
    j, k = S.pairs(rb, S.THRESHOLDS[0])
    assert j.size > 20 and np.all(k > j) and np.all(k - j < 33)
    order = np.lexsort((k, j))
    assert np.array_equal(order, np.arange(j.size))
    v = rb[j, k - j - 1]
    assert np.all(v * v > S.THRESHOLDS[0])
    assert S.pairs(rb, float((v * v).max()))[0].size == 0                         # strictly greater


def test_header_binding_and_build_know_the_entry_points(mih):
    from mendeliht_amd import api
    header = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"^int\s+(mih_\w+)\s*\(", header, flags=re.M))
    for name in ("mih_ld_band", "mih_ld_pairs", "mih_ld_prune"):
        assert name in declared and name in api.exported_symbols()
    for name in ("ld", "ld_pairs", "ld_prune"):
        assert callable(getattr(api.SnpLinAlg, name)) and not hasattr(api.DosageMatrix, name)
    assert "ld.hip" in open(os.path.join(ROOT, "mendeliht.jl_amd", "csrc", "Makefile")).read()
