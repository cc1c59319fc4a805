"""The SNP correlation band, its pair list and the LD pruning on the device (csrc/ld.hip: mih_ld_band, mih_ld_pairs,
mih_ld_prune; ld, ld_pairs and ld_prune of SnpLinAlg) against the numpy statement tests/ld_spec.py.

The integer statistics D_jk, A_jk, A_kj, M_jk and D_jj are compared exactly.  Tolerance of r, derived and not measured
(ld_spec.bound, u = 2^-53): each of C's terms is a few roundings away from exact integers, |dC_jk| <= c u T_jk with T the sum of
the terms' magnitudes and c = 8 from the count of the roundings of the spec's expression, so
    |dr| <= c u T_jk / sqrt(C_jj C_kk) + |r| c u (T_jj / C_jj + T_kk / C_kk) + 4 u |r|,
doubled because the numpy side rounds too.  Pair lists and masks are compared exactly: tests/test_ld_spec_cpu.py asserts that
no band pair of these inputs has r^2 within 1e-9 of a threshold used here, orders of magnitude above the bound.

The shapes are those where the kernels change path: one sample, the 16 rows of a dword of the 2-bit image, the 64 rows of one
matrix-core step and the 128 of a tile, several tiles and -- with slice_rows 128 and 256 -- several row slices; column counts
around the 32 of a column group with one, two, three, four and five groups; windows that stay inside a group, reach the next
one by a column, span whole groups, or exceed the matrix; panels of one and two groups against up to five."""
import ctypes as C
import re

import numpy as np
import pytest

import ld_spec as S
from conftest import free_device_bytes
from test_gpu_hardcall_pack import edge_codes, from_bed

from mendeliht_amd import api

pytestmark = pytest.mark.gpu

BAD_ARG = 2
VARIANTS = [(0, 0), (32, 0), (64, 0), (0, 128), (0, 256), (32, 128), (64, 256)]      # (panel_cols, slice_rows)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def last_error(mih):
    buf = C.create_string_buffer(512)
    mih.lib().mih_last_error(buf, 512)
    return buf.value.decode(errors="replace")


# ---- 1. edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", S.EDGE_P)
def test_edge_shapes(mih, p):
    cases = [c for c in S.edge_cases() if c[1] == p]
    assert len(cases) >= len(S.EDGE_W)
    equal = total = 0
    for n, p, window, missing, seed in cases:
        what = (n, p, window, missing)
        codes = S.planted(n, p, seed, missing)
        x = from_bed(mih, codes)
        v = np.random.default_rng(seed).standard_normal(n)
        before = x.xtv(v)
        want_st, want_diag = S.stats(codes, window)
        want, tol = S.r(codes, window, want_st), S.bound(codes, window, want_st)
        r, st, diag = x.ld(window, stats=True)
        assert st.shape == want_st.shape and np.array_equal(st, want_st), what              # exact integers
        assert np.array_equal(diag, want_diag), what
        S.check(r, want, tol, what)
        ok = ~np.isnan(want)
        equal, total = equal + int((r[ok] == want[ok]).sum()), total + int(ok.sum())
        assert bits(x.ld(window)) == bits(r), what                                          # a second call, and without stats
        for pc, sr in VARIANTS[1:]:
            r2, st2, diag2 = x.ld(window, stats=True, panel_cols=pc, slice_rows=sr)
            assert bits(r2) == bits(r) and bits(st2) == bits(st) and bits(diag2) == bits(diag), what + (pc, sr)
        assert bits(x.xtv(v)) == bits(before), what                                         # the source is only read
    print(f"ld p={p}: {equal} of {total} r bit-equal to the numpy statement")


# ---- 2. the slice rule --------------------------------------------------------------------------------------------------------
def test_more_rows_than_one_f32_accumulator_may_cover(mih):
    """n = 2^22 + 129, p = 33: every genotype is 2 except one column of 1s, a few missing entries, and ONE genotype 1 that
    columns 1 and 2 share in row 2^22 + 5.  D_jk is 4 n minus the missing rows, exactly; for the pair (1, 2) it is 4 n - 3, an
    accumulator value of 2^22 + 128.25, which f32 cannot hold (its spacing there is 1/2): a slice longer than 2^22 rows gets
    this integer wrong.  slice_rows = 2^22 really is two slices, the second of 129 rows; 2^22 + 128 and 2^23 must be taken as
    2^22 (the header's rule); the library's own rule runs 1025 slices of 4096 rows at this shape, because four (group,
    partner) items are too few work for the device.  All four give the same integers and the same bits of r."""
    n, p, one, shared = (1 << 22) + 129, 33, 20, (1 << 22) + 5
    base = np.full(p, 2, dtype=np.int64)
    base[one] = 1
    exc = {j: {} for j in range(p)}                                # column -> {row: genotype, -1 = missing}
    for j, rows in {0: [0, 5, n - 1], 7: [5, 1 << 22, (1 << 22) + 128], one: [4, n - 1], 32: [(1 << 22) - 1, 1 << 22]}.items():
        exc[j].update({i: -1 for i in rows})
    exc[1][shared] = exc[2][shared] = 1
    stride = (n + 3) // 4
    bed = np.full((p, stride), 0xFF, dtype=np.uint8)               # .bed code 11: two copies
    bed[one] = 0xAA                                                # code 10: one copy
    bed[:, -1] &= (1 << (2 * (n - 4 * (stride - 1)))) - 1          # the pad rows of the last byte
    for j in range(p):
        for i, g in exc[j].items():
            code = 1 if g < 0 else 2                               # code 01: missing, 10: one copy
            bed[j, i // 4] = (int(bed[j, i // 4]) & (0xFF ^ (3 << (2 * (i % 4))))) | (code << (2 * (i % 4)))
    x = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)

    def t(j, i):                                                   # the tile code: the genotype, 0 where missing
        return max(int(exc[j].get(i, base[j])), 0)
    miss = [{i for i, g in exc[j].items() if g < 0} for j in range(p)]
    s = np.array([base[j] * (n - len(exc[j])) + sum(t(j, i) for i in exc[j]) for j in range(p)], dtype=np.int64)
    m = np.array([len(miss[j]) for j in range(p)], dtype=np.int64)
    d = np.array([base[j] ** 2 * (n - len(exc[j])) + sum(t(j, i) ** 2 for i in exc[j]) for j in range(p)], dtype=np.int64)
    want_st = np.zeros((p, p - 1, 4), dtype=np.int64)
    for j in range(p):
        for k in range(j + 1, p):
            rows = set(exc[j]) | set(exc[k])
            want_st[j, k - j - 1] = [base[j] * base[k] * (n - len(rows)) + sum(t(j, i) * t(k, i) for i in rows),
                                     sum(t(k, i) for i in miss[j]), sum(t(j, i) for i in miss[k]), len(miss[j] & miss[k])]
    assert want_st[1, 0, 0] == 4 * n - 3 and want_st[3, 0, 0] == 4 * n and want_st[0, 6, 0] == 4 * (n - 4)
    assert float(np.float32(want_st[1, 0, 0] / 4.0)) != want_st[1, 0, 0] / 4.0        # f32 cannot hold this sum ...
    assert float(np.float32(want_st[3, 0, 0] / 4.0)) == want_st[3, 0, 0] / 4.0        # ... as it can the all-2 pairs'
    want, tol = S.r((n, s, m, d), p, want_st), S.bound((n, s, m, d), p, want_st)
    assert np.count_nonzero(want[~np.isnan(want)]) == 1 and want[1, 0] > 0.9           # columns 1 and 2 alone are polymorphic
    first = None
    for slice_rows in (1 << 22, (1 << 22) + 128, 1 << 23, 0):
        r, st, diag = x.ld(p, stats=True, slice_rows=slice_rows)
        assert np.array_equal(st, want_st), (slice_rows, np.argwhere(st != want_st)[:4].tolist())
        assert np.array_equal(diag, d), slice_rows
        S.check(r, want, tol, slice_rows)
        first = r if first is None else first
        assert bits(r) == bits(first), slice_rows


# ---- 3. the pair list ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def list_inputs(mih):
    out = []
    for n, p, missing, seed in S.list_cases():
        codes = S.planted(n, p, seed, missing)
        out.append((codes, from_bed(mih, codes)))
    return out


def test_pair_lists_are_the_specs_in_order(mih, list_inputs):
    for codes, x in list_inputs:
        p = codes.shape[1]
        for w in S.PAIR_WINDOWS:
            window = S.window_of(w, p)
            want_r = S.r(codes, window)
            band = x.ld(window)
            for thr in S.THRESHOLDS:
                what = (codes.shape, window, thr)
                wj, wk = S.pairs(want_r, thr)
                j, k, r = x.ld_pairs(window, thr)
                assert np.array_equal(j, wj) and np.array_equal(k, wk), what
                assert bits(r) == bits(band[j, k - j - 1]), what                  # the entries of ld(), bit for bit
                for pc, sr in VARIANTS[1:4]:
                    again = x.ld_pairs(window, thr, panel_cols=pc, slice_rows=sr)
                    assert all(bits(a) == bits(b) for a, b in zip(again, (j, k, r))), what + (pc, sr)


def test_cap_cuts_the_list_and_reports_the_full_count(mih, list_inputs, monkeypatch):
    codes, x = list_inputs[0]
    thr = S.THRESHOLDS[0]
    full = x.ld_pairs(33, thr)
    total = full[0].size
    assert total > 8
    cj, ck, cr = np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int64), np.full(4, -7.0)
    count = C.c_int64(-1)
    L = mih.lib()
    assert L.mih_ld_pairs(x._h, 33, thr, 32, 0, 1, ptr(cj), ptr(ck), ptr(cr), C.byref(count)) == 0 and count.value == total
    assert (cj[0], ck[0]) == (full[0][0], full[1][0]) and cr[0] == full[2][0]
    assert np.all(cj[1:] == -7) and np.all(ck[1:] == -7) and np.all(cr[1:] == -7.0)          # nothing beyond cap is written
    count = C.c_int64(-1)
    assert L.mih_ld_pairs(x._h, 33, thr, 0, 0, 0, None, None, None, C.byref(count)) == 0 and count.value == total
    for cap in (3, total - 1, total, total + 5):
        for pc in (0, 32):                                                                   # a cut inside a later panel, too
            got = x.ld_pairs(33, thr, cap=cap, panel_cols=pc)
            assert all(bits(a) == bits(b[:cap]) for a, b in zip(got, full)), (cap, pc)
    monkeypatch.setattr(api, "_ld_first_room", lambda p: 2)          # cap = None with a first room that is too small
    got = x.ld_pairs(33, thr)
    assert all(bits(a) == bits(b) and a.shape == b.shape for a, b in zip(got, full))


# ---- 4. pruning ---------------------------------------------------------------------------------------------------------------
def test_prune_masks_are_the_specs(mih, list_inputs):
    for codes, x in list_inputs:
        p = codes.shape[1]
        for window, step in S.PRUNE_SHAPES:
            window, step = S.window_of(window, p), S.window_of(step, p)
            rband = S.r(codes, window)
            for thr in S.THRESHOLDS:
                want = S.prune(codes, window, step, thr, rband)
                keep = x.ld_prune(window, step, thr)
                assert keep.dtype == np.bool_ and np.array_equal(keep, want), (codes.shape, window, step, thr)
                assert np.array_equal(x.ld_prune(window, step, thr, panel_cols=32, slice_rows=128), want)
        keep = x.ld_prune(50, 5, S.THRESHOLDS[0])
        phi = x.grm(cols=keep)                                       # the pipeline step: the mask goes where cols= goes
        assert phi.shape == (x.n, x.n) and np.all(np.isfinite(phi))
        count = C.c_int64(-1)
        kp = np.full(p, 7, dtype=np.uint8)
        assert mih.lib().mih_ld_prune(x._h, 50, 5, S.THRESHOLDS[0], 0, 0, ptr(kp), C.byref(count)) == 0
        assert np.array_equal(kp.astype(bool), keep) and count.value == x.ld_pairs(50, S.THRESHOLDS[0])[0].size


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(mih):
    L = mih.lib()
    codes = edge_codes(17, 5, 1)
    x = from_bed(mih, codes)
    dense = mih.DenseMatrix(np.random.default_rng(0).standard_normal((17, 5)))
    dosage = mih.DosageMatrix(np.where(codes < 0, 0xFFFF, codes).astype(np.uint16), 2)
    r, st, dg = np.full((5, 4), -7.0), np.full((5, 4, 4), -7, dtype=np.int64), np.full(5, -7, dtype=np.int64)
    cj, ck, cr = np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int64), np.full(4, -7.0)
    keep = np.full(5, 7, dtype=np.uint8)
    count = C.c_int64(-7)

    calls = [("band dense", lambda: L.mih_ld_band(dense._h, 5, 0, 0, ptr(r), ptr(st), ptr(dg))),
             ("band dosage", lambda: L.mih_ld_band(dosage._h, 5, 0, 0, ptr(r), ptr(st), ptr(dg))),
             ("band null handle", lambda: L.mih_ld_band(None, 5, 0, 0, ptr(r), ptr(st), ptr(dg))),
             ("band window", lambda: L.mih_ld_band(x._h, 1, 0, 0, ptr(r), ptr(st), ptr(dg))),
             ("band null", lambda: L.mih_ld_band(x._h, 5, 0, 0, None, ptr(st), ptr(dg))),
             ("pairs dense", lambda: L.mih_ld_pairs(dense._h, 5, 0.2, 0, 0, 4, ptr(cj), ptr(ck), ptr(cr), C.byref(count))),
             ("pairs window", lambda: L.mih_ld_pairs(x._h, 0, 0.2, 0, 0, 4, ptr(cj), ptr(ck), ptr(cr), C.byref(count))),
             ("pairs nan", lambda: L.mih_ld_pairs(x._h, 5, float("nan"), 0, 0, 4, ptr(cj), ptr(ck), ptr(cr), C.byref(count))),
             ("pairs cap", lambda: L.mih_ld_pairs(x._h, 5, 0.2, 0, 0, -1, ptr(cj), ptr(ck), ptr(cr), C.byref(count))),
             ("pairs null list", lambda: L.mih_ld_pairs(x._h, 5, 0.2, 0, 0, 4, ptr(cj), None, ptr(cr), C.byref(count))),
             ("pairs null count", lambda: L.mih_ld_pairs(x._h, 5, 0.2, 0, 0, 4, ptr(cj), ptr(ck), ptr(cr), None)),
             ("prune dense", lambda: L.mih_ld_prune(dense._h, 5, 1, 0.2, 0, 0, ptr(keep), C.byref(count))),
             ("prune window", lambda: L.mih_ld_prune(x._h, 1, 1, 0.2, 0, 0, ptr(keep), C.byref(count))),
             ("prune step", lambda: L.mih_ld_prune(x._h, 5, 0, 0.2, 0, 0, ptr(keep), C.byref(count))),
             ("prune nan", lambda: L.mih_ld_prune(x._h, 5, 1, float("nan"), 0, 0, ptr(keep), C.byref(count))),
             ("prune null", lambda: L.mih_ld_prune(x._h, 5, 1, 0.2, 0, 0, None, C.byref(count)))]
    before = free_device_bytes()
    for what, call in calls:
        assert call() == BAD_ARG and last_error(mih), what
        assert np.all(r == -7.0) and np.all(st == -7) and np.all(dg == -7), what
        assert np.all(cj == -7) and np.all(ck == -7) and np.all(cr == -7.0) and np.all(keep == 7) and count.value == -7, what
    assert abs(free_device_bytes() - before) <= 64 << 20
    for call in (lambda: x.ld(1), lambda: x.ld_pairs(5, float("nan")), lambda: x.ld_pairs(5, 0.2, cap=-1),
                 lambda: x.ld_prune(5, 0, 0.2), lambda: x.ld_prune(1, 1, 0.2), lambda: x.ld_prune(5, 1, float("nan"))):
        with pytest.raises(api.ArgumentError):
            call()
    assert not hasattr(dosage, "ld") and not hasattr(dense, "ld_prune")
    want = S.r(codes, 5)
    S.check(x.ld(5), want, S.bound(codes, 5), "after the refusals")   # and the handle still serves


def test_a_band_the_device_cannot_hold_is_refused_before_anything_is_allocated(mih):
    x = mih.SnpLinAlg.synthetic(128, 200_000)
    before = free_device_bytes()
    with pytest.raises(MemoryError) as e:
        x.ld_pairs(200_000, 0.5, panel_cols=200_000)                 # one panel of 4e10 band entries
    need, free = (int(v) for v in re.findall(r"(\d{9,}) bytes", str(e.value)))
    assert need >= 8 * 200_000 * 199_999 and need > free and abs(free - before) <= 64 << 20
    assert abs(free_device_bytes() - before) <= 64 << 20
    keep = x.ld_prune(50, 5, 0.2)                                    # and with the library's panels the same matrix is served
    assert keep.shape == (200_000,) and keep.any()
