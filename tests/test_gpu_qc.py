"""Quality control and sample selection on the 2-bit matrix (csrc/qc.hip: mih_snp_counts, mih_snp_subset; SnpLinAlg.counts, maf,
missing_rate, subset, filter).  Everything is exact: counts are integers and equal the numpy statement (tests/qc_spec.py); a
subset equals, bit for bit, the handle mih_snp_create builds from the .bed encoding of codes[rows][:, cols] -- export_bed, mu and
sinv, X'r single and fused, X v, one fit.  The shapes are those where the kernels change path: the dword (16 rows), the half
record (64), the tile (128), a wave's four tiles (512), a workgroup's 64 (8192), the group of 32 columns, result dwords that
straddle source dwords and tiles, and a sparse selection whose result tile spans hundreds of source tiles."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import qc_spec as Q
from conftest import GOLD
from test_gpu_hardcall_pack import assert_same_handle, bed_of, codes_of, edge_codes, from_bed

from mendeliht_amd import genotypes as G

pytestmark = pytest.mark.gpu

EDGE_N = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 8191, 8193]
_SOURCES = {}


def source(mih, n, p):
    """edge_codes(n, p) and its handle, built once per shape and never changed."""
    if (n, p) not in _SOURCES:
        codes = edge_codes(n, p, 7000 * n + p)
        codes.setflags(write=False)
        _SOURCES[(n, p)] = (codes, from_bed(mih, codes))
    return _SOURCES[(n, p)]


def check_subset(mih, x, codes, rows=None, cols=None, fit=False):
    want = codes if rows is None else codes[rows]
    want = want if cols is None else want[:, cols]
    got = x.subset(rows, cols)
    assert_same_handle(mih, got, from_bed(mih, want), fit=fit and want.shape[0] >= 257)
    return got


# ---- 1. counts at edge shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_counts_at_edge_shapes(mih, n):
    for p in (1, 31, 32, 33, 70):
        codes, x = source(mih, n, p)
        rng = np.random.default_rng(n * 97 + p)
        every = np.ones(n, dtype=bool)
        single = np.zeros(n, dtype=bool)
        single[n // 2] = True
        ends = every.copy()
        ends[[0, n - 1]] = False
        row_masks = [None, every, single, np.arange(n) % 2 == 0, rng.random(n) < 0.5, ends]
        col_masks = [None] * len(row_masks)
        col_masks[4] = rng.random(p) < 0.5
        if p > 32:
            row_masks += [None, rng.random(n) < 0.5]
            col_masks += [np.arange(p) == 32] * 2
        for rm, cm in zip(row_masks, col_masks):
            cc, miss = x.counts(rm, cm)
            want_cc, want_miss = Q.counts(codes, rm, cm)
            assert cc.dtype == np.int32 and cc.shape == (p, 4) and miss.dtype == np.int32 and miss.shape == (n,)
            assert np.array_equal(cc, want_cc), (n, p)
            assert np.array_equal(miss, want_miss), (n, p)
            if cm is not None:
                assert not cc[~cm].any()
            if rm is not None:
                assert not miss[~rm].any()
        # index arrays name the same selections as masks
        idx = np.flatnonzero(row_masks[4])
        a, b = x.counts(idx, None), Q.counts(codes, row_masks[4], None)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(x.maf(), Q.maf(Q.counts(codes)[0]), equal_nan=True)
        assert np.array_equal(x.maf(rows=row_masks[3]), Q.maf(Q.counts(codes, row_masks[3])[0]), equal_nan=True)
        assert np.array_equal(x.missing_rate(0), (codes < 0).sum(axis=0) / float(n))
        assert np.array_equal(x.missing_rate(1), (codes < 0).sum(axis=1) / float(p))
    if n >= 127:
        assert np.isnan(x.maf()[68]) and x.maf()[3] == 0.0                 # edge_codes' all-missing and monomorphic columns


# ---- 2. subset equals the matrix built from the filtered .bed ---------------------------------------------------------------------
def row_selections(n, rng):
    sels = [("all", np.arange(n)), ("one", np.array([n // 2])), ("every other", np.arange(0, n, 2))]
    if n > 1:
        sels += [("drop first", np.arange(1, n)), ("drop last", np.arange(n - 1)), ("every third", np.arange(1, n, 3)),
                 ("random half", np.flatnonzero(rng.random(n) < 0.5))]
    sels += [(f"block {m}", np.arange(5, 5 + m)) for m in (16, 64, 128, 129) if 5 + m <= n]
    return [(name, r) for name, r in sels if r.size]


@pytest.mark.parametrize("n", EDGE_N + [2047, 2049])
def test_subset_equals_the_filtered_bed(mih, n):
    p = 70
    codes, x = source(mih, n, p)
    rng = np.random.default_rng(n)
    col_sels = [None, np.arange(1, p), np.array([33]), np.flatnonzero(rng.random(p) < 0.5)]
    col_sels += [np.sort(rng.choice(p, w, replace=False)) for w in (31, 32, 33)]
    assert_same_handle(mih, x.subset(), x)                                  # everything: the source itself
    assert_same_handle(mih, x.subset(np.ones(n, dtype=bool), np.arange(p)), x)
    for c in col_sels[1:]:                                                  # columns only
        check_subset(mih, x, codes, None, c)
    for k, (name, r) in enumerate(row_selections(n, rng)):
        check_subset(mih, x, codes, r, None, fit=name == "random half")      # rows only
        check_subset(mih, x, codes, r, col_sels[1 + k % (len(col_sels) - 1)], fit=name == "every other")   # both together
    mask = np.zeros(n, dtype=bool)
    mask[::2] = True
    assert_same_handle(mih, x.subset(mask), x.subset(np.flatnonzero(mask)))  # a mask names the same selection


@pytest.mark.parametrize("p", [1, 31, 32, 33])
def test_subset_of_narrow_sources(mih, p):
    for n in (129, 257):
        codes, x = source(mih, n, p)
        rng = np.random.default_rng(n + p)
        check_subset(mih, x, codes, np.flatnonzero(rng.random(n) < 0.5), None)
        check_subset(mih, x, codes, np.arange(1, n, 3), np.arange(p)[p // 2:])
        check_subset(mih, x, codes, None, np.arange(p)[: max(1, p - 1)])


@pytest.mark.parametrize("n", [257, 2049])
def test_subset_result_heights_around_the_dword_and_the_tile(mih, n):
    codes, x = source(mih, n, 70)
    rng = np.random.default_rng(n + 1)
    for n_out in (15, 16, 17, 127, 128, 129):
        r = np.sort(rng.choice(n, n_out, replace=False))
        check_subset(mih, x, codes, r, None)
        check_subset(mih, x, codes, r, np.sort(rng.choice(70, 33, replace=False)))


def test_subset_sparse_rows_span_many_source_tiles(mih):
    """One row in 300 of 40 000: a result tile of 128 rows spans 300 source tiles per column group."""
    codes, x = source(mih, 40_000, 70)
    rng = np.random.default_rng(300)
    r = np.arange(7, 40_000, 300)
    check_subset(mih, x, codes, r, None)
    check_subset(mih, x, codes, r, np.flatnonzero(rng.random(70) < 0.5))
    check_subset(mih, x, codes, np.sort(rng.choice(40_000, 300, replace=False)), np.arange(1, 70), fit=True)


def test_subset_leaves_a_kept_column_all_missing(mih):
    codes = np.array(source(mih, 257, 70)[0])
    codes[3:, 40] = -1                                         # column 40 has genotypes in rows 0, 1, 2 only
    codes[:3, 40] = [0, 1, 2]
    codes[96:112, 41] = -1                                     # sixteen missing rows that fill a source dword and, once three
    codes[113:116, 41] = -1                                    # rows are dropped, straddle two result dwords
    x = from_bed(mih, codes)
    r = np.arange(3, 257)
    got = check_subset(mih, x, codes, r, None, fit=False)
    cc = got.counts()[0]
    assert list(cc[40]) == [0, 0, 0, 254] and np.isnan(got.mu_sigma()[0][40]) and cc[41, 3] >= 19
    check_subset(mih, x, codes, r, np.arange(35, 45))
    check_subset(mih, x, codes, np.arange(0, 257, 2), np.array([40, 41]))


# ---- 3. the source is untouched -------------------------------------------------------------------------------------------------
def test_source_is_untouched(mih):
    codes = edge_codes(513, 70, 11)
    x = from_bed(mih, codes)
    r = np.random.default_rng(2).standard_normal(513)
    before = (x.export_bed(), x.mu_sigma(), x.xtv(r), x.counts())
    rng = np.random.default_rng(3)
    sub = x.subset(rng.random(513) < 0.5, rng.random(70) < 0.5)

    def same():
        after = (x.export_bed(), x.mu_sigma(), x.xtv(r), x.counts())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2], equal_nan=True)
        for a, b in zip(before[1] + before[3], after[1] + after[3]):
            assert np.array_equal(a, b, equal_nan=True)
    same()
    sub.xtv(np.ones(sub.n))
    del sub
    same()
    assert x.shape == (513, 70)


# ---- 4. subset of a subset ---------------------------------------------------------------------------------------------------------
def test_subset_of_a_subset(mih):
    codes, x = source(mih, 2049, 70)
    rng = np.random.default_rng(4)
    r1, c1 = np.flatnonzero(rng.random(2049) < 0.7), np.flatnonzero(rng.random(70) < 0.8)
    r2, c2 = np.flatnonzero(rng.random(r1.size) < 0.6), np.flatnonzero(rng.random(c1.size) < 0.6)
    twice, once = x.subset(r1, c1).subset(r2, c2), x.subset(r1[r2], c1[c2])
    assert_same_handle(mih, twice, once, fit=True)
    assert_same_handle(mih, once, from_bed(mih, codes[r1[r2]][:, c1[c2]]))


# ---- 5. flags -------------------------------------------------------------------------------------------------------------------
def test_flags(mih):
    codes = edge_codes(300, 40, 12)
    rng = np.random.default_rng(5)
    r, c = np.flatnonzero(rng.random(300) < 0.5), np.flatnonzero(rng.random(40) < 0.5)
    bed = bed_of(codes[r][:, c])
    x = from_bed(mih, codes)
    for kw in (dict(center=False, scale=False), dict(dtype=np.float32), dict(center=True, scale=False, impute=False, dtype=np.float32)):
        got = x.subset(r, c, **kw)
        flags = dict(center=x.center, scale=x.scale, impute=x.impute, dtype=x.dtype)
        flags.update(kw)
        want = mih.SnpLinAlg(bed, r.size, **flags)
        assert got.dtype is want.dtype
        assert_same_handle(mih, got, want, fit=True)
    plain = mih.SnpLinAlg(bed_of(codes), 300, center=False, scale=True, impute=False, dtype=np.float32)
    got = plain.subset(r, c)                                   # the default inherits the source's flags
    assert (got.center, got.scale, got.impute, got.dtype) == (False, True, False, np.float32)
    assert_same_handle(mih, got, mih.SnpLinAlg(bed, r.size, center=False, scale=True, impute=False, dtype=np.float32))
    assert_same_handle(mih, x.subset(r, c, reserve=True), from_bed(mih, codes[r][:, c]))


# ---- 6. filter -------------------------------------------------------------------------------------------------------------------
def test_filter_on_the_crafted_matrix(mih):
    codes = Q.crafted_codes()
    x = from_bed(mih, codes)
    want = Q.filter(codes)
    assert want[2:] == (3, True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rmask, cmask = x.filter()
    assert rmask.dtype == bool and cmask.dtype == bool
    assert np.array_equal(rmask, want[0]) and np.array_equal(cmask, want[1])
    assert list(np.flatnonzero(~rmask)) == list(range(100)) + [500]
    assert list(np.flatnonzero(~cmask)) == list(range(20)) + [50, 90, 91]
    with pytest.warns(UserWarning, match="success rates"):
        r2, c2 = x.filter(maxiters=2)
    assert np.array_equal(r2, want[0]) and np.array_equal(c2, want[1])
    with pytest.warns(UserWarning):
        r1, c1 = x.filter(maxiters=1)
    w1 = Q.filter(codes, maxiters=1)
    assert np.array_equal(r1, w1[0]) and np.array_equal(c1, w1[1]) and r1[500] and c1[50]
    r0, c0 = x.filter(min_maf=0)
    w0 = Q.filter(codes, min_maf=0)
    assert np.array_equal(r0, w0[0]) and np.array_equal(c0, w0[1]) and c0[90] and c0[91] and (~c0).sum() == 21
    sub = x.subset(rmask, cmask)
    assert sub.shape == (899, 177)
    assert_same_handle(mih, sub, from_bed(mih, codes[rmask][:, cmask]), fit=True)
    again = sub.filter()                                       # what is left satisfies the rates
    assert again[0].all() and again[1].all()


@pytest.mark.parametrize("rate", [0.01, 0.05, 0.20])
def test_filter_on_random_matrices(mih, rate):
    from conftest import make_bed
    n, p = 513, 70
    rng = np.random.default_rng(int(rate * 1000))
    codes = codes_of(make_bed(rng, n, p, missing_rate=rate), n)
    extra = rng.random(n) < 0.1                                # some rows and columns are worse than the rest
    codes[np.ix_(extra, rng.random(p) < 0.3)] = -1
    x = from_bed(mih, codes)
    for kw in ({}, dict(min_success_rate_per_row=0.9, min_success_rate_per_col=0.93, min_maf=0.05), dict(min_maf=0, maxiters=20),
               dict(min_success_rate_per_row=0.7, min_success_rate_per_col=0.75, min_maf=0.02, maxiters=2)):
        want = Q.filter(codes, **kw)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            rmask, cmask = x.filter(**kw)
        assert np.array_equal(rmask, want[0]) and np.array_equal(cmask, want[1]), (rate, kw)
        assert any(issubclass(w.category, UserWarning) for w in caught) == (not want[3])
        if rmask.any() and cmask.any():
            sub = x.subset(rmask, cmask)
            assert sub.shape == (rmask.sum(), cmask.sum())
            y = np.random.default_rng(1).standard_normal(sub.n)
            mih.fit_iht(y, sub, None, k=min(3, sub.p), verbose=False)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(mih):
    codes, x = source(mih, 257, 70)
    n, p = x.shape
    E, D = mih.api.ArgumentError, mih.api.DimensionMismatch

    def still_works():
        assert np.array_equal(x.counts()[0], Q.counts(codes)[0])
        check_subset(mih, x, codes, np.arange(1, n, 3), np.array([33]))

    for call in (lambda: x.subset(np.ones(n + 1, dtype=bool)), lambda: x.subset(None, np.ones(p - 1, dtype=bool)),
                 lambda: x.counts(np.ones(n - 1, dtype=bool)), lambda: x.counts(None, np.ones(p + 1, dtype=bool)),
                 lambda: x.maf(rows=np.ones(n + 3, dtype=bool))):
        with pytest.raises(D, match="mask"):
            call()
    still_works()
    for call, word in ((lambda: x.subset(np.zeros(n, dtype=bool)), "empty"), (lambda: x.subset(None, np.array([], dtype=np.int64)), "empty"),
                       (lambda: x.subset(np.array([5, 4, 9])), "increasing"), (lambda: x.subset(None, np.array([5, 4, 9])), "increasing"),
                       (lambda: x.subset(np.array([4, 5, 5])), "increasing"), (lambda: x.subset(np.array([0, n])), "outside"),
                       (lambda: x.subset(None, np.array([p])), "outside"), (lambda: x.subset(np.array([-1, 3])), "outside"),
                       (lambda: x.counts(np.array([5, 4])), "increasing"), (lambda: x.counts(None, np.array([p])), "outside")):
        with pytest.raises(E, match=word):
            call()
        still_works()
    # the C entry points refuse the same selections, and any handle that is not 2-bit
    L = mih.lib()

    def last_error():
        buf = C.create_string_buffer(512)
        L.mih_last_error(buf, 512)
        return buf.value.decode()

    def i64(a):
        return np.ascontiguousarray(a, dtype=np.int64)

    out = C.c_void_p(None)
    for rows, cols, word in ((i64([3, 2]), None, "increasing"), (i64([2, 2]), None, "increasing"), (i64([n]), None, "outside"),
                             (None, i64([0, p]), "outside"), (i64([1]), i64([1, 1]), "increasing")):
        rc = L.mih_snp_subset(x._h, None if rows is None else rows.ctypes.data_as(C.c_void_p), 0 if rows is None else rows.size,
                              None if cols is None else cols.ctypes.data_as(C.c_void_p), 0 if cols is None else cols.size, 1, 1, 1, 64, C.byref(out))
        assert rc == 2 and not out.value and word in last_error()
    one = i64([0])
    assert L.mih_snp_subset(x._h, one.ctypes.data_as(C.c_void_p), 0, None, 0, 1, 1, 1, 64, C.byref(out)) == 2 and "empty" in last_error()
    num = np.where(codes < 0, 0xFFFF, codes).astype(np.uint16)
    for other in (mih.DosageMatrix(num, 1), mih.DenseMatrix(np.where(codes < 0, 0, codes).astype(np.float64))):
        assert L.mih_snp_subset(other._h, None, 0, None, 0, 1, 1, 1, 64, C.byref(out)) == 2 and not out.value
        assert "2-bit" in last_error()
        cc = np.full((p, 4), -5, dtype=np.int32)
        assert L.mih_snp_counts(other._h, None, None, cc.ctypes.data_as(C.c_void_p), None) == 2 and "2-bit" in last_error()
        assert np.all(cc == -5)
        assert not hasattr(other, "subset") and not hasattr(other, "filter")
    still_works()


# ---- 8. from a streamed file ---------------------------------------------------------------------------------------------------------
def test_subset_of_a_streamed_vcf(mih):
    x = G.read_vcf_snp(os.path.join(GOLD, "normal_head.vcf.gz"))[0]
    n, p = x.shape
    codes = codes_of(x.export_bed(), n)
    assert_same_handle(mih, x, from_bed(mih, codes))
    rng = np.random.default_rng(8)
    r, c = np.flatnonzero(rng.random(n) < 0.5), np.flatnonzero(rng.random(p) < 0.5)
    check_subset(mih, x, codes, r, c, fit=True)
    cc, miss = x.counts(r, c)
    want = Q.counts(codes, r, c)
    assert np.array_equal(cc, want[0]) and np.array_equal(miss, want[1])
