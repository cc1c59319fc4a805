"""SnpLinAlg.transpose (csrc/transpose.hip: mih_snp_transpose): the handle of the transposed genotypes equals, bit for bit, the
handle mih_snp_create builds from the .bed encoding of the transposed code matrix (tests/xb_spec.py: transpose_codes) -- the
exported codes (so the tiles, with missing genotypes and pads in place), mu and 1/sigma per sample, X'r single and fused and X v
(so the missing lists, whose order those sums follow).  The shapes are those where the kernel changes path: the dword (16), the
group of 32 columns, the tile (128 rows), the 128 x 128 block, one past each, group counts that are no multiple of 4, and one
image tall enough for its passes to cross a row slice."""
import numpy as np
import pytest

import xb_spec as S
from test_gpu_hardcall_pack import assert_same_handle, bed_of, edge_codes, from_bed

pytestmark = pytest.mark.gpu

EDGE_N = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257, 513]
EDGE_P = [1, 31, 32, 33, 127, 128, 129, 385]


def check_transpose(mih, codes, x=None):
    x = from_bed(mih, codes) if x is None else x
    got = x.transpose()
    assert_same_handle(mih, got, from_bed(mih, S.transpose_codes(codes)))
    return x, got


@pytest.mark.parametrize("n", EDGE_N)
def test_transpose_at_edge_shapes(mih, n):
    for p in EDGE_P:
        codes = edge_codes(n, p, 9000 * n + p)
        x, xt = check_transpose(mih, codes)
        cc, rm = xt.counts()
        want = np.stack([(codes.T == v).sum(axis=0) for v in (0, 1, 2, -1)], axis=1)
        assert np.array_equal(cc, want) and np.array_equal(rm, (codes < 0).sum(axis=0)), (n, p)


def _missing_patterns(n, p):
    base = np.random.default_rng(n * 17 + p).integers(0, 3, size=(n, p)).astype(np.int64)

    def put(rows, cols):
        c = base.copy()
        c[np.ix_(rows, cols)] = -1
        return c

    pats = {"none": base.copy(), "everything": np.full((n, p), -1, dtype=np.int64)}
    corners = base.copy()
    for i, j in ((0, 0), (0, p - 1), (n - 1, 0), (n - 1, p - 1)):
        corners[i, j] = -1
    pats["corners"] = corners
    tile = base.copy()                                            # first and last row of a tile, of either matrix
    for i in (0, 127, 128, 255):
        if i < n:
            tile[i, ::3] = -1
    for j in (0, 127, 128, 255):
        if j < p:
            tile[1::2, j] = -1
    pats["tile edges"] = tile
    pats["a whole column"] = put(range(n), [p // 2])
    pats["a whole row"] = put([n // 2], range(p))
    return pats


@pytest.mark.parametrize("shape", [(257, 385), (129, 33), (16, 129)])
def test_missing_genotypes_at_the_edges(mih, shape):
    n, p = shape
    for name, codes in _missing_patterns(n, p).items():
        x, xt = check_transpose(mih, codes)
        assert xt.counts()[0][:, 3].sum() == (codes < 0).sum(), name
        back = xt.transpose()                                     # twice is the matrix itself
        assert_same_handle(mih, back, x)


def test_transpose_twice_and_flags(mih):
    codes = edge_codes(129, 70, 3)
    x = from_bed(mih, codes)
    assert_same_handle(mih, x.transpose().transpose(), x)
    raw = x.transpose(center=False, scale=False, impute=False, reserve=-1)
    assert (raw.center, raw.scale, raw.impute) == (False, False, False) and raw.shape == (70, 129)
    want = mih.SnpLinAlg(bed_of(S.transpose_codes(codes)), 70, center=False, scale=False, impute=False)
    assert_same_handle(mih, raw, want)


def test_source_is_untouched(mih):
    codes = edge_codes(257, 129, 4)
    x = from_bed(mih, codes)
    R = np.random.default_rng(4).standard_normal((257, 3))
    before, bed = x.xtv(R), x.export_bed()
    xt = x.transpose()
    del xt
    assert np.array_equal(x.xtv(R).view(np.uint64), before.view(np.uint64))
    assert np.array_equal(x.export_bed(), bed)


def test_tall_image(mih):
    """n = 33, p = 2^18 + 33: the image has 2^18 + 33 rows, so its X'r passes run over more than one row slice."""
    n, p = 33, 2 ** 18 + 33
    rng = np.random.default_rng(33)
    codes = rng.integers(0, 3, size=(n, p)).astype(np.int64)
    codes[rng.random((n, p)) < 0.01] = -1
    codes[:, [0, p - 1, 2 ** 18]] = -1
    x = from_bed(mih, codes)
    xt = x.transpose(reserve=-1)
    assert xt.shape == (p, n)
    assert np.array_equal(xt.export_bed(), bed_of(S.transpose_codes(codes)))
    cc, rm = xt.counts()
    assert np.array_equal(cc, np.stack([(codes.T == v).sum(axis=0) for v in (0, 1, 2, -1)], axis=1))
    assert np.array_equal(rm, (codes < 0).sum(axis=0))


def test_refusals(mih):
    d = mih.DosageMatrix(np.zeros((4, 3), dtype=np.uint16), 1)
    assert not hasattr(d, "transpose")
    import ctypes as C
    h = C.c_void_p(None)
    assert mih.lib().mih_snp_transpose(d._h, 1, 1, 1, 64, -1, C.byref(h)) == 2 and not h.value          # MIH_BAD_ARG
    x = from_bed(mih, edge_codes(17, 5, 1))
    assert mih.lib().mih_snp_transpose(x._h, 1, 1, 1, 16, -1, C.byref(h)) == 2 and not h.value
