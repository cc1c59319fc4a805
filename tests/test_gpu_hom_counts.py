"""k_xtv_hom's digit sums by carry-save positional counting (HomCsa of csrc/score_image.h; its arithmetic is checked on the host
by tests/test_hom_csa_cpu.py).  The kernel adds a list in rounds of 4 chunks (kCsaGroup) of 8 entries, a list that has ended
feeds zero words, and the 4-bit fields behind the adders are emptied before the 6th round since the last time (kCsaFlush = 5) --
by the whole wave, whose rounds are those of its longest list.  The yardstick is the one of test_gpu_score_lists.py:
np.array_equal between the image's pass and the 2-bit pass on the SAME handle, with an explicit threshold.  The shape: three
sub-slices in every row slice, the last one short, and planted columns whose lists end at every place of a round."""
import functools

import numpy as np
import pytest

from gpu_helpers import _pack, peel_rule

pytestmark = pytest.mark.gpu

IMG = "k_xtv_dma_img<1,2|1,4,8,fp4>+k_xtv_hom"
TWO_BIT = "k_xtv_dma<1,2,4,8,fp4>"
PLINK = np.array([0, 2, 3, 1], dtype=np.uint8)          # dosage 0, 1, 2, missing -> PLINK code
SUB_ROWS = 64 * 128                                     # kHomSubBlocks x 128 (csrc/common.h)
CHUNK, GROUP, FLUSH = 8, 4, 5                           # kHomChunk, kCsaGroup, kCsaFlush (csrc/score_image.h)

N, P = 2078 * 128 + 100, 192
SPLITS, BPS = 16, 130
SLICE_ROWS = 128 * BPS
LONG = 0                                                # 9 + 8 + 1 chunks in the three sub-slices of slice 0: 3 + 2 + 1 rounds
LADDER = range(1, 64)                                   # column i: i chunks in sub-slice 0 of slice 1
EXACT = [0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 40, 41]      # (17 .. 24: one chunk fewer than a round, 33 .. 40: one more)
EXACT_COLS = range(64, 64 + len(EXACT))
HIGH_MAF = range(176, P)                                # 16 .. 25 % dosage 2: class 2 at tau = 0.05 (the columns before: at most about 1 %)
BALLAST = 4000                                          # dosage-2 entries in slice 3 that put columns 0 .. 63 first in k_xtv_hom's order


def _row_slices(n, p):
    """auto_splits of csrc/xtv.hip restated (as in test_gpu_score_image.py): (slices, blocks per slice)."""
    nbp = -(-n // 128)
    groups = (-(-p // 32) + 15) // 16
    s = 1
    while s < 4 and n >= 100000 * s:
        s *= 2
    while s < 16 and groups * s < 2048 and nbp // (2 * s) >= 8:
        s *= 2
    s = min(s, nbp)
    return s, -(-nbp // s)


def _pass(mih, x, r):
    mih.profile_passes(x, reset=True)
    mih.profile_enable(x, True)
    try:
        out = x.xtv(r, xtv_digits=428)
    finally:
        mih.profile_enable(x, False)
    return out, [q["kernel"] for q in mih.profile_passes(x, reset=True)]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def _problem():
    """n = 266 084, p = 192: 16 row slices of 130 blocks (the last: 129, with 100 rows in its last block), so every slice has the
    sub-slices 64 + 64 + 2 (the last slice: + 1) blocks.  Columns 0 .. 63 are one slot group of k_xtv_hom (4000 and more dosage-2
    entries each in slice 3 put them first in its order by falling count; every other column has fewer):
      * column 0 holds 72, 64 and 1 dosage-2 entries in the three sub-slices of slice 0, where the other 63 lists of its group are
        empty: 3 + 2 + 1 = kCsaFlush + 1 rounds of the wave, the sixth one after the fields were emptied;
      * column i = 1 .. 63 holds i chunks in sub-slice 0 of slice 1 (with 1 .. 8 entries in the last), column 0 none: 64 lists of
        64 different lengths, a lane leaves after every chunk of every round.
    Columns 64 .. 78 hold EXACT[i] entries in sub-slice 1 of slice 2, the same number (up to 41 <= 100 rows) in the short last
    sub-slice of the last slice, the matrix's last row among them, and none elsewhere.  The rest are ordinary columns of low and
    (the last 16) high allele frequency.  Returns (packed matrix, dosage-2 counts, the residuals)."""
    assert _row_slices(N, P) == (SPLITS, BPS) and 2 * SUB_ROWS < SLICE_ROWS < 3 * SUB_ROWS
    assert -(-N // 128) - (SPLITS - 1) * BPS == 129 and N - (SPLITS - 1) * SLICE_ROWS - 2 * SUB_ROWS == 100
    rng = np.random.default_rng(991)
    maf = np.concatenate([rng.uniform(0.02, 0.1, HIGH_MAF[0]), rng.uniform(0.4, 0.5, len(HIGH_MAF))]).astype(np.float32)[:, None]
    g = (rng.random((P, N), dtype=np.float32) < maf).astype(np.uint8)
    g[64 + len(EXACT):] += rng.random((P - 64 - len(EXACT), N), dtype=np.float32) < maf[64 + len(EXACT):]

    def plant(col, row0, rows, count, must=()):
        at = rng.choice(np.setdiff1d(np.arange(row0, row0 + rows), must), count - len(must), replace=False)
        g[col, at] = 2
        g[col, list(must)] = 2

    long_counts = (9 * CHUNK, 8 * CHUNK, 1)
    assert sum(-(-c // (CHUNK * GROUP)) for c in long_counts) == FLUSH + 1
    for sub, count in enumerate(long_counts):
        plant(LONG, sub * SUB_ROWS, min(SUB_ROWS, SLICE_ROWS - sub * SUB_ROWS), count)
    for i in LADDER:
        plant(i, SLICE_ROWS, SUB_ROWS, CHUNK * (i - 1) + 1 + i % CHUNK)
    for col in range(64):
        plant(col, 3 * SLICE_ROWS, SLICE_ROWS, BALLAST + 64 - col)
    for col, count in zip(EXACT_COLS, EXACT):
        plant(col, 2 * SLICE_ROWS + SUB_ROWS, SUB_ROWS, count)
        plant(col, (SPLITS - 1) * SLICE_ROWS + 2 * SUB_ROWS, 100, count, must=(N - 1,) if count else ())
    c2 = (g == 2).sum(axis=1)
    assert np.all(c2[64:176] < BALLAST) and np.all(c2[:64] > BALLAST)
    assert np.all(c2[:176] <= 0.05 * N) and np.all(c2[176:] > 0.05 * N)
    planted = np.flatnonzero((g[:64 + len(EXACT)] == 2).any(axis=0))     # the dosage-2 rows of the planted columns
    normal = rng.standard_normal(N)
    big = 2.0 - 2.0 ** -52                              # +-max on exactly those rows: |R| at the top of its 54 bits, fields of 0 and 3
    saturated = np.clip(0.25 * rng.standard_normal(N), -1.5, 1.5)
    saturated[planted] = rng.choice([-big, big], planted.size)
    assert len(peel_rule(saturated)) == 0
    # 2/3 of a power of two on every planted row: every digit +1, every field of U at 3 wherever the scale is a power of two -- in
    # column 63's 63 chunks that is 15 rounds in a row whose carry words hold a 3 in every field
    thirds = np.clip(0.25 * rng.standard_normal(N), -1.5, 1.5)
    thirds[planted] = float(0x0055555555555555) * 2.0 ** -53
    thirds[np.setdiff1d(np.arange(N), planted)[0]] = big
    assert len(peel_rule(thirds)) == 0
    zero = rng.standard_normal(N)
    zero[planted] = 0.0                                 # every list entry reads U of R = 0, like the padding
    peeled = rng.standard_normal(N)
    row = int(np.flatnonzero(g[LONG, :SUB_ROWS] == 2)[0])                # a dosage-2 row of column 0 in sub-slice 0 of slice 0
    peeled[row] = 1e8
    assert [int(i) for i in peel_rule(peeled)] == [row]
    return _pack(PLINK[g]), c2, [normal, saturated, thirds, zero, peeled]


@functools.lru_cache(maxsize=None)
def _matrix(mih):
    """The handle and its 2-bit results, computed once for both thresholds."""
    packed, _, residuals = _problem()
    x = mih.SnpLinAlg(packed, n=N, center=True, scale=True, impute=True)
    x.score_image("release")
    base = []
    for r in residuals:
        out, names = _pass(mih, x, r)
        assert names == [TWO_BIT], names
        base.append(out)
    return x, base


@pytest.mark.parametrize("tau", [1.0, 0.05])
def test_lists_that_end_at_every_place_of_a_round(mih, tau):
    """tau = 1: every column one-bit (no class-2 launch); tau = 0.05: the 16 columns of high allele frequency are class 2, every
    planted column is class 1.  Five residuals: normal; +-max on exactly the planted dosage-2 rows; the value whose digits are all +1 on
    them; zero on all of them; one peeled outlier on a dosage-2 row of column 0."""
    _, c2, residuals = _problem()
    one_bit = int(np.count_nonzero(c2 <= tau * N))
    assert one_bit == (P if tau == 1.0 else 176)
    x, base = _matrix(mih)
    nbytes, c1 = x.score_image("build", tau)
    assert nbytes > 0 and c1 == one_bit, (c1, one_bit)
    for r, want in zip(residuals, base):
        got, names = _pass(mih, x, r)
        assert names == [IMG], names
        assert _same_bits(got, want), int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    x.score_image("release")


def test_resident_fit_with_every_column_one_bit(mih):
    """A device-resident Normal fit (step_mode 0) of a few steps that backtracks, with the image at max_hom_fraction = 1 (every
    column's dosage 2 goes through k_xtv_hom) and without it: model and loglikelihood identical."""
    n, p = 2000, 7500                                   # (more effects than the rows support: some steps backtrack)
    x = mih.SnpLinAlg.synthetic(n, p, seed=4)
    rng = np.random.default_rng(992)
    supp = np.sort(rng.choice(p, 400, replace=False))
    y = x.xv_sparse(supp, rng.standard_normal(400)) + 0.05 * rng.standard_normal(n)
    runs = {}
    for image in (False, True):
        if image:
            nbytes, c1 = x.score_image("build", 1.0)
            assert nbytes > 0 and c1 == p
        else:
            x.score_image("release")
        mih.profile_passes(x, reset=True)
        mih.profile_enable(x, True)
        try:
            f = mih.fit_iht(y, x, None, verbose=False, step_mode=0, k=750, max_iter=8)
        finally:
            mih.profile_enable(x, False)
        names = {q["kernel"] for q in mih.profile_passes(x, reset=True)} & {IMG, TWO_BIT}
        assert names == ({IMG} if image else {TWO_BIT}), names
        runs[image] = f
    a, b = runs[False], runs[True]
    assert int(np.sum(a.trace["backtracks"])) > 0
    assert a.iter == b.iter and list(a.trace["backtracks"]) == list(b.trace["backtracks"])
    assert _same_bits(a.beta, b.beta) and _same_bits(a.c, b.c)
    assert _same_bits(a.trace["logl"], b.trace["logl"])
    assert a.logl == b.logl
