"""The exception lists of the score image in their wave-coalesced layout (csrc/score_image.hip: k_img_lists places the 16-byte
chunks of a slot group chunk-index-major, k_xtv_hom finds them again by ballots; the arithmetic is hom_chunk_slot of
csrc/score_image.h, checked on the host by tests/test_score_lists_cpu.py).  The yardstick is the one of test_gpu_score_image.py:
np.array_equal between the image's pass and the 2-bit pass on the SAME handle, with an explicit threshold.  The shapes are the
ones at which the placement can go wrong: list lengths that differ widely inside a group of 64 slots, one very long list among
empty ones, exactly one group, one slot more than a group, pad positions in the last group, a second workgroup of a slice that
is not full, slices with one and with two sub-slices, a ragged last block."""
import functools

import numpy as np
import pytest

from gpu_helpers import _pack

pytestmark = pytest.mark.gpu

IMG = "k_xtv_dma_img<1,2|1,4,8,fp4>+k_xtv_hom"
TWO_BIT = "k_xtv_dma<1,2,4,8,fp4>"
PLINK = np.array([0, 2, 3, 1], dtype=np.uint8)          # dosage 0, 1, 2, missing -> PLINK code
SUB_ROWS = 64 * 128                                     # kHomSubBlocks x 128 (csrc/common.h)


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


def _draw(rng, n, p):
    """Dosages p x n with allele frequencies uniform on 0.02 .. 0.5 (two uniform draws per genotype: quicker than binomial)."""
    maf = rng.uniform(0.02, 0.5, p).astype(np.float32)[:, None]
    g = (rng.random((p, n), dtype=np.float32) < maf).astype(np.uint8)
    g += rng.random((p, n), dtype=np.float32) < maf
    return g


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


def _two_bit(mih, x, residuals):
    x.score_image("release")
    base = []
    for r in residuals:
        out, names = _pass(mih, x, r)
        assert names == [TWO_BIT], names
        base.append(out)
    return base


def _image_equals(mih, x, residuals, base, tau, want_class1):
    nbytes, c1 = x.score_image("build", tau)
    assert nbytes > 0 and c1 == want_class1, (c1, want_class1)
    for r, want in zip(residuals, base):
        got, names = _pass(mih, x, r)
        assert names == [IMG], names
        assert _same_bits(got, want), int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    x.score_image("release")


N_MAIN, P_MAIN = 140_000, 700
RUN = (1000, 2500)                                      # column 1's 1500 consecutive dosage-2 rows
COMPANIONS = range(3, 83)                               # 80 columns of about as many dosage-2 entries as column 1, all of them elsewhere
COMPANION_ROWS = (7 * 69 * 128, 7 * 69 * 128 + SUB_ROWS)   # sub-slice 0 of slice 7


@functools.lru_cache(maxsize=None)
def _main_problem():
    """n = 140 000, p = 700: 16 row slices of 69 blocks -- two sub-slices (64 + 5 blocks) in every slice but the last, which has 59
    blocks and one; 704 positions at tau = 1: 11 slot groups, two workgroups of k_xtv_hom a slice (512 + 192 slots), four pad
    positions in the last group.  Column 0 holds no dosage 2.  Column 1 holds 1500 of them in a row inside sub-slice 0 of slice 0
    (188 chunks: past HomSum's flush at 85 terms many times) and none elsewhere; columns 3 .. 82 hold 1460 .. 1539 each, all of
    them inside sub-slice 0 of slice 7, so k_xtv_hom's order by falling count puts column 1 among them: in slice 0 its neighbouring
    lanes are empty, in slice 7 a whole group is long while column 1 is empty.  Column 2 holds a dosage 2 exactly in the first and
    last row of every slice and sub-slice.  Returns (the packed matrix, the columns' dosage-2 counts, the two residuals)."""
    n, p = N_MAIN, P_MAIN
    splits, bps = _row_slices(n, p)
    assert (splits, bps) == (16, 69) and SUB_ROWS < 128 * bps < 2 * SUB_ROWS
    assert -(-n // 128) - 15 * bps == 59                # the last slice: one sub-slice
    rng = np.random.default_rng(881)
    g = _draw(rng, n, p)
    g[0] = np.minimum(g[0], 1)
    g[1] = np.minimum(g[1], 1)
    assert RUN[1] <= SUB_ROWS                           # inside sub-slice 0 of slice 0
    g[1, RUN[0]:RUN[1]] = 2
    for i, j in enumerate(COMPANIONS):
        g[j] = np.minimum(g[j], 1)
        at = rng.choice(np.arange(*COMPANION_ROWS), 1460 + i, replace=False)
        g[j, at] = 2
    edges = []
    for s in range(splits):
        r0, r1 = 128 * bps * s, min(128 * bps * (s + 1), n)
        edges += [r0, r1 - 1]
        if r0 + SUB_ROWS < r1:
            edges += [r0 + SUB_ROWS - 1, r0 + SUB_ROWS]
    g[2] = np.minimum(g[2], 1)
    g[2, edges] = 2
    unit = 0.05 * rng.standard_normal(n)                # the edge rows dominate column 2's answer (the outlier guard leaves them in)
    unit[edges] = rng.choice([-1.0, 1.0], len(edges))
    residuals = [rng.standard_normal(n), unit]
    c2 = (g == 2).sum(axis=1)
    return _pack(PLINK[g]), c2, residuals


@functools.lru_cache(maxsize=None)
def _main_matrix(mih):
    """The main problem's handle and its 2-bit results, computed once for both thresholds."""
    packed, c2, residuals = _main_problem()
    x = mih.SnpLinAlg(packed, n=N_MAIN, center=True, scale=True, impute=True)
    return x, _two_bit(mih, x, residuals)


@pytest.mark.parametrize("tau", [1.0, 0.07])
def test_lists_of_widely_different_length_in_one_group(mih, tau):
    """tau = 1: every column one-bit (704 positions, no class-2 launch); tau = 0.07: f^2 <= 0.07 is f <= 0.26, about half of the
    columns, the planted ones among them."""
    _, c2, residuals = _main_problem()
    assert c2[0] == 0 and c2[1] == 1500 and 1460 <= c2[3] and c2[82] <= 1539 and c2[2] == 16 * 2 + 15 * 2
    one_bit = int(np.count_nonzero(c2 <= tau * N_MAIN))
    if tau == 1.0:
        assert one_bit == P_MAIN
    else:
        assert 0.35 * P_MAIN < one_bit < 0.65 * P_MAIN and np.all(c2[:83] <= tau * N_MAIN)
    x, base = _main_matrix(mih)
    _image_equals(mih, x, residuals, base, tau, one_bit)


@pytest.mark.parametrize("n,p,tau", [(3000, 64, 1.0), (3000, 65, 1.0), (3000, 130, 1.0), (3000, 130, 0.05)])
def test_group_edges_and_short_slices(mih, n, p, tau):
    """p = 64: one slot group exactly, no pad position; p = 65: one slot more than a group (a second group of one column and 63
    pads); n = 3000, p = 130: a ragged last block and two slices of 12 blocks -- a single short sub-slice each -- with three groups
    (tau = 1) or both classes (tau = 0.05)."""
    splits, bps = _row_slices(n, p)
    assert (splits, bps) == (2, 12)
    rng = np.random.default_rng([882, n, p])
    g = _draw(rng, n, p)
    g[0] = np.minimum(g[0], 1)                          # one empty list per slice in any case
    c2 = (g == 2).sum(axis=1)
    one_bit = int(np.count_nonzero(c2 <= tau * n))
    assert one_bit == p if tau == 1.0 else 0 < one_bit < p
    x = mih.SnpLinAlg(_pack(PLINK[g]), n=n, center=True, scale=True, impute=True)
    unit = np.zeros(n)
    unit[[0, 128 * bps - 1, 128 * bps, n - 1]] = (1.0, -1.0, 1.0, 1.0)
    residuals = [rng.standard_normal(n), unit + 0.05 * rng.standard_normal(n)]
    _image_equals(mih, x, residuals, _two_bit(mih, x, residuals), tau, one_bit)


def test_fit_at_the_default_threshold_equals_the_fit_without_image(mih):
    """A device-resident Normal fit (step_mode 0) that backtracks, with the image built at the library's default threshold
    (max_hom_fraction = 0) and without it: model, loglikelihood trace and backtracks identical."""
    n, p = 2000, 7500                                   # (more effects than the rows support: some steps backtrack)
    x = mih.SnpLinAlg.synthetic(n, p, seed=4)
    rng = np.random.default_rng(883)
    supp = np.sort(rng.choice(p, 400, replace=False))
    y = x.xv_sparse(supp, rng.standard_normal(400)) + 0.05 * rng.standard_normal(n)
    runs = {}
    for image in (False, True):
        if image:
            nbytes, c1 = x.score_image("build")
            assert nbytes > 0 and 0 < c1 < p
        else:
            x.score_image("release")
        mih.profile_passes(x, reset=True)
        mih.profile_enable(x, True)
        try:
            f = mih.fit_iht(y, x, None, verbose=False, step_mode=0, k=750, max_iter=30)
        finally:
            mih.profile_enable(x, False)
        names = {q["kernel"] for q in mih.profile_passes(x, reset=True)} & {IMG, TWO_BIT}
        assert names == ({IMG} if image else {TWO_BIT}), names
        runs[image] = f
    a, b = runs[False], runs[True]
    assert int(np.sum(a.trace["backtracks"])) > 0
    assert a.iter == b.iter and list(a.trace["backtracks"]) == list(b.trace["backtracks"])
    assert _same_bits(a.beta, b.beta) and _same_bits(a.c, b.c)
    assert _same_bits(a.trace["logl"], b.trace["logl"]) and _same_bits(a.trace["tol"], b.trace["tol"])
    assert a.logl == b.logl
