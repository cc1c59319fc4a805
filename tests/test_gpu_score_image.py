"""The score image of a 2-bit matrix (csrc/score_image.hip, mih_mat_score_image): the single-residual X'r pass in the 428 format
over the image -- one-bit tiles for the columns with few dosage-2 entries, exact digit sums for those entries (k_xtv_hom) -- gives
bit for bit what the pass over the matrix gives.  Every comparison is np.array_equal between the SAME handle with and without the
image; the image is forced with the explicit call, and the pass record's kernel name says which pass ran."""
import functools

import numpy as np
import pytest

from gpu_helpers import _pack, peel_rule

pytestmark = pytest.mark.gpu

IMG = "k_xtv_dma_img<1,2|1,4,8,fp4>+k_xtv_hom"
TWO_BIT = "k_xtv_dma<1,2,4,8,fp4>"
PLINK = np.array([0, 2, 3, 1], dtype=np.uint8)          # dosage 0, 1, 2, missing (3 here) -> PLINK code


@functools.lru_cache(maxsize=None)
def _dosage(n, p, miss, seed):
    """Dosages p x n (3 = missing) with allele frequencies spread over 0.02 .. 0.5: at max_hom_fraction = 0.05 (f^2 <= 0.05, f <= 0.22)
    both classes are populated."""
    rng = np.random.default_rng([771, n, p, seed])
    maf = rng.uniform(0.02, 0.5, p)
    maf[:2] = (0.03, 0.45)                              # one column of each class whatever the draw
    g = rng.binomial(2, maf[:, None], size=(p, n)).astype(np.uint8)
    if miss:
        g[rng.random((p, n)) < miss] = 3
    g.setflags(write=False)
    return g


def _matrix(mih, g, center=True, scale=True, impute=True):
    return mih.SnpLinAlg(_pack(PLINK[g]), n=g.shape[1], center=center, scale=scale, impute=impute)


def _pass(mih, x, r):
    """One single-residual 428 pass: (result, the kernel names of its pass records)."""
    mih.profile_passes(x, reset=True)
    mih.profile_enable(x, True)
    try:
        out = x.xtv(r, xtv_digits=428)
    finally:
        mih.profile_enable(x, False)
    return out, [q["kernel"] for q in mih.profile_passes(x, reset=True)]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _check(mih, x, residuals, tau, want_class1=None):
    """Every residual through the 2-bit pass and through the image's; returns the 2-bit results."""
    x.score_image("release")
    base = []
    for r in residuals:
        out, names = _pass(mih, x, r)
        assert names == [TWO_BIT], names
        base.append(out)
    nbytes, c1 = x.score_image("build", tau)
    assert nbytes > 0 and c1 > 0
    if want_class1 is not None:
        assert c1 == want_class1, (c1, want_class1)
    assert x.score_image("query") == (nbytes, c1)
    for r, want in zip(residuals, base):
        got, names = _pass(mih, x, r)
        assert names == [IMG], names
        assert _same_bits(got, want), int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    x.score_image("release")
    assert x.score_image("query") == (0, 0)
    return base


def _residuals(n, seed):
    rng = np.random.default_rng([772, n, seed])
    g = rng.standard_normal(n)
    # one entry at +-max, the rest large enough that the outlier guard leaves the row in: |R| of that row is at the top of the 54 bits
    top = np.clip(rng.standard_normal(n) * 0.25, -1.5, 1.5)
    top[n - 1] = 1.0
    top[n // 3] = -(2.0 - 2.0 ** -52)
    top2 = top.copy()
    top2[n // 3] = 2.0 - 2.0 ** -52
    return [g, np.zeros(n), top, top2, np.ones(n)]


@pytest.mark.parametrize("n,p", [(257, 70), (383, 33), (3000, 70), (128 * 33, 33)])
@pytest.mark.parametrize("tau", [0.05, 1.0])
def test_image_pass_equals_two_bit_pass(mih, n, p, tau):
    """p = 70 and 33: an odd number of one-bit column groups, a half-empty last tile, pad columns; n = 257, 383: a ragged last
    block; n = 3000, 128 x 33: two and four row slices of unequal length.  tau = 0.05: both classes; tau = 1: every column one-bit
    (no class-2 launch)."""
    g = _dosage(n, p, 0.0, 0)
    c2 = (g == 2).sum(axis=1)
    want = int(np.count_nonzero(c2 <= tau * n))
    assert want == p if tau == 1.0 else 0 < want < p
    x = _matrix(mih, g)
    _check(mih, x, _residuals(n, 0), tau, want_class1=want)


def test_no_column_qualifies_is_refused(mih):
    g = _dosage(3000, 70, 0.0, 0).copy()
    g[:, 7] = 2                                         # every column holds a dosage 2
    x = _matrix(mih, g)
    with pytest.raises(mih.MendelIHTError):
        x.score_image("build", 1e-9)                    # not one dosage-2 entry allowed: no column qualifies
    assert x.score_image("query") == (0, 0)
    r = np.random.default_rng(5).standard_normal(3000)
    out, names = _pass(mih, x, r)
    assert names == [TWO_BIT]


def test_nan_residual_is_nan_in_every_column_both_ways(mih):
    n, p = 3000, 70
    x = _matrix(mih, _dosage(n, p, 0.0, 0))
    r = np.random.default_rng(6).standard_normal(n)
    r[17] = np.nan
    a, names = _pass(mih, x, r)
    assert names == [TWO_BIT] and np.isnan(a).all()
    x.score_image("build", 0.05)
    b, names = _pass(mih, x, r)
    assert names == [IMG] and np.isnan(b).all()


@pytest.mark.parametrize("center,scale,impute", [(1, 1, 1), (1, 1, 0), (0, 0, 1), (0, 0, 0), (1, 0, 1)])
def test_missing_genotypes_and_matrix_options(mih, center, scale, impute):
    n, p = 3000, 70
    g = _dosage(n, p, 0.02, 1)
    x = _matrix(mih, g, bool(center), bool(scale), bool(impute))
    _check(mih, x, _residuals(n, 1)[:3], 0.05)


def test_synthetic_shard_with_a_column_offset(mih):
    x = mih.SnpLinAlg.synthetic(3000, 70, seed=5, col_offset=1000)
    base = _check(mih, x, _residuals(3000, 2)[:2], 0.05)
    whole = mih.SnpLinAlg.synthetic(3000, 1070, seed=5)
    want = whole.xtv(_residuals(3000, 2)[0], xtv_digits=428)[1000:]
    assert _same_bits(base[0], want)                    # (the shard is that block of the whole matrix)


SUB_ROWS = 64 * 128          # kHomSubBlocks x 128 (csrc/common.h): the rows of a sub-slice of the exception lists


def _row_slices(n, p):
    """auto_splits of csrc/xtv.hip restated for any n (gpu_helpers.xtv_slices stops at 100 000 rows): the slice count doubles to 4
    while n >= 100 000 s, then on to 16 while ceil(ceil(p / 32) / 16) s < 2048 and nbp // (2 s) >= 8; never more than nbp.  Returns
    (slices, blocks per slice).  test_exception_lists_at_slice_and_sub_slice_edges checks it against the library through the
    results: a wrong slice count here would put the planted rows off the edges, not change the outcome, so the count the test relies
    on is asserted where it is used."""
    nbp = -(-n // 128)
    groups = (-(-p // 32) + 15) // 16
    s = 1
    while s < 4 and n >= 100000 * s:
        s *= 2
    while s < 16 and groups * s < 2048 and nbp // (2 * s) >= 8:
        s *= 2
    s = min(s, nbp)
    return s, -(-nbp // s)


@functools.lru_cache(maxsize=None)
def _exception_problem():
    """n = 300 000 rows, p = 70: 16 row slices of 147 blocks, so every slice has THREE sub-slices (64 + 64 + 19 blocks).  Column 0 holds
    no dosage 2, column 1 nothing but dosage 2 (sparse), column 2 a dosage 2 exactly in the first and last row of every slice and of
    every sub-slice, column 3 1500 dosage-2 entries in a row inside one sub-slice (and few elsewhere): all four are one-bit at
    tau = 0.05."""
    n, p = 300_000, 70
    rng = np.random.default_rng(773)
    maf = rng.uniform(0.02, 0.5, p)
    g = rng.binomial(2, maf[:, None], size=(p, n)).astype(np.uint8)
    g[0] = np.minimum(g[0], 1)
    g[1] = 2 * (rng.random(n) < 0.01)
    splits, bps = _row_slices(n, p)
    assert (splits, bps) == (16, 147) and 2 * SUB_ROWS < 128 * bps < 3 * SUB_ROWS      # the shape the docstring describes
    edges = []
    for s in range(splits):
        r0, r1 = 128 * bps * s, min(128 * bps * (s + 1), n)
        edges += [r0, r1 - 1] + [r0 + k * SUB_ROWS + d for k in (1, 2) for d in (-1, 0)]
    g[2] = rng.binomial(1, 0.1, n)
    g[2, edges] = 2
    g[3] = rng.binomial(1, 0.2, n)
    g[3, 20000:21500] = 2                               # inside sub-slice 0 of slice 1 (a slice is 147 x 128 = 18816 rows, a sub-slice 8192)
    g[3, 1000:2500] = 2                                 # and inside sub-slice 0 of slice 0
    return g, edges


def _image_bytes(g, tau, splits, bps):
    """The bytes mih_mat_score_image reports (ScoreImage::bytes, csrc/score_image.hip) for dosages g if the pass has `splits` row
    slices of `bps` blocks: tiles, column map, thread order, list offsets and the lists -- every (slice, sub-slice, one-bit column)
    list padded to 8 entries of 2 bytes.  The lists' padding depends on where the slices and sub-slices are cut, so the figure is
    the library's only if its row slices are these."""
    p, n = g.shape
    nbp = -(-n // 128)
    two = g == 2
    one_bit = two.sum(axis=1) <= tau * n
    p1 = int(one_bit.sum())
    ncg2, nt1 = -(-(p - p1) // 32), -(-p1 // 64)
    nss = -(-bps // (SUB_ROWS // 128))
    cuts = [min(128 * (s * bps + k * (SUB_ROWS // 128)), n) for s in range(splits) for k in range(nss)]
    ends = [min(c + SUB_ROWS, 128 * min((s + 1) * bps, nbp), n) for c, (s, k) in zip(cuts, [(s, k) for s in range(splits) for k in range(nss)])]
    chunks = 0
    for lo, hi in zip(cuts, ends):
        if hi > lo:
            chunks += int((-(-two[one_bit, lo:hi].sum(axis=1) // 8)).sum())
    nseg = splits * nss * 2 * nt1 * 32
    return (ncg2 + nt1) * nbp * 1024 + 4 * ((ncg2 + 2 * nt1) * 32 + nt1 * 64) + 4 * (nseg + 1) + max(16 * chunks, 16)


def test_exception_lists_at_slice_and_sub_slice_edges(mih):
    g, edges = _exception_problem()
    n = g.shape[1]
    c2 = (g == 2).sum(axis=1)
    # the library cuts its lists where this file thinks the slices and sub-slices are: the image's size says so (a change of
    # auto_splits or of the sub-slice length moves the lists' padding and the offset table, and fails here instead of silently
    # taking the planted rows off the edges)
    x0 = _matrix(mih, g)
    assert x0.score_image("build", 0.05)[0] == _image_bytes(g, 0.05, *_row_slices(n, g.shape[0]))
    assert x0.score_image("build", 0.05)[0] != _image_bytes(g, 0.05, 8, 2 * 147)
    del x0
    assert c2[0] == 0 and (g[1] == 1).sum() == 0 and c2[1] > 0 and c2[3] >= 3000 and np.all(c2[:4] <= 0.05 * n)
    x = _matrix(mih, g)
    rng = np.random.default_rng(774)
    unit = 0.05 * rng.standard_normal(n)                # the edge rows dominate (not by so much that the outlier guard takes them out):
    unit[edges] = rng.choice([-1.0, 1.0], len(edges))   # column 2's exceptions are most of its answer
    _check(mih, x, [rng.standard_normal(n), unit], 0.05, want_class1=int(np.count_nonzero(c2 <= 0.05 * n)))


@pytest.mark.parametrize("shape", ["one_outlier_1e8", "two_outliers"])
def test_peeled_row_with_a_two_in_a_one_bit_column(mih, shape):
    """The outlier shapes of test_xtv_fixed_point_under_adversarial_dynamic_range: the peeled rows ride the f64 side channel of the
    finalize kernel and have zero digits, so a dosage 2 on such a row contributes nothing to k_xtv_hom's sums either."""
    n, p = 3000, 48
    g = _dosage(n, p, 0.0, 3).copy()
    rng = np.random.default_rng(31415)
    r = rng.standard_normal(n)
    i0 = int(np.argmax(np.abs(r)))
    if shape == "one_outlier_1e8":
        r[i0] *= 1e8
        rows = [i0]
    else:
        r[5] *= 1e9
        r[2000] *= -3e6
        rows = [5, 2000]
    assert set(rows) <= set(int(i) for i in peel_rule(r))
    one_bit = np.flatnonzero((g == 2).sum(axis=1) + len(rows) <= 0.05 * n)
    assert one_bit.size >= 2
    g[one_bit[:2][:, None], rows] = 2
    x = _matrix(mih, g, False, False, False)
    _check(mih, x, [r], 0.05)


def _fit_record(mih, y, x, z, step_mode, **kw):
    mih.profile_passes(x, reset=True)
    mih.profile_counters(x, reset=True)
    mih.profile_enable(x, True)
    try:
        f = mih.fit_iht(y, x, z, verbose=False, step_mode=step_mode, **kw)
    finally:
        mih.profile_enable(x, False)
    names = {q["kernel"] for q in mih.profile_passes(x, reset=True)} & {IMG, TWO_BIT}
    return f, mih.profile_counters(x, reset=True), names


def test_fits_are_identical_with_and_without_the_image(mih):
    """A Normal fit that backtracks, device-resident (step_mode 0) and host-driven (step_mode 1), on the same handle without and
    with the image: iterations, backtracks, beta, c, the loglikelihood trace and tol are identical, resident_handbacks unchanged."""
    n, p = 400, 1500                                    # (more effects than the rows support: steps 2, 4 and 5 backtrack)
    x = mih.SnpLinAlg.synthetic(n, p, seed=4)
    rng = np.random.default_rng(775)
    supp = np.sort(rng.choice(p, 80, replace=False))
    y = x.xv_sparse(supp, rng.standard_normal(80)) + 0.05 * rng.standard_normal(n)
    kw = dict(k=150, max_iter=30)
    runs = {}
    for image in (False, True):
        x.score_image("build" if image else "release", 0.05)
        for mode in (0, 1):
            f, cnt, names = _fit_record(mih, y, x, None, mode, **kw)
            assert names == ({IMG} if image else {TWO_BIT}), names
            runs[image, mode] = (f, cnt)
    assert int(np.sum(runs[False, 0][0].trace["backtracks"])) > 0
    for mode in (0, 1):
        (a, ca), (b, cb) = runs[False, mode], runs[True, mode]
        assert a.iter == b.iter and list(a.trace["backtracks"]) == list(b.trace["backtracks"])
        assert _same_bits(a.beta, b.beta) and _same_bits(a.c, b.c)
        assert _same_bits(a.trace["logl"], b.trace["logl"]) and _same_bits(a.trace["tol"], b.trace["tol"])
        assert ca["resident_handbacks"] == cb["resident_handbacks"]
        assert ca["resident_steps"] == cb["resident_steps"]


def test_trim_drops_an_unpinned_image_and_spares_a_pinned_one(mih):
    n, p = 3000, 70
    x = _matrix(mih, _dosage(n, p, 0.0, 0))
    r = np.random.default_rng(8).standard_normal(n)
    want, names = _pass(mih, x, r)
    assert names == [TWO_BIT]
    nbytes, _ = x.score_image("build", 0.05)
    got, names = _pass(mih, x, r)
    assert names == [IMG] and _same_bits(got, want)
    assert mih.device_trim(0) >= nbytes                  # nobody uses it: gone
    assert x.score_image("query") == (0, 0)
    got, names = _pass(mih, x, r)
    assert names == [TWO_BIT] and _same_bits(got, want)
    # a live session pins the image it was created on
    x.score_image("build", 0.05)
    y = x.xv_sparse(np.array([3, 40]), np.array([0.5, -0.7])) + r
    sess = mih.IHTSession(y, x, None, k=4)
    mih.device_trim(0)
    assert x.score_image("query")[0] == nbytes
    mih.profile_passes(x, reset=True)
    mih.profile_enable(x, True)
    sess.step()
    mih.profile_enable(x, False)
    assert IMG in {q["kernel"] for q in mih.profile_passes(x, reset=True)}
    sess.close()
    del sess
    assert mih.device_trim(0) >= nbytes
    assert x.score_image("query") == (0, 0)
