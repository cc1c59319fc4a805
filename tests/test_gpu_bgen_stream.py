"""BGEN streamed into the device dosage matrix (genotypes.read_bgen_device, mih_dosage_create_bgen): the matrix is the one the
host reader builds, bit for bit; variant ranges and regrids; parse_genotypes, iht and cross_validate routed through it; the
files it does not take go to read_bgen unchanged; read_bgen's refusals word for word; bounded host memory."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from bgen_files import genotype_block, write_blocks, write_imputed, write_probs
from conftest import FIX, GOLD, ROOT
from test_genotype_readers_cpu import bed_codes

import mendeliht_amd as M
from mendeliht_amd import genotypes as G
from mendeliht_amd.api import ArgumentError

pytestmark = pytest.mark.gpu


def old_matrix(path, sample_path=None):
    num, den = G.genotype_values(G.read_bgen(path, sample_path)[0])
    return M.DosageMatrix(num, den)


def assert_same(x, y):
    assert isinstance(x, M.DosageMatrix) and x.denom == y.denom and (x.n, x.p) == (y.n, y.p)
    assert np.array_equal(x.export(), y.export())
    for a, b in zip(x.mu_sigma(), y.mu_sigma()):
        assert np.array_equal(a, b)


def streamed(path, **kw):
    got = G.read_bgen_device(path, **kw)
    want = G.read_bgen(path, kw.get("sample_path"))
    assert list(got[1:]) == list(want[1:])
    return got[0]


def probs(rng, n, p, nbits, missing=0.05, hard=False):
    full = (1 << nbits) - 1
    if hard:
        g = rng.integers(0, 3, (n, p))
        kaa, kab = np.where(g == 0, full, 0), np.where(g == 1, full, 0)
    else:
        kaa = rng.integers(0, full + 1, (n, p))
        kab = (rng.random((n, p)) * (full - kaa + 1)).astype(np.int64)
    return kaa, kab, rng.random((n, p)) < missing


def test_golden_excerpt(mih):
    path, sp = os.path.join(GOLD, "normal_head.bgen"), os.path.join(GOLD, "normal.sample")
    x = streamed(path, sample_path=sp)
    assert x.denom == 1
    assert_same(x, old_matrix(path, sp))


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("nbits", range(1, 17))
def test_every_depth_and_size(mih, tmp_path, nbits, comp):
    rng = np.random.default_rng([nbits, comp])
    for n in (1, 7, 8, 9, 1000, 4099):
        path = str(tmp_path / f"b{n}.bgen")
        kaa, kab, miss = probs(rng, n, 11, nbits, hard=nbits == 16)
        if nbits == 16:                  # fractional 16-bit dosages are not on a 16-bit grid: multiples of 3 (denominator 21845)
            kaa[::3, 1], kab[::3, 1] = 0, 21
        write_probs(path, kaa, kab, miss, nbits, comp=comp, samples=n % 2 == 1)
        assert_same(streamed(path), old_matrix(path))


def test_grid_reductions(mih, tmp_path):
    rng = np.random.default_rng(7)
    n, p = 300, 6
    cases = {}
    cases[1] = probs(rng, n, p, 8, hard=True)                                   # 8-bit hard calls: denominator 1
    kaa, kab, miss = probs(rng, n, p, 8)
    cases[3] = (kaa // 85 * 85, kab // 85 * 85, miss)                           # numerators all multiples of 85: 255 / 85 = 3
    cases[255] = probs(rng, n, p, 8)                                            # fractional 8-bit: 255
    kaa, kab, miss = probs(rng, n, p, 16)
    kaa, kab = kaa // 3 * 3, kab // 3 * 3
    kaa[0, :], kab[0, :], miss[0, :] = 0, 3, False                              # a numerator with no factor 5, 17 or 257
    cases[21845] = (kaa, kab, miss)                                             # 16-bit multiples of 3: 65535 / 3
    for want, (kaa, kab, miss) in cases.items():
        path = str(tmp_path / f"g{want}.bgen")
        write_probs(path, kaa, kab, miss, 16 if want == 21845 else 8)
        x = streamed(path)
        assert x.denom == want, (want, x.denom)
        assert_same(x, old_matrix(path))
    # columns whose own divisors differ (g_j = 255, 85, 1: hard calls, multiples of 85, fractional) end on the common grid
    a, b, c = probs(rng, n, 3, 8, hard=True), probs(rng, n, 3, 8), probs(rng, n, 3, 8)
    kaa = np.concatenate([a[0], b[0] // 85 * 85, c[0]], axis=1)
    kab = np.concatenate([a[1], b[1] // 85 * 85, c[1]], axis=1)
    miss = np.concatenate([a[2], b[2], c[2]], axis=1)
    path = str(tmp_path / "mixed.bgen")
    write_probs(path, kaa, kab, miss, 8)
    x = streamed(path)
    assert x.denom == 255
    assert_same(x, old_matrix(path))


def test_many_workers(mih, tmp_path):
    path = str(tmp_path / "big.bgen")
    write_imputed(path, 200_000, 100, 8, seed=3)
    want = old_matrix(path)
    assert_same(streamed(path), want)
    assert_same(streamed(path, threads=3), want)


def test_variant_ranges_regrid_to_the_whole(mih, tmp_path):
    rng = np.random.default_rng(11)
    n, p = 500, 60
    kaa, kab, miss = probs(rng, n, p, 8)
    kaa[:, :20], kab[:, :20] = kaa[:, :20] // 85 * 85, kab[:, :20] // 85 * 85        # columns 0..19: grid 1/3
    g = rng.integers(0, 3, (n, 20))
    kaa[:, 20:40], kab[:, 20:40] = np.where(g == 0, 255, 0), np.where(g == 1, 255, 0)   # 20..39: hard calls
    path = str(tmp_path / "r.bgen")
    write_probs(path, kaa, kab, miss, 8)
    whole = streamed(path)
    assert whole.denom == 255
    mu, s = whole.mu_sigma()
    for a, b, own in ((0, 20, 3), (20, 40, 1), (40, 60, 255), (5, 45, 255), (33, 34, 1)):
        x, samples, chrom, pos, ids, ref, alt = G.read_bgen_device(path, variants=range(a, b))
        assert x.denom == own and x.p == b - a and ids == [f"rs{j + 1}" for j in range(a, b)]
        x.regrid(whole.denom)
        assert x.denom == whole.denom
        assert np.array_equal(x.export(), whole.export(a, b - a))
        assert np.array_equal(x.mu_sigma()[0], mu[a:b]) and np.array_equal(x.mu_sigma()[1], s[a:b])
    with pytest.raises(ArgumentError):
        G.read_bgen_device(path, variants=range(0, 5))[0].regrid(100)              # not a multiple of 3


@pytest.fixture(scope="module")
def pheno_bgen(tmp_path_factory):
    """data/normal's first 2000 variants as 8-bit BGEN with some imputation-like uncertainty, and its phenotypes"""
    d = tmp_path_factory.mktemp("route")
    n = 1000
    codes = bed_codes(os.path.join(FIX, "normal.bed"), n)[:, :2000]
    soft = np.random.default_rng(5).random(codes.shape) < 0.1
    kaa = np.where(codes == 0, np.where(soft, 240, 255), 0)
    kab = np.where(codes == 1, 255, np.where(soft & (codes == 0), 15, 0))
    write_probs(str(d / "g.bgen"), kaa, kab, codes < 0, 8)
    np.savetxt(d / "phenotypes.txt", np.loadtxt(os.path.join(FIX, "normal_y_fam6.txt")))
    return d


def test_routing(mih, pheno_bgen, monkeypatch):
    d = pheno_bgen
    path = str(d / "g.bgen")
    old_x = old_matrix(path)
    kw = dict(phenotypes=str(d / "phenotypes.txt"), summaryfile=str(d / "s.txt"), betafile=str(d / "b.txt"))

    def not_streamed(*a, **k):
        raise G._NotStreamable("the old reader")
    with monkeypatch.context() as mp:                       # the fit on the old reader's DosageMatrix
        mp.setattr(G, "read_bgen_device", not_streamed)
        old = mih.iht(path, 9, mih.Normal, **kw)

    def no(*a, **k):
        raise AssertionError("read_bgen called for a streamable file")
    monkeypatch.setattr(G, "read_bgen", no)
    x = mih.parse_genotypes(path)[0]
    assert x.denom == old_x.denom == 17                     # numerators 15, 255, 510 over 255: all multiples of 15
    assert_same(x, old_x)
    new = mih.iht(path, 9, mih.Normal, **kw)
    assert new.iter == old.iter and np.array_equal(new.beta, old.beta) and new.logl == old.logl and new.σg == old.σg
    assert np.count_nonzero(new.beta) == 9 and np.array_equal(np.asarray(new.c), np.asarray(old.c))
    mse = mih.cross_validate(path, mih.Normal, path=range(8, 11), q=3, phenotypes=str(d / "phenotypes.txt"),
                             cv_summaryfile=str(d / "cv.txt"), folds=mih.hash_folds(1000, 3), verbose=False)
    assert len(mse) == 3 and np.all(np.isfinite(mse))


def test_fallback_to_read_bgen(mih, tmp_path):
    rng = np.random.default_rng(13)
    n = 200
    r = rng.standard_normal(n)
    # 16-bit fractional dosages: today's DenseMatrix of the standardized values, with its warning
    kaa, kab, miss = probs(rng, n, 5, 16)
    write_probs(str(tmp_path / "f16.bgen"), kaa, kab, miss, 16)
    # the bit depth changes at variant 3 (8, then 10 bits); a 20-bit file (both hard calls: on the grid 1 / 1)
    g = rng.integers(0, 3, (n, 6))
    blocks = [genotype_block(np.where(g[:, j] == 0, (1 << b) - 1, 0), np.where(g[:, j] == 1, (1 << b) - 1, 0), miss[:, 0], b)
              for j, b in enumerate((8, 8, 10, 10, 8, 10))]
    write_blocks(str(tmp_path / "mixed.bgen"), n, blocks)
    kaa, kab, miss = probs(rng, n, 4, 20, hard=True)
    write_probs(str(tmp_path / "b20.bgen"), kaa, kab, miss, 20, comp=0)
    for name in ("f16.bgen", "mixed.bgen", "b20.bgen"):
        path = str(tmp_path / name)
        with pytest.raises(ArgumentError):
            G.read_bgen_device(path)
        with warnings.catch_warnings(record=True) as w_new:
            warnings.simplefilter("always")
            new = mih.parse_genotypes(path)
        cols, *meta = G.read_bgen(path)
        with warnings.catch_warnings(record=True) as w_old:
            warnings.simplefilter("always")
            num, val = G.genotype_values(cols)
        assert [str(x.message) for x in w_new] == [str(x.message) for x in w_old]
        assert list(new[1:]) == meta
        if num is None:
            assert name == "f16.bgen" and isinstance(new[0], mih.DenseMatrix) and len(w_new) == 1
            assert np.array_equal(new[0].xtv(r), mih.DenseMatrix(val).xtv(r))
        else:
            assert name != "f16.bgen"
            assert_same(new[0], mih.DosageMatrix(num, val))


def refusal(path):
    with pytest.raises(ArgumentError) as old:
        G.read_bgen(path)
    with pytest.raises(ArgumentError) as new:
        G.read_bgen_device(path)
    assert str(new.value) == str(old.value)
    with pytest.raises(ArgumentError) as routed:
        M.parse_genotypes(path)
    assert str(routed.value) == str(old.value)
    return str(old.value)


def test_refusals(mih, tmp_path):
    rng = np.random.default_rng(17)
    n, p = 120_000, 100                                   # several runs of blocks, several workers
    kaa, kab, miss = probs(rng, n, p, 8, missing=0.01)
    cols = [(kaa[:, j], kab[:, j], miss[:, j]) for j in range(p)]

    def file(name, **bad):
        blocks = [genotype_block(*c, 8) for c in cols]
        for j, kw in bad.items():
            j = int(j[1:])
            a, b_, m = (x.copy() for x in cols[j])
            kw = dict(kw)
            if kw.pop("sum", False):
                m[77], a[77], b_[77] = False, 200, 100
            pl = None
            if kw.pop("ploidy", False):
                pl = np.full(n, 2); pl[n - 3] = 3
            blocks[j] = genotype_block(a, b_, m, kw.pop("nbits", 8), ploidy=pl, **kw)
        path = str(tmp_path / name)
        write_blocks(path, n, blocks, comp=1, level=1)
        return path

    assert refusal(file("phased.bgen", v40=dict(phased=1))).endswith("marker 41: phased BGEN data is not supported")
    assert refusal(file("ploidy.bgen", v70=dict(ploidy=True))).endswith("marker 71: ploidy other than 2 is not supported")
    assert refusal(file("sum.bgen", v56=dict(sum=True))).endswith("marker 57: probabilities sum above 1")
    assert refusal(file("n.bgen", v9=dict(n_field=n + 1))).endswith("marker 10: genotype block disagrees with the header")
    assert refusal(file("b0.bgen", v88=dict(nbits=0))).endswith("marker 89: 0 bits per probability")
    # two defects: the first in file order is named, whichever side (host or device) finds it
    assert refusal(file("two1.bgen", v12=dict(ploidy=True), v30=dict(phased=1))).endswith("marker 13: ploidy other than 2 is not supported")
    assert refusal(file("two2.bgen", v12=dict(phased=1), v90=dict(sum=True))).endswith("marker 13: phased BGEN data is not supported")
    assert refusal(file("two3.bgen", v80=dict(pminmax=(2, 3)), v95=dict(sum=True))).endswith("marker 81: ploidy other than 2 is not supported")
    # one block with a sample of ploidy 3 and the phased flag: read_bgen checks the ploidy first
    assert refusal(file("same.bgen", v50=dict(ploidy=True, phased=1))).endswith("marker 51: ploidy other than 2 is not supported")


def test_bounded_host_memory(mih, tmp_path):
    path = str(tmp_path / "m.bgen")
    write_imputed(path, 200_000, 2_000, 8, seed=9)
    script = tmp_path / "child.py"
    script.write_text(f"""
import json, sys
import numpy as np
sys.path.insert(0, {ROOT!r})
import mendeliht_amd as m
from mendeliht_amd import genotypes as G

def kb(key):                                          # this process's own counters (ru_maxrss would carry the parent's across exec)
    return int([ln for ln in open('/proc/self/status') if ln.startswith(key + ':')][0].split()[1])
m.DosageMatrix(np.zeros((64, 2), np.uint16), 1).export()   # the runtime is up: device, streams, first copies both ways
rss0 = kb('VmRSS')
x = G.read_bgen_device({path!r})[0]
print(json.dumps(dict(grow_mb=(kb('VmHWM') - rss0) / 1024, p=x.p, denom=x.denom)))
""")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["p"] == 2000 and got["denom"] == 255
    assert got["grow_mb"] <= 768, got


def test_gcd_across_chunks(mih, tmp_path):
    """a column's divisor is the gcd over all its chunks of 8192 samples: hard calls everywhere but ONE fractional sample in the
    last chunk (or the first) make the whole column 1/255, not 1/1 in the other chunks"""
    rng = np.random.default_rng(23)
    n, p = 20_000, 4
    kaa, kab, miss = probs(rng, n, p, 8, hard=True, missing=0.01)
    for j, i in ((0, n - 5), (1, 3), (2, 16_390)):
        kaa[i, j], kab[i, j], miss[i, j] = 100, 51, False                       # num = 510 - 200 - 51 = 259, prime to 255
    path = str(tmp_path / "c.bgen")
    write_probs(path, kaa, kab, miss, 8)
    x = streamed(path)
    assert x.denom == 255
    assert_same(x, old_matrix(path))
    assert set(np.unique(x.export()[:, 3])) <= {0, 255, 510, 0xFFFF}           # column 3: hard calls on the common grid


def test_16_bit_columns_whose_common_grid_is_too_fine(mih, tmp_path):
    """16-bit columns on the grids 1/21845 (g_j = 3) and 1/13107 (g_j = 5): each fits, their common grid 1/65535 does not --
    read_bgen's path (a Float64 DenseMatrix with its warning), found by the gcd of the columns decoded so far"""
    rng = np.random.default_rng(29)
    n, p = 300, 6
    kaa, kab, miss = probs(rng, n, p, 16, hard=True)
    for j in range(p):                                   # num = 2 * 65535 - k_AB: 65541 = 3 * 21847 (g_j = 3), 65555 = 5 * 13111 (5)
        kaa[7, j], kab[7, j], miss[7, j] = 0, 65529 if j % 2 == 0 else 65515, False
    path = str(tmp_path / "g35.bgen")
    write_probs(path, kaa, kab, miss, 16)
    with pytest.raises(ArgumentError, match="finer than 1/32767"):
        G.read_bgen_device(path)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        x = mih.parse_genotypes(path)[0]
    assert isinstance(x, mih.DenseMatrix) and any("dense Float64" in str(m.message) for m in w)
    for a in range(0, p, 2):                             # two neighbouring columns alone stream; each grid by itself
        assert G.read_bgen_device(path, variants=range(a, a + 1))[0].denom == 21845
        assert G.read_bgen_device(path, variants=range(a + 1, a + 2))[0].denom == 13107


def test_offsets_that_skip_variants(mih, tmp_path):
    """the C ABI with every third block of an uncompressed file (runs whose offsets are far apart are read block by block):
    those columns of the whole read, nothing else"""
    import ctypes as C
    path = str(tmp_path / "gap.bgen")
    write_imputed(path, 200_000, 90, 8, seed=31, comp=0)
    whole = streamed(path)
    idx = G.bgen_index(path)
    pick = np.arange(0, 90, 3)
    offs = np.ascontiguousarray(idx.offsets[pick])
    h, den, bb, bw = C.c_void_p(None), C.c_int32(0), C.c_int64(-1), C.c_int32(0)
    rc = mih.lib().mih_dosage_create_bgen(os.fsencode(path), idx.n, pick.size, offs.ctypes.data_as(C.c_void_p), 0, 0, 0,
                                          C.byref(h), C.byref(den), C.byref(bb), C.byref(bw))
    assert rc == 0 and bw.value == 0
    x = mih.DosageMatrix(None, den.value, _handle=h)
    x.regrid(whole.denom)
    assert np.array_equal(x.export(), whole.export()[:, pick])
    assert np.array_equal(x.mu_sigma()[0], whole.mu_sigma()[0][pick])
