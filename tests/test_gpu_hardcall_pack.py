"""Hard calls packed into the 2-bit matrix on the device (k_pack_u16; mih_snp_builder_*, mih_snp_create_dosage,
mih_snp_create_vcf; DosageMatrix.to_snp, SnpBuilder, read_vcf_snp, read_bgen_snp, two_bit=True).  The yardstick is exact: for the
same genotypes the packed handle equals the one mih_snp_create builds from the .bed encoding, bit for bit -- export_bed, mu and
sinv, X'r single and fused, X v, one fit -- at the shapes where the pack kernel changes path: the u16 pad (8 rows), the dword
(16), the half record (64), the tile (128), a wave's four tiles (512) and a workgroup's sixteen (2048) per trip, one workgroup's
row span (64 block pairs of 128 rows = 8192), and column counts around the group of 32."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

from conftest import FIX, GOLD, make_bed
from test_genotype_readers_cpu import bed_codes, write_bgen, write_bgen_probs, write_vcf
from vcf_files import GT_TOKENS, containers, gzip_bytes, random_tokens, vcf_text, write

from mendeliht_amd import genotypes as G

pytestmark = pytest.mark.gpu

MISSING = 0xFFFF


def codes_of(bed, n):
    """n x p ALT allele counts (-1 missing) of PLINK columns (p, ceil(n/4))."""
    two = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n]
    return np.array([0, -1, 1, 2], dtype=np.int64)[two].T.copy()


def bed_of(codes):
    """The .bed columns of n x p allele counts: 0 -> 00, 1 -> 10, 2 -> 11, missing -> 01."""
    n, p = codes.shape
    code = np.zeros((p, (n + 3) // 4 * 4), dtype=np.uint8)
    code[:, :n] = np.array([1, 0, 2, 3], dtype=np.uint8)[codes.T + 1]
    return (code[:, 0::4] | (code[:, 1::4] << 2) | (code[:, 2::4] << 4) | (code[:, 3::4] << 6)).astype(np.uint8)


def numerators(codes, unit=1):
    return np.where(codes < 0, MISSING, codes * unit).astype(np.uint16)


def edge_codes(n, p, seed):
    """5 % missing; where there is room, a monomorphic-0, a monomorphic-2 and an all-missing column."""
    rng = np.random.default_rng(seed)
    codes = codes_of(make_bed(rng, n, p, missing_rate=0.05), n)
    if p >= 31:
        codes[:, 3], codes[:, 17], codes[:, p - 2] = 0, 2, -1
    return codes


def from_bed(mih, codes):
    return mih.SnpLinAlg(bed_of(codes), codes.shape[0], center=True, scale=True, impute=True)


def outcome(fn):
    """What a call gives: its result's arrays, or the error it raises (an all-missing column is whatever the library makes of it)."""
    try:
        r = fn()
    except Exception as e:       # noqa: BLE001 -- compared, not swallowed
        return ("raised", type(e).__name__, str(e))
    return ("fitted", r.iter, np.array(r.beta), np.array(r.c), np.array(r.trace["logl"]))


def assert_same_handle(mih, got, want, fit=False):
    n, p = want.shape
    assert isinstance(got, mih.SnpLinAlg) and got.shape == (n, p)
    assert (got.center, got.scale, got.impute) == (want.center, want.scale, want.impute)
    assert np.array_equal(got.export_bed(), want.export_bed())
    for a, b in zip(got.mu_sigma(), want.mu_sigma()):
        assert np.array_equal(a, b, equal_nan=True)
    rng = np.random.default_rng(n * 131 + p)
    R = rng.standard_normal((n, 5))
    assert np.array_equal(got.xtv(R[:, 0]), want.xtv(R[:, 0]), equal_nan=True)
    assert np.array_equal(got.xtv(R), want.xtv(R), equal_nan=True)
    idx = np.sort(rng.choice(p, min(p, 4), replace=False))
    val = rng.standard_normal(idx.size)
    assert np.array_equal(got.xv_sparse(idx, val), want.xv_sparse(idx, val), equal_nan=True)
    if fit:
        y = R[:, 1] + 0.5
        a, b = (outcome(lambda x=x: mih.fit_iht(y, x, None, k=min(3, p), verbose=False)) for x in (got, want))
        assert a[:2] == b[:2], (a, b)
        if a[0] == "raised":
            assert a == b
        else:
            for u, v in zip(a[2:], b[2:]):
                assert np.array_equal(u, v, equal_nan=True)


# ---- 1. the whole-handle pack at edge shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 511, 513, 2047, 2049, 8191, 8192, 8193])
def test_whole_handle_pack_at_edge_shapes(mih, n):
    for p in (1, 31, 32, 33, 70):
        codes = edge_codes(n, p, 1000 * n + p)
        got = mih.DosageMatrix(numerators(codes), 1).to_snp()
        assert_same_handle(mih, got, from_bed(mih, codes), fit=n >= 257)


# ---- 2. the hard-call unit -----------------------------------------------------------------------------------------------------
def test_hard_call_unit(mih):
    codes = edge_codes(257, 70, 5)
    want = from_bed(mih, codes)
    assert_same_handle(mih, mih.DosageMatrix(numerators(codes), 1).to_snp(), want)
    assert_same_handle(mih, mih.DosageMatrix(numerators(codes, 2), 2).to_snp(), want)
    assert_same_handle(mih, mih.DosageMatrix(numerators(codes), 1).regrid(3).to_snp(), want)
    num = numerators(np.where(codes < 0, 0, codes), 2)
    num[5, 40] = 1
    num[9, 55] = 1
    d = mih.DosageMatrix(num, 2)
    with pytest.raises(mih.api.ArgumentError, match=r"column 41\b"):
        d.to_snp()
    h, bad = C.c_void_p(None), C.c_int64(-7)
    assert mih.lib().mih_snp_create_dosage(d._h, 1, 1, 1, 64, C.byref(h), C.byref(bad)) == 2         # MIH_BAD_ARG
    assert bad.value == 40 and not h.value


# ---- 3. the builder -------------------------------------------------------------------------------------------------------------
def test_builder(mih):
    codes = edge_codes(257, 70, 6)
    whole = mih.DosageMatrix(numerators(codes), 1).to_snp()
    assert_same_handle(mih, whole, from_bed(mih, codes))
    starts = np.cumsum([0, 5, 27, 32, 1])                          # panels of 5, 27, 32, 1 and 5 columns
    panels = [(int(a), int(b)) for a, b in zip(starts, list(starts[1:]) + [70])]
    assert [b - a for a, b in panels] == [5, 27, 32, 1, 5]
    order = np.random.default_rng(3).permutation(len(panels))
    assert list(order) != sorted(order)
    b = mih.SnpBuilder(257, 70)
    for i in order:
        a, e = panels[i]
        b.add(a, mih.DosageMatrix(numerators(codes[:, a:e]), 1))
    assert_same_handle(mih, b.finish(), whole, fit=True)

    def panel(a, e, rows=257):
        return mih.DosageMatrix(numerators(codes[:rows, a:e]), 1)

    b = mih.SnpBuilder(257, 70)
    b.add(0, panel(0, 40))
    with pytest.raises(mih.api.ArgumentError, match=r"column 36\b"):      # columns 35 .. 39 are there already
        b.add(35, panel(35, 70))
    assert b.bad_col == 35
    with pytest.raises(mih.api.ArgumentError, match=r"column 41\b"):      # a gap: columns 40 .. 49
        b.add(50, panel(50, 70)).finish()
    with pytest.raises(mih.api.DimensionMismatch):
        b.add(40, panel(40, 50, rows=256))
    with pytest.raises(mih.api.DimensionMismatch):
        b.add(65, panel(40, 50))                                          # past the last column
    b.add(40, panel(40, 50))
    assert_same_handle(mih, b.finish(), whole)                            # the refusals left the builder as it was
    with pytest.raises(mih.api.ArgumentError):
        b.finish()                                                        # it is closed
    bad = numerators(codes[:, :10], 3)
    bad[200, 4] = 2
    b = mih.SnpBuilder(257, 70)
    with pytest.raises(mih.api.ArgumentError, match=r"column 25\b"):
        b.add(20, mih.DosageMatrix(bad, 3))
    assert b.bad_col == 24
    with pytest.raises(mih.api.ArgumentError):                            # nothing after a refused numerator may be used
        b.add(0, panel(0, 5))
    b.close()


# ---- 4. VCF streamed -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gt_vcf(tmp_path_factory):
    d = tmp_path_factory.mktemp("gt")
    data = vcf_text(random_tokens(np.random.default_rng(41), 300, 70, GT_TOKENS[:6], missing=0.05))
    files = containers(d, "gt", data) + [("gzip2", write(d / "gt_gz2.vcf.gz", gzip_bytes(data, 2)))]
    cols = G.read_vcf(files[0][1])
    num, den = G.genotype_values(cols[0])
    assert den == 1
    return files, np.where(num == MISSING, -1, num.astype(np.int64)), cols[1:]


def test_vcf_streamed(mih, gt_vcf):
    files, codes, meta = gt_vcf
    assert (codes < 0).any() and set(np.unique(codes)) == {-1, 0, 1, 2}
    want = from_bed(mih, codes)
    for tag, path in files:
        for kw in (dict(chunk_bytes=4096), {}, dict(chunk_bytes=4096, threads=1)):
            got = G.read_vcf_snp(path, **kw)
            assert_same_handle(mih, got[0], want)
            assert tuple(got[1:]) == tuple(meta), tag
    dev = G.read_vcf_device(files[0][1])
    assert_same_handle(mih, dev[0].to_snp(), want, fit=True)
    part = G.read_vcf_snp(files[3][1], variants=range(13, 57), chunk_bytes=4096)
    assert_same_handle(mih, part[0], from_bed(mih, codes[:, 13:57]))
    assert tuple(part[1:]) == tuple(G.read_vcf_device(files[3][1], variants=range(13, 57))[1:])
    x = mih.parse_genotypes(files[0][1])[0]
    assert isinstance(x, mih.DosageMatrix) and x.denom == 1               # without two_bit: today's behaviour
    x = mih.parse_genotypes(files[0][1], two_bit=True)[0]
    assert_same_handle(mih, x, want)


def test_vcf_ds_hard_calls_and_refusal(mih, gt_vcf, tmp_path):
    codes = gt_vcf[1]
    spell = np.array([".", "0", "1.0", "2.000"])
    toks = [list(spell[codes[:, j] + 1]) for j in range(codes.shape[1])]
    want = from_bed(mih, codes)
    path = write(tmp_path / "ds.vcf", vcf_text(toks, "DS"))
    for kw in (dict(chunk_bytes=4096), {}):
        assert_same_handle(mih, G.read_vcf_snp(path, dosage=True, **kw)[0], want)
    toks[40][123] = "0.5"
    toks[55][7] = "1.5"
    for tag, bad in containers(tmp_path, "half", vcf_text(toks, "DS")):
        for kw in (dict(chunk_bytes=4096), {}):
            with pytest.raises(mih.api.ArgumentError, match=r"record 41\b") as e:
                G.read_vcf_snp(bad, dosage=True, **kw)
            assert not isinstance(e.value, G._NotStreamable), tag
    with pytest.raises(mih.api.ArgumentError, match=r"record 41\b"):
        mih.parse_genotypes(bad, dosage=True, two_bit=True)                # no silent DosageMatrix
    assert isinstance(mih.parse_genotypes(bad, dosage=True)[0], mih.DosageMatrix)
    toks[40][123] = "0/1"                                                 # outside the streamed grammar: the reader's own words
    with pytest.raises(G._NotStreamable, match=r"record 41\b"):
        mih.parse_genotypes(write(tmp_path / "odd.vcf", vcf_text(toks, "DS")), dosage=True, two_bit=True)


# ---- 5. BGEN by panels -----------------------------------------------------------------------------------------------------------
def test_bgen_by_panels(mih, tmp_path):
    codes = bed_codes(os.path.join(FIX, "normal.bed"), 1000)[:, :200]
    want = from_bed(mih, codes)
    path = os.path.join(GOLD, "normal_head.bgen")
    dev = G.read_bgen_device(path)
    for kw in (dict(panel=64), {}):
        got = G.read_bgen_snp(path, **kw)
        assert_same_handle(mih, got[0], want)
        assert tuple(got[1:]) == tuple(dev[1:])
    part = G.read_bgen_snp(path, variants=range(30, 101), panel=64)
    assert_same_handle(mih, part[0], from_bed(mih, codes[:, 30:101]))
    assert tuple(part[1:]) == tuple(G.read_bgen_device(path, variants=range(30, 101))[1:])
    small = edge_codes(50, 60, 9)
    write_bgen(tmp_path / "hard.bgen", small, 1, nbits=8)
    assert_same_handle(mih, G.read_bgen_snp(tmp_path / "hard.bgen", panel=16)[0], from_bed(mih, small))
    kaa, kab = np.where(small == 0, 255, 0), np.where(small == 1, 255, 0)
    kaa[3, 41], kab[3, 41] = 128, 127                                     # one fractional probability: a dosage of 127 / 255
    write_bgen_probs(tmp_path / "frac.bgen", kaa, kab, small < 0, 8)
    for kw in (dict(panel=16), {}):
        with pytest.raises(mih.api.ArgumentError, match=r"marker 42\b"):
            G.read_bgen_snp(tmp_path / "frac.bgen", **kw)
    with pytest.raises(mih.api.ArgumentError, match=r"marker 42\b"):
        mih.parse_genotypes(str(tmp_path / "frac.bgen"), two_bit=True)


# ---- 6. the reference's "PLINK = VCF = BGEN" testset, exact ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def normal_files(tmp_path_factory):
    """data/normal as a PLINK trio, a GT VCF and an 8-bit BGEN with hard calls, all 10 000 variants (written from normal.bed)."""
    d = tmp_path_factory.mktemp("normal")
    n = 1000
    codes = bed_codes(os.path.join(FIX, "normal.bed"), n)
    shutil.copyfile(os.path.join(FIX, "normal.bed"), d / "normal.bed")
    y = np.loadtxt(os.path.join(FIX, "normal_y_fam6.txt"))
    with open(d / "normal.fam", "w") as f:
        for i, v in enumerate(y):
            f.write(f"{i + 1}\t{i + 1}\t0\t0\t1\t{float(v)!r}\n")
    with open(d / "normal.bim", "w") as f:
        for j in range(codes.shape[1]):
            f.write(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n")
    np.savetxt(d / "phenotypes.txt", y)
    write_vcf(d / "normal.vcf.gz", codes, 1)
    write_bgen(d / "normal.bgen", codes, 1, nbits=8)
    return d


def test_reference_testset_exact(mih, normal_files):
    """test/wrapper_test.jl:184-202 with two_bit=True: the three containers give the same fit, with ==."""
    d = normal_files
    kw = dict(phenotypes=str(d / "phenotypes.txt"), summaryfile=str(d / "s.txt"))
    ref = mih.iht(str(d / "normal"), 10, mih.Normal, betafile=str(d / "b0.txt"), **kw)
    for src in ("normal.vcf.gz", "normal.bgen"):
        res = mih.iht(str(d / src), 10, mih.Normal, betafile=str(d / "b1.txt"), two_bit=True, **kw)
        assert res.iter == ref.iter
        assert np.all(res.beta == ref.beta) and np.all(res.c == ref.c)
        assert res.logl == ref.logl
        assert np.array_equal(res.trace["logl"], ref.trace["logl"])
        rows = open(d / "b1.txt").read().splitlines()
        assert rows[0] == "chr\tpos\tSNPid\tref\talt\tEstimated_beta" and len(rows) == 10_001
    x = mih.parse_genotypes(str(d / "normal.bgen"), two_bit=True)[0]
    assert isinstance(x, mih.SnpLinAlg) and x.shape == (1000, 10_000)
    mse = mih.cross_validate(str(d / "normal.vcf.gz"), mih.Normal, path=range(8, 12), q=3, two_bit=True, cv_summaryfile=str(d / "cv.txt"),
                             phenotypes=str(d / "phenotypes.txt"), folds=mih.hash_folds(1000, 3), verbose=False)
    want = mih.cross_validate(str(d / "normal"), mih.Normal, path=range(8, 12), q=3, cv_summaryfile=str(d / "cv.txt"),
                              phenotypes=str(d / "phenotypes.txt"), folds=mih.hash_folds(1000, 3), verbose=False)
    assert np.array_equal(mse, want)


def test_golden_k7_through_two_bit_vcf(mih, normal_files):
    """The reference's recorded run (docs/src/man/examples.md:230-267) reproduced from a VCF input packed into 2 bits."""
    d = normal_files
    g = json.load(open(os.path.join(GOLD, "golden_normal_k7.json")))
    res = mih.iht(str(d / "normal.vcf.gz"), 7, mih.Normal, phenotypes=str(d / "phenotypes.txt"), two_bit=True,
                  covariates=os.path.join(FIX, "covariates.txt"), summaryfile=str(d / "s.txt"), betafile=str(d / "b.txt"))
    assert res.iter == g["iterations"]
    assert list(np.flatnonzero(res.beta) + 1) == g["positions_1based"]
    np.testing.assert_allclose(res.trace["logl"], g["logl"], rtol=1e-9)
