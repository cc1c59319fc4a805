"""VCF / BGEN readers of parse_genotypes (no GPU): the committed excerpts of the reference's data/normal.{vcf.gz,bgen} decode to
normal.bed exactly; round trips through the writers below (DS with 1-4 decimals, 8- and 10-bit BGEN, missing entries); the
grid and its gcd reduction; the Float64 fallback; every refusal."""
import gzip
import math
import os
import struct
import warnings
import zlib
from fractions import Fraction

import numpy as np
import pytest

from conftest import FIX, GOLD

from mendeliht_amd import genotypes as G
from mendeliht_amd.api import ArgumentError


def bed_codes(path, n):
    """n x p ALT (A2) allele counts of a PLINK .bed, -1 where missing."""
    raw = np.fromfile(path, dtype=np.uint8, offset=3).reshape(-1, (n + 3) // 4)
    two = np.stack([(raw >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(raw.shape[0], -1)[:, :n]
    return np.array([0, -1, 1, 2], dtype=np.int64)[two].T.copy()


def write_vcf(path, num, den, decimals=None, alt=None):
    """num: n x p numerators (-1 missing) over den; GT when den == 1 and decimals is None, else DS with `decimals` digits."""
    n, p = num.shape
    lines = ["##fileformat=VCFv4.2\n", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"s{i + 1}" for i in range(n)) + "\n"]
    gt = {-1: "./.", 0: "0/0", 1: "0/1", 2: "1/1"}
    for j in range(p):
        if decimals is None:
            vals, fmt = [gt[int(v)] for v in num[:, j]], "GT"
        else:
            vals, fmt = ["." if v < 0 else f"{v / den:.{decimals}f}" for v in num[:, j]], "DS"
        lines.append(f"{1 + j // 100}\t{10 * j + 1}\trs{j + 1}\tA\t{alt or 'G'}\t.\tPASS\t.\t{fmt}\t" + "\t".join(vals) + "\n")
    data = "".join(lines).encode()
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        open(path, "wb").write(data)


def write_bgen_probs(path, kaa, kab, miss, nbits, comp=1, layout=2, phased=0, ploidy=2, nalleles=2, samples=True):
    """BGEN v1.2 with the stored probabilities (k_AA, k_AB) / (2^nbits - 1) of each sample (n x p integer arrays)."""
    n, p = kaa.shape
    ids = [f"s{i + 1}".encode() for i in range(n)]
    sblock = struct.pack("<II", 8 + sum(2 + len(s) for s in ids), n) + b"".join(struct.pack("<H", len(s)) + s for s in ids) if samples else b""
    flags = comp | (layout << 2) | ((1 << 31) if samples else 0)
    header = struct.pack("<III", 20, p, n) + b"bgen" + struct.pack("<I", flags)
    out = [struct.pack("<I", len(header) + len(sblock)), header, sblock]
    for j in range(p):
        def s16(x):
            return struct.pack("<H", len(x)) + x.encode()
        v = s16(f"v{j + 1}") + s16(f"rs{j + 1}") + s16(str(1 + j // 100)) + struct.pack("<IH", 10 * j + 1, nalleles)
        v += b"".join(struct.pack("<I", 1) + a.encode() for a in "ACGT"[:nalleles])
        pl = np.full(n, ploidy, np.uint8) | np.where(miss[:, j], 0x80, 0).astype(np.uint8)
        vals = np.stack([np.where(miss[:, j], 0, kaa[:, j]), np.where(miss[:, j], 0, kab[:, j])], axis=1).reshape(-1).astype(np.uint64)
        bits = ((vals[:, None] >> np.arange(nbits, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(-1)
        g = struct.pack("<IHBB", n, 2, ploidy, ploidy) + pl.tobytes() + bytes([phased, nbits]) + np.packbits(bits, bitorder="little").tobytes()
        if comp == 1:
            z = zlib.compress(g)
            v += struct.pack("<II", len(z) + 4, len(g)) + z
        else:
            v += struct.pack("<I", len(g)) + g
        out.append(v)
    open(path, "wb").write(b"".join(out))


def write_bgen(path, codes, den, nbits=8, **kw):
    """Hard calls (den == 1, -1 missing) as B-bit probabilities."""
    assert den == 1
    full = (1 << nbits) - 1
    miss = codes < 0
    write_bgen_probs(path, np.where(codes == 0, full, 0), np.where(codes == 1, full, 0), miss, nbits, **kw)


def test_golden_excerpts_decode_to_bed():
    codes = bed_codes(os.path.join(FIX, "normal.bed"), 1000)[:, :200]
    cols, samples, chrom, pos, ids, ref, alt = G.read_vcf(os.path.join(GOLD, "normal_head.vcf.gz"))
    num, den = G.genotype_values(cols)
    assert den == 1 and np.array_equal(num.astype(np.int64), np.where(codes < 0, 0xFFFF, codes))
    assert len(samples) == 1000 and len(pos) == 200 and isinstance(pos[0], int)
    cols, samples, chrom, pos, ids, ref, alt = G.read_bgen(os.path.join(GOLD, "normal_head.bgen"), os.path.join(GOLD, "normal.sample"))
    num2, den2 = G.genotype_values(cols)
    assert den2 == 1 and np.array_equal(num2, num)
    assert samples[:3] == ["1", "2", "3"] and ids[:2] == ["snp1", "snp2"] and (ref[0], alt[0]) == ("1", "2")
    assert len(cols) == 200 and all(q == 65535 for _, q in cols)           # 16-bit probabilities, hard calls


@pytest.mark.parametrize("decimals", [1, 2, 3, 4])
def test_vcf_ds_roundtrip(tmp_path, decimals):
    rng = np.random.default_rng(decimals)
    den = 10 ** decimals
    num = rng.integers(0, 2 * den + 1, (30, 12))
    num[rng.random(num.shape) < 0.1] = -1
    write_vcf(tmp_path / "d.vcf", num, den, decimals)
    cols = G.read_vcf(tmp_path / "d.vcf", dosage=True)[0]
    u16, q = G.genotype_values(cols)
    assert q == den                                                   # generic data: nothing to reduce
    want = [[None if v < 0 else Fraction(int(v), den) for v in num[:, j]] for j in range(12)]
    got = [[None if v == 0xFFFF else Fraction(int(v), q) for v in u16[:, j]] for j in range(12)]
    assert got == want


def test_denominator_reduction_and_gt(tmp_path):
    num = np.array([[0, 50, 100], [150, 200, -1], [50, 0, 200]])      # halves written with 2 decimals
    write_vcf(tmp_path / "h.vcf.gz", num, 100, 2)
    u16, q = G.genotype_values(G.read_vcf(tmp_path / "h.vcf.gz", dosage=True)[0])
    assert q == 2 and u16.tolist() == [[0, 1, 2], [3, 4, 0xFFFF], [1, 0, 4]]
    codes = np.array([[0, 1], [2, -1], [1, 1]])
    write_vcf(tmp_path / "g.vcf", codes, 1)
    u16, q = G.genotype_values(G.read_vcf(tmp_path / "g.vcf")[0])
    assert q == 1 and u16.tolist() == [[0, 1], [2, 0xFFFF], [1, 1]]
    d = np.array([[0.0, 1 / 255, np.nan], [2.0, 254 / 255, 1.0]])
    u16, q = G.dosage_grid(d)
    assert q == 255 and u16.tolist() == [[0, 1, 0xFFFF], [510, 254, 255]]
    assert G.dosage_grid(np.array([[0.5, 1.5], [2.0, np.nan]]))[1] == 2
    with pytest.raises(ArgumentError):
        G.dosage_grid(np.array([[0.123456789]]))
    with pytest.raises(ArgumentError):
        G.dosage_grid(np.array([[2.5]]))


@pytest.mark.parametrize("nbits,comp", [(8, 1), (10, 0), (10, 1)])
def test_bgen_roundtrip(tmp_path, nbits, comp):
    rng = np.random.default_rng(nbits + comp)
    full = (1 << nbits) - 1
    n, p = 40, 9
    kaa = rng.integers(0, full + 1, (n, p))
    kab = (rng.random((n, p)) * (full - kaa + 1)).astype(np.int64)
    miss = rng.random((n, p)) < 0.1
    write_bgen_probs(tmp_path / "x.bgen", kaa, kab, miss, nbits, comp=comp)
    cols, samples, chrom, pos, ids, ref, alt = G.read_bgen(tmp_path / "x.bgen")
    assert samples[:2] == ["s1", "s2"] and (ref[0], alt[0]) == ("A", "C") and pos[1] == 11
    u16, q = G.genotype_values(cols)
    assert q == full
    kbb = full - kaa - kab
    want = np.where(miss, 0xFFFF, 2 * kbb + kab)
    assert np.array_equal(u16.astype(np.int64), want)


def test_float64_fallback_keeps_the_values(tmp_path):
    rng = np.random.default_rng(5)
    full = 65535
    kaa = rng.integers(0, full + 1, (25, 4))
    kab = (rng.random((25, 4)) * (full - kaa + 1)).astype(np.int64)
    miss = np.zeros((25, 4), bool); miss[3, 1] = True
    write_bgen_probs(tmp_path / "f.bgen", kaa, kab, miss, 16)
    cols = G.read_bgen(tmp_path / "f.bgen")[0]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        num, X = G.genotype_values(cols)
    assert num is None and any("dense Float64" in str(x.message) for x in w)
    d = np.where(miss, np.nan, (2 * (full - kaa - kab) + kab) / full)
    np.testing.assert_array_equal(X, G.standardize_dosages(d))
    assert X[3, 1] == 0.0
    c = d[:, 0]; m = c.mean(); s = math.sqrt(m * (1 - m / 2))
    np.testing.assert_allclose(X[:, 0], (c - m) / s, rtol=1e-15)


def test_standardize_semantics():
    d = np.array([[0.0, 2.0, np.nan, 1.0], [0.0, np.nan, np.nan, 1.0], [0.0, 2.0, np.nan, 1.0]])
    X = G.standardize_dosages(d)
    assert np.all(X[:, :3] == 0.0)              # monomorphic at 0 and 2 (sigma = 0), all missing
    assert np.all(X[:, 3] == 0.0)               # all hets: sigma > 0, centred to 0


def test_refusals(tmp_path):
    codes = np.array([[0, 1], [2, 1]])
    kaa, kab, miss = np.where(codes == 0, 255, 0), np.where(codes == 1, 255, 0), codes < 0
    for kw, what in ((dict(comp=2), "zstd"), (dict(layout=1), "layout 1"), (dict(phased=1), "phased"),
                     (dict(ploidy=3), "ploidy"), (dict(nalleles=3), "biallelic")):
        write_bgen_probs(tmp_path / "r.bgen", kaa, kab, miss, 8, **kw)
        with pytest.raises(ArgumentError, match=what):
            G.read_bgen(tmp_path / "r.bgen")
    write_vcf(tmp_path / "m.vcf", codes, 1, alt="G,T")
    with pytest.raises(ArgumentError, match="multi-allelic"):
        G.read_vcf(tmp_path / "m.vcf")
    write_vcf(tmp_path / "big.vcf", np.array([[250]]), 100, 2)
    with pytest.raises(ArgumentError, match="above 2"):
        G.read_vcf(tmp_path / "big.vcf", dosage=True)
    write_vcf(tmp_path / "g.vcf", codes, 1)
    with pytest.raises(ArgumentError, match="no DS"):
        G.read_vcf(tmp_path / "g.vcf", dosage=True)
    with pytest.raises(ArgumentError, match="Unrecognized"):
        G.parse_genotypes(str(tmp_path / "nothing.txt"))
