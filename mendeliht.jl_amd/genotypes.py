"""VCF and BGEN genotype readers -- parse_genotypes (src/wrapper.jl:360-485) for the GPU path.

The reference decodes VCF / BGEN genotypes into a dense Matrix{Float64}.  Real dosages sit on a small integer grid (hard
calls: num / 1; VCF DS with q decimals: num / 10^q; BGEN with B-bit probabilities: num / (2^B - 1)), so the readers keep the
exact numerators and one common denominator, reduced by their gcd: with denom <= 32767 the matrix goes to the device as a
DosageMatrix (16 bits per entry, the same values); otherwise as a DenseMatrix of the standardized f64 values, with a warning.
"""
import gzip
import math
import os
import struct
import warnings
import zlib
from fractions import Fraction

import numpy as np

from .api import ArgumentError, DenseMatrix, DimensionMismatch, DosageMatrix, SnpBuilder, SnpLinAlg, _count_lines, _read_bim, _snp_dtype

MAX_DENOM = 32767
MISSING = 0xFFFF


# ---- the grid ----------------------------------------------------------------------------------
def _reduce(num, den):
    """num (int64, -1 = missing) / den reduced by the gcd of den and every numerator."""
    g = den
    for v in np.unique(num[num > 0]):
        g = math.gcd(g, int(v))
        if g == 1:
            break
    if g > 1:
        num = np.where(num >= 0, num // g, -1)
    return num, den // g


def _to_u16(num):
    return np.where(num < 0, MISSING, num).astype(np.uint16)


def dosage_grid(d):
    """Float dosages (NaN = missing) -> (uint16 numerators, denom): the smallest grid among hard calls, up to 4 decimals and
    B <= 15 bit probabilities that holds every value, reduced by the gcd.  ArgumentError if there is none."""
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 2:
        raise DimensionMismatch("dosages must be a matrix")
    ok = ~np.isnan(d)
    v = d[ok]
    if v.size and (v.min() < 0.0 or v.max() > 2.0):
        raise ArgumentError("dosages must lie in [0, 2]")
    for den in sorted({1, 10, 100, 1000, 10000} | {(1 << b) - 1 for b in range(2, 16)}):
        q = v * den
        k = np.rint(q)
        if np.all(np.abs(q - k) <= 1e-7):
            num = np.full(d.shape, -1, dtype=np.int64)
            num[ok] = k.astype(np.int64)
            num, den = _reduce(num, den)
            return _to_u16(num), den
    raise ArgumentError("the dosages sit on no grid num / denom with denom <= 32767 (hard calls, up to 4 decimals, "
                        "B <= 15 bit probabilities): use a DenseMatrix")


def standardize_dosages(d):
    """standardize_genotypes! (wrapper.jl:406-423) in numpy, NaN = missing (imputed by the mean, i.e. 0 after centring)."""
    d = np.array(d, dtype=np.float64)
    for j in range(d.shape[1]):
        c = d[:, j]
        ok = ~np.isnan(c)
        m = c[ok].sum() / ok.sum() if ok.any() else 0.0
        s = math.sqrt(m * (1.0 - m / 2.0))
        c[~ok] = m
        c -= m
        if s > 0:
            c /= s
    return d


def _combine(cols):
    """Columns of (int64 numerators, -1 = missing; denominator) -> (n x p int64 numerators, common denominator) reduced, or
    None when the common denominator is beyond int64 arithmetic."""
    den = 1
    for _, q in cols:
        den = den * q // math.gcd(den, q)
        if den > (1 << 40):
            return None
    num = np.empty((cols[0][0].size if cols else 0, len(cols)), dtype=np.int64, order="F")
    for j, (c, q) in enumerate(cols):
        num[:, j] = np.where(c >= 0, c * (den // q), -1)
    return _reduce(num, den)


def genotype_values(cols):
    """Columns of (numerators, denom) -> (uint16 numerators, denom) on their common reduced grid, or (None, the standardized
    Float64 matrix) with a warning when that grid is finer than 1/32767 (e.g. 16-bit BGEN with fractional probabilities)."""
    got = _combine(cols)
    if got is not None and got[1] <= MAX_DENOM:
        return _to_u16(got[0]), got[1]
    d = np.empty((cols[0][0].size, len(cols)), order="F")
    for j, (c, q) in enumerate(cols):
        d[:, j] = np.where(c >= 0, c / q, np.nan)
    warnings.warn("the genotypes sit on no grid num / denom with denom <= 32767: stored as a dense Float64 matrix "
                  "(8 bytes per entry)", stacklevel=3)
    return None, standardize_dosages(d)


# ---- VCF ---------------------------------------------------------------------------------------
def _gt_count(tok):
    """ALT allele count of a GT value ("0/1", "1|1", "./." missing)."""
    a = tok.replace("|", "/").split("/")
    if "." in a or tok == "":
        return -1
    return sum(x != "0" for x in a)


def _ds_frac(tok):
    if tok in (".", ""):
        return None
    try:
        return Fraction(tok)
    except ValueError:
        raise ArgumentError(f"unreadable DS value {tok!r}") from None


def read_vcf(path, dosage=False):
    """(columns of (numerators, denom), sample ids, chr, pos, ids, ref, alt) of a VCF (`.vcf` or `.vcf.gz`): GT as ALT allele
    counts (denom 1), or the DS field with dosage=True (its decimals exactly)."""
    opener = gzip.open if str(path).endswith(".gz") else open
    field = "DS" if dosage else "GT"
    samples, cols, chrom, pos, ids, ref, alt = None, [], [], [], [], [], []
    with opener(path, "rt") as f:
        for line in f:
            if line.startswith("##"):
                continue
            t = line.rstrip("\n").split("\t")
            if line.startswith("#"):
                samples = t[9:]
                continue
            if samples is None:
                raise ArgumentError(f"{path}: no #CHROM header line")
            if len(t) != 9 + len(samples):
                raise DimensionMismatch(f"{path}: record {len(cols) + 1} has {len(t) - 9} samples, the header {len(samples)}")
            if "," in t[4]:
                raise ArgumentError(f"{path}: record {len(cols) + 1} ({t[2]}) is multi-allelic; only biallelic records are supported")
            fmt = t[8].split(":")
            if field not in fmt:
                raise ArgumentError(f"{path}: record {len(cols) + 1} has no {field} field")
            k = fmt.index(field)
            vals = [s.split(":")[k] if s.count(":") >= k else "." for s in t[9:]]
            if dosage:
                fr = [_ds_frac(v) for v in vals]
                if any(x is not None and x < 0 for x in fr):
                    raise ArgumentError(f"{path}: record {len(cols) + 1} has a negative DS value")
                den = 1
                for x in fr:
                    if x is not None:
                        den = den * x.denominator // math.gcd(den, x.denominator)
                c = np.array([-1 if x is None else x.numerator * (den // x.denominator) for x in fr], dtype=np.int64)
                if (c > 2 * den).any():
                    raise ArgumentError(f"{path}: record {len(cols) + 1} has a DS value above 2")
            else:
                c, den = np.array([_gt_count(v) for v in vals], dtype=np.int64), 1
            cols.append((c, den))
            chrom.append(t[0]); pos.append(int(t[1])); ids.append(t[2]); ref.append(t[3]); alt.append(t[4])
    if samples is None:
        raise ArgumentError(f"{path}: no #CHROM header line")
    return cols, samples, chrom, pos, ids, ref, alt


# ---- BGEN v1.2 ---------------------------------------------------------------------------------
def _u(fmt, b, off):
    if isinstance(b, _FileWindow):
        return b.unpack(fmt, off)
    return struct.unpack_from(fmt, b, off)[0]


class _FileWindow:
    """A file read through a small window (os.pread) that answers what _u and _bgen_str ask of a bytes object: the header walk
    reads each variant's header and at most WINDOW bytes beyond it, not the genotype block that follows (a mapping of the file
    would fault in the pages around every header)."""

    WINDOW = 1024

    def __init__(self, f):
        self.fd, self.size = f.fileno(), os.fstat(f.fileno()).st_size
        self.lo, self.buf = 0, b""

    def _cover(self, lo, hi):
        if not (self.lo <= lo and hi <= self.lo + len(self.buf)):
            self.lo, self.buf = lo, os.pread(self.fd, max(hi - lo, self.WINDOW), lo)
        return lo - self.lo

    def __len__(self):
        return self.size

    def __getitem__(self, sl):
        lo, hi = max(sl.start, 0), min(sl.stop, self.size)
        if hi <= lo:
            return b""
        o = self._cover(lo, hi)
        return self.buf[o:o + hi - lo]

    def unpack(self, fmt, off):
        size = struct.calcsize(fmt)
        o = self._cover(off, off + size)
        return struct.unpack_from(fmt, self.buf, o)[0]


def _bgen_str(b, off, width):
    n = _u("<H" if width == 2 else "<I", b, off)
    return b[off + width:off + width + n].decode(), off + width + n


def _bgen_head(b, path, sample_path):
    """(offset of the first variant block, M, N, compression, sample ids) of a BGEN v1.2 file's header and sample block, with
    read_bgen's checks and messages."""
    off, lh, m, n = _u("<I", b, 0), _u("<I", b, 4), _u("<I", b, 8), _u("<I", b, 12)
    if b[16:20] not in (b"bgen", b"\0\0\0\0"):
        raise ArgumentError(f"{path} is not a BGEN file")
    flags = _u("<I", b, 4 + lh - 4)
    comp, layout = flags & 3, (flags >> 2) & 15
    if comp == 2:
        raise ArgumentError(f"{path}: zstd-compressed BGEN is not supported (compression none or zlib only)")
    if comp not in (0, 1):
        raise ArgumentError(f"{path}: unknown BGEN compression {comp}")
    if layout != 2:
        raise ArgumentError(f"{path}: BGEN layout {layout} is not supported (layout 2 only)")
    samples = None
    if flags >> 31:
        q, pos_ = _u("<I", b, 4 + lh + 4), 4 + lh + 8
        samples = []
        for _ in range(q):
            s, pos_ = _bgen_str(b, pos_, 2)
            samples.append(s)
    if sample_path is None and os.path.isfile(str(path)[:-5] + ".sample"):
        sample_path = str(path)[:-5] + ".sample"
    if sample_path is not None:
        with open(sample_path) as f:
            rows = [ln.split() for ln in f if ln.strip()][2:]       # header and type lines
        samples = [r[0] for r in rows]
    if samples is None:
        samples = [str(i + 1) for i in range(n)]
    if len(samples) != n:
        raise DimensionMismatch(f"{path}: {len(samples)} sample ids for N = {n}")
    return off, m, n, comp, samples


def _bgen_variant(b, p_):
    """The identifying data of the variant block at p_: (rsid, chr, pos, alleles, offset of its genotype block's length)."""
    _vid, p_ = _bgen_str(b, p_, 2)
    rsid, p_ = _bgen_str(b, p_, 2)
    ch, p_ = _bgen_str(b, p_, 2)
    vpos, k = _u("<I", b, p_), _u("<H", b, p_ + 4)
    p_ += 6
    alleles = []
    for _ in range(k):
        a, p_ = _bgen_str(b, p_, 4)
        alleles.append(a)
    return rsid, ch, vpos, alleles, p_


def read_bgen(path, sample_path=None):
    """(columns of (numerators, denom), sample ids, chr, pos, ids, ref, alt) of a BGEN v1.2 file, layout 2, compression none
    or zlib, unphased diploid biallelic: d = (2 k_BB + k_AB) / (2^B - 1), the ALT (second) allele counted as
    second_dosage! does (wrapper.jl:381).  Sample ids from `sample_path` (default: the .sample file beside the .bgen), else
    the file's own sample block, else 1..N."""
    with open(path, "rb") as f:
        b = f.read()
    off, m, n, comp, samples = _bgen_head(b, path, sample_path)
    cols, chrom, pos, ids, ref, alt = [], [], [], [], [], []
    p_ = off + 4
    for v in range(m):
        rsid, ch, vpos, alleles, p_ = _bgen_variant(b, p_)
        if len(alleles) != 2:
            raise ArgumentError(f"{path}: marker {v + 1} of BGEN is not biallelic!")
        clen = _u("<I", b, p_)
        blk = b[p_ + 4:p_ + 4 + clen]
        p_ += 4 + clen
        if comp == 1:
            dlen = _u("<I", blk, 0)
            blk = zlib.decompress(blk[4:])
            if len(blk) != dlen:
                raise ArgumentError(f"{path}: marker {v + 1}: corrupt genotype block")
        nn, kk, pmin, pmax = _u("<I", blk, 0), _u("<H", blk, 4), blk[6], blk[7]
        if nn != n or kk != 2:
            raise ArgumentError(f"{path}: marker {v + 1}: genotype block disagrees with the header")
        ploidy = np.frombuffer(blk, dtype=np.uint8, count=n, offset=8)
        if pmin != 2 or pmax != 2 or ((ploidy & 0x3F) != 2).any():
            raise ArgumentError(f"{path}: marker {v + 1}: ploidy other than 2 is not supported")
        phased, nbits = blk[8 + n], blk[9 + n]
        if phased:
            raise ArgumentError(f"{path}: marker {v + 1}: phased BGEN data is not supported")
        if not 1 <= nbits <= 32:
            raise ArgumentError(f"{path}: marker {v + 1}: {nbits} bits per probability")
        nb = (2 * n * nbits + 7) // 8
        bits = np.unpackbits(np.frombuffer(blk, dtype=np.uint8, count=nb, offset=10 + n), bitorder="little")
        vals = bits[:2 * n * nbits].reshape(2 * n, nbits).astype(np.int64) @ (np.int64(1) << np.arange(nbits, dtype=np.int64))
        full = (1 << nbits) - 1
        k_aa, k_ab = vals[0::2], vals[1::2]
        k_bb = full - k_aa - k_ab
        miss = (ploidy & 0x80) != 0
        if (k_bb[~miss] < 0).any():
            raise ArgumentError(f"{path}: marker {v + 1}: probabilities sum above 1")
        cols.append((np.where(miss, -1, 2 * k_bb + k_ab), full))
        chrom.append(ch); pos.append(vpos); ids.append(rsid); ref.append(alleles[0]); alt.append(alleles[1])
    return cols, samples, chrom, pos, ids, ref, alt


class BgenIndex:
    """What the variant headers of a BGEN file hold (bgen_index): samples, chrom, pos, ids, ref, alt of the variants walked,
    `offsets` (int64) the file offset of each one's genotype block -- its 4-byte length field -- and the file's n (N),
    nvariants (M) and compression."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _NotStreamable(ArgumentError):
    """A BGEN or VCF file the streamed reader does not take: parse_genotypes reads it with read_bgen / read_vcf instead."""


def _bgen_walk(path, sample_path=None, stop=None):
    """The header walk of bgen_index over variants [0, stop) (all: None), skipping every genotype block by its stored length.
    Also returns (v, ArgumentError) of the first variant that is not biallelic, or None: read_bgen's refusal of it comes after
    the defects of the blocks before it.  A file too short for its headers raises _NotStreamable (read_bgen fails on it in
    a way of its own)."""
    try:
        with open(path, "rb") as f:
            b = _FileWindow(f)
            off, m, n, comp, samples = _bgen_head(b, path, sample_path)
            stop = m if stop is None else min(stop, m)
            chrom, pos, ids, ref, alt = [], [], [], [], []
            offsets = np.empty(stop, dtype=np.int64)
            bad = None
            p_ = off + 4
            for v in range(stop):
                rsid, ch, vpos, alleles, p_ = _bgen_variant(b, p_)
                if len(alleles) != 2 and bad is None:
                    bad = (v, ArgumentError(f"{path}: marker {v + 1} of BGEN is not biallelic!"))
                offsets[v] = p_
                p_ += 4 + _u("<I", b, p_)
                if p_ > len(b):
                    raise struct.error("genotype block past the end of the file")
                chrom.append(ch); pos.append(vpos); ids.append(rsid)
                ref.append(alleles[0] if alleles else ""); alt.append(alleles[1] if len(alleles) > 1 else "")
    except (struct.error, ValueError, IndexError, UnicodeDecodeError) as e:
        if isinstance(e, (ArgumentError, DimensionMismatch)):
            raise
        raise _NotStreamable(f"{path}: the BGEN headers cannot be walked ({e})") from None
    return BgenIndex(samples=samples, chrom=chrom, pos=pos, ids=ids, ref=ref, alt=alt, offsets=offsets, n=n, nvariants=m,
                     compression=comp), bad


def bgen_index(path, sample_path=None, variants=None):
    """Walk the headers of a BGEN v1.2 file without reading a genotype: sample ids by read_bgen's rules, per-variant chr, pos,
    rsid, ref, alt, and the file offset of each genotype block (a BgenIndex), of every variant or of the contiguous range
    `variants` of 0-based indices.  The header refusals are read_bgen's."""
    if variants is not None and (not isinstance(variants, range) or variants.step != 1):
        raise ArgumentError("variants must be a contiguous range of 0-based variant indices")
    idx, bad = _bgen_walk(path, sample_path, None if variants is None else variants.stop)
    if bad is not None:
        raise bad[1]
    if variants is not None:
        a, e = variants.start, min(variants.stop, idx.nvariants)
        for k in ("chrom", "pos", "ids", "ref", "alt", "offsets"):
            setattr(idx, k, getattr(idx, k)[a:e])
    return idx


_BGEN_REFUSED = {1: "corrupt genotype block", 2: "genotype block disagrees with the header", 3: "ploidy other than 2 is not supported",
                 4: "phased BGEN data is not supported", 6: "probabilities sum above 1"}
_BGEN_CANNOT = {10: "more than 16 bits per probability", 11: "the bits per probability change between markers",
                12: "16-bit probabilities on a grid finer than 1/32767", 13: "a genotype block read_bgen reads its own way"}


def _bgen_nbits(path, offset, n, comp):
    """The bit depth byte of the genotype block at `offset`."""
    with open(path, "rb") as f:
        f.seek(offset)
        blk = f.read(_u("<I", f.read(4), 0))
    if comp == 1:
        blk = zlib.decompress(blk[4:])
    return blk[9 + n]


def read_bgen_device(path, sample_path=None, variants=None, threads=None, device=0):
    """read_bgen's 7-tuple with a DosageMatrix in place of the columns, streamed from the file into the device: host threads
    read and inflate the genotype blocks, the GPU unpacks them (mih_dosage_create_bgen).  The matrix is the one
    DosageMatrix(*genotype_values(read_bgen(path)[0])) holds, bit for bit.  `variants`: a contiguous range of 0-based variant
    indices (a column shard), the metadata of those variants returned.  Refusals are read_bgen's ArgumentErrors; a file this
    path does not take (more than 16 bits per probability, bit depths that change, 16-bit fractional dosages) raises an
    ArgumentError too -- parse_genotypes reads such files with read_bgen."""
    import ctypes as C

    from .api import _check, lib
    path = str(path)
    if variants is not None and (not isinstance(variants, range) or variants.step != 1):
        raise ArgumentError("variants must be a contiguous range of 0-based variant indices")
    idx, bad = _bgen_walk(path, sample_path, None if variants is None else variants.stop)
    a, e = (0, idx.nvariants) if variants is None else (variants.start, variants.stop)
    if not 0 <= a <= e <= idx.nvariants:
        raise ArgumentError(f"variants {variants} out of range for {idx.nvariants} variants")
    if idx.nvariants == 0:
        raise _NotStreamable(f"{path} holds no variants")
    if a == e:
        raise ArgumentError(f"variants {variants} is empty")
    stream_to = e if bad is None else min(e, bad[0])
    if stream_to > a:
        offs = np.ascontiguousarray(idx.offsets[a:stream_to])
        h, den, bb, bw = C.c_void_p(None), C.c_int32(0), C.c_int64(-1), C.c_int32(0)
        rc = lib().mih_dosage_create_bgen(os.fsencode(path), idx.n, stream_to - a, offs.ctypes.data_as(C.c_void_p), idx.compression,
                                          int(threads or 0), device, C.byref(h), C.byref(den), C.byref(bb), C.byref(bw))
        if rc != 0 and bw.value:
            v, why = a + bb.value, bw.value
            if why in _BGEN_CANNOT:
                raise _NotStreamable(f"{path}: marker {v + 1}: {_BGEN_CANNOT[why]}: not streamed")
            if why == 5:
                raise ArgumentError(f"{path}: marker {v + 1}: {_bgen_nbits(path, int(idx.offsets[v]), idx.n, idx.compression)} bits per probability")
            raise ArgumentError(f"{path}: marker {v + 1}: {_BGEN_REFUSED[why]}")
        _check(rc)
    if bad is not None and bad[0] < e:
        if stream_to > a:
            lib().mih_mat_destroy(h)
        raise bad[1]
    x = DosageMatrix(None, den.value, device=device, _handle=h)
    return x, idx.samples, idx.chrom[a:e], idx.pos[a:e], idx.ids[a:e], idx.ref[a:e], idx.alt[a:e]


PANEL_BYTES = 1 << 30          # read_bgen_snp: u16 numerators held at a time


def read_bgen_snp(path, sample_path=None, variants=None, panel=None, threads=None, device=0, center=True, scale=True, impute=True,
                  dtype=np.float64, reserve=None):
    """read_bgen_device's 7-tuple with a SnpLinAlg first, for a file of hard calls (every probability 0 or 1): the headers are
    walked once, then panels of `panel` variants (default: about 1 GB of u16 numerators) are streamed into the device by
    read_bgen_device, packed into the 2-bit image (SnpBuilder.add) and dropped, so device memory peaks at the 2-bit image plus
    one panel.  The matrix is SnpLinAlg of the .bed encoding of the same genotypes, bit for bit.  A marker with a fractional
    dosage raises an ArgumentError naming it; the other refusals are read_bgen_device's."""
    path = str(path)
    if variants is not None and (not isinstance(variants, range) or variants.step != 1):
        raise ArgumentError("variants must be a contiguous range of 0-based variant indices")
    idx = bgen_index(path, sample_path, variants)
    a, e = (0, idx.nvariants) if variants is None else (variants.start, variants.stop)
    if not 0 <= a <= e <= idx.nvariants:
        raise ArgumentError(f"variants {variants} out of range for {idx.nvariants} variants")
    if idx.nvariants == 0:
        raise _NotStreamable(f"{path} holds no variants")
    if a == e:
        raise ArgumentError(f"variants {variants} is empty")
    step = int(panel) if panel else max(1, PANEL_BYTES // (2 * ((idx.n + 7) // 8 * 8)))
    if step < 1:
        raise ArgumentError("panel must be a positive number of variants")
    b = SnpBuilder(idx.n, e - a, center=center, scale=scale, impute=impute, dtype=dtype, device=device)
    try:
        for lo in range(a, e, step):
            hi = min(lo + step, e)
            part = read_bgen_device(path, sample_path, range(lo, hi), threads, device)[0]
            try:
                b.add(lo - a, part)
            except ArgumentError:
                raise ArgumentError(f"{path}: marker {a + b.bad_col + 1}: a dosage other than 0, 1 or 2: not a hard call") from None
            finally:
                del part
        x = b.finish(reserve)
    finally:
        b.close()
    return x, idx.samples, idx.chrom, idx.pos, idx.ids, idx.ref, idx.alt


# ---- VCF, streamed -----------------------------------------------------------------------------
def _vcf_text(fn, v):
    """The text a mih_vcf_header / mih_vcf_meta call holds, as bytes."""
    import ctypes as C
    need = C.c_int64(0)
    fn(v, None, 0, C.byref(need))
    buf = C.create_string_buffer(max(need.value, 1))
    fn(v, buf, need.value, C.byref(need))
    return buf.raw[:need.value]


def read_vcf_device(path, dosage=False, variants=None, threads=None, device=0, chunk_bytes=None):
    """read_vcf's 7-tuple with a DosageMatrix in place of the columns, streamed from the file into the device: plain text, gzip
    or BGZF (found from the bytes), host threads read and inflate, the GPU tokenises the sample fields (mih_vcf_open,
    mih_dosage_create_vcf).  The matrix is the one DosageMatrix(*genotype_values(read_vcf(path, dosage)[0])) holds, bit for
    bit.  `variants`: a contiguous range of 0-based record indices (a column shard) on its own reduced grid, the metadata of
    those records returned.  `chunk_bytes`: the text staged per transfer (default 8 MB; at least the longest line).  A file
    this path does not take -- anything but GT alleles 0 1 . and plain decimals of at most 4 places up to 2, ragged or
    multi-allelic records, '\r', header or container trouble, a path that is no readable regular file -- raises _NotStreamable, naming the 1-based record and the reason:
    parse_genotypes reads such a file with read_vcf, whose results and errors stay what they are."""
    return _read_vcf_streamed(path, dosage, variants, threads, device, chunk_bytes, None)


def read_vcf_snp(path, dosage=False, variants=None, threads=None, device=0, chunk_bytes=None, center=True, scale=True, impute=True,
                 dtype=np.float64, reserve=None):
    """read_vcf_device's 7-tuple with a SnpLinAlg first, for a file of hard calls: GT, or DS (dosage=True) where every value is
    0, 1 or 2.  The text is streamed as read_vcf_device streams it, but the tokeniser writes a small panel per chunk that is
    packed at once into the 2-bit image (mih_snp_create_vcf): device memory never holds n x p numerators.  The matrix is
    SnpLinAlg of the .bed encoding of read_vcf's genotypes (ALT counted as allele 2), bit for bit.  A DS record with another
    value raises an ArgumentError naming the 1-based record; every other refusal is read_vcf_device's _NotStreamable."""
    return _read_vcf_streamed(path, dosage, variants, threads, device, chunk_bytes,
                              (bool(center), bool(scale), bool(impute), _snp_dtype(dtype), reserve))


_VCF_NOT_HARD_CALL = 10


def _read_vcf_streamed(path, dosage, variants, threads, device, chunk_bytes, snp):
    """read_vcf_device (snp None) and read_vcf_snp (snp = center, scale, impute, dtype, reserve)."""
    import ctypes as C

    from .api import _check, lib
    path = str(path)
    if variants is not None and (not isinstance(variants, range) or variants.step != 1):
        raise ArgumentError("variants must be a contiguous range of 0-based record indices")
    L = lib()
    v, br, bw = C.c_void_p(None), C.c_int64(-1), C.c_int32(0)

    def cannot():                       # the library's own words: "path: record N: reason"
        buf = C.create_string_buffer(1024)
        L.mih_last_error(buf, 1024)
        return _NotStreamable(f"{buf.value.decode(errors='replace')}: not streamed")
    rc = L.mih_vcf_open(os.fsencode(path), int(threads or 0), int(chunk_bytes or 0), C.byref(v), C.byref(br), C.byref(bw))
    if rc != 0 and bw.value:
        raise cannot()
    _check(rc)
    try:
        n, m = C.c_int64(0), C.c_int64(0)
        _check(L.mih_vcf_info(v, C.byref(n), C.byref(m), None, None))
        a, e = (0, m.value) if variants is None else (variants.start, variants.stop)
        if not 0 <= a <= e <= m.value:
            raise ArgumentError(f"variants {variants} out of range for {m.value} records")
        if m.value == 0:
            raise _NotStreamable(f"{path} holds no variants")
        if a == e:
            raise ArgumentError(f"variants {variants} is empty")
        try:
            samples = _vcf_text(L.mih_vcf_header, v).decode("ascii").split("\t")[9:]
        except UnicodeDecodeError:
            raise _NotStreamable(f"{path}: record 1: sample ids that are not ASCII: not streamed") from None
        h, den = C.c_void_p(None), C.c_int32(0)
        if snp is None:
            rc = L.mih_dosage_create_vcf(v, 1 if dosage else 0, a, e - a, int(threads or 0), device, C.byref(h), C.byref(den),
                                         C.byref(br), C.byref(bw))
        else:
            center, scale, impute, dtype, reserve = snp
            rc = L.mih_snp_create_vcf(v, 1 if dosage else 0, a, e - a, int(threads or 0), int(center), int(scale), int(impute),
                                      32 if dtype is np.float32 else 64, device, C.byref(h), C.byref(br), C.byref(bw))
        if rc != 0 and bw.value == _VCF_NOT_HARD_CALL:
            buf = C.create_string_buffer(1024)
            L.mih_last_error(buf, 1024)
            raise ArgumentError(buf.value.decode(errors="replace"))
        if rc != 0 and bw.value:
            raise cannot()
        _check(rc)
        if snp is None:
            x = DosageMatrix(None, den.value, device=device, _handle=h)
        else:
            x = SnpLinAlg(None, center=center, scale=scale, impute=impute, device=device, _handle=h, dtype=dtype)
            x._reserve(reserve)
        rows = [ln.split("\t") for ln in _vcf_text(L.mih_vcf_meta, v).decode("ascii").split("\n")[:-1]]
    finally:
        L.mih_vcf_close(v)
    chrom, pos, ids, ref, alt = ([r[k] for r in rows] for k in range(5))
    return x, samples, chrom, [int(q) for q in pos], ids, ref, alt


# ---- parse_genotypes ---------------------------------------------------------------------------
def parse_genotypes(tgtfile, dosage=False, device=0, two_bit=False):
    """parse_genotypes(tgtfile, dosage) -- wrapper.jl:451-485: (X, sample_ids, chr, pos, snpid, ref, alt).  VCF (`.vcf`,
    `.vcf.gz`; GT allele counts, or DS with dosage=True) and BGEN (`.bgen`) give a DosageMatrix (or, on a grid finer than
    1/32767, a DenseMatrix of the standardized values); a binary PLINK trio (the path without .bed/.bim/.fam) gives
    SnpLinAlg(center=true, scale=true, impute=true).  Either way X is the standardized matrix the reference fits.
    two_bit=True: a VCF or BGEN file of hard calls gives that SnpLinAlg too (read_vcf_snp, read_bgen_snp) -- the same standardized
    matrix at an eighth of the memory, on the 2-bit kernels; a file that is not all hard calls, or one the streamed readers do
    not take, is an ArgumentError in the reader's words (never a silent DosageMatrix)."""
    tgt = str(tgtfile)
    if two_bit and tgt.endswith((".vcf", ".vcf.gz")):
        return read_vcf_snp(tgt, dosage, device=device)
    if two_bit and tgt.endswith(".bgen"):
        return read_bgen_snp(tgt, device=device)
    if tgt.endswith((".vcf", ".vcf.gz")):
        try:
            return read_vcf_device(tgt, dosage, device=device)
        except _NotStreamable:          # read_vcf's own path: whatever is outside the streamed grammar, and its errors
            cols, samples, chrom, pos, ids, ref, alt = read_vcf(tgt, dosage)
    elif tgt.endswith(".bgen"):
        try:
            return read_bgen_device(tgt, device=device)
        except _NotStreamable:          # read_bgen's own path: > 16 bits, mixed depths, 16-bit fractional dosages, its errors
            cols, samples, chrom, pos, ids, ref, alt = read_bgen(tgt)
    elif all(os.path.isfile(tgt + e) for e in (".bed", ".bim", ".fam")):
        if dosage:
            raise ArgumentError("PLINK files detected but dosage = true!")
        n = _count_lines(tgt + ".fam")
        with open(tgt + ".fam") as f:
            samples = [ln.split()[1] for ln in f if ln.strip()]
        chrom, pos, ids, a1, a2 = _read_bim(tgt)
        x = SnpLinAlg(tgt + ".bed", n, center=True, scale=True, impute=True, device=device)
        return x, samples, chrom, [int(q) for q in pos], ids, a1, a2
    else:
        raise ArgumentError("Unrecognized target file format: target file can only be VCF files (ends in .vcf or .vcf.gz), "
                            "BGEN (ends in .bgen) or PLINK (do not include.bim/bed/fam) and all trio must exist in 1 directory)")
    if not cols:
        raise ArgumentError(f"{tgt} holds no variants")
    num, val = genotype_values(cols)
    x = DenseMatrix(val, device=device) if num is None else DosageMatrix(num, val, device=device)
    return x, samples, chrom, pos, ids, ref, alt
