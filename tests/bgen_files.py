"""BGEN v1.2 writers for the streamed-reader tests and tools/bench_bgen_ingest.py: any bit depth 1..32, compression none or zlib,
with or without a sample block, and per-block control of every field read_bgen checks (for the refusal cases)."""
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def pack_probs(kaa, kab, nbits):
    """The probability section of a layout-2 block: (k_AA, k_AB) of every sample, nbits each, LSB first."""
    if nbits == 8:
        return np.stack([kaa, kab], axis=1).astype(np.uint8).tobytes()
    if nbits == 16:
        return np.stack([kaa, kab], axis=1).astype("<u2").tobytes()
    vals = np.stack([kaa, kab], axis=1).reshape(-1).astype(np.uint64)
    bits = ((vals[:, None] >> np.arange(nbits, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little").tobytes()


def genotype_block(kaa, kab, miss, nbits, ploidy=None, phased=0, n_field=None, k_field=2, pminmax=(2, 2)):
    """The (inflated) genotype block of one variant; `ploidy`: the samples' ploidy bytes before the missing bit (default 2)."""
    n = kaa.size
    pl = (np.full(n, 2, np.uint8) if ploidy is None else np.asarray(ploidy, np.uint8)) | np.where(miss, 0x80, 0).astype(np.uint8)
    kaa, kab = np.where(miss, 0, kaa), np.where(miss, 0, kab)
    return (struct.pack("<IHBB", n if n_field is None else n_field, k_field, *pminmax) + pl.tobytes() + bytes([phased, nbits]) +
            pack_probs(kaa, kab, nbits))


def variant_record(j, block, comp, nalleles=2, level=6):
    """Variant j's identifying data (v{j+1}, rs{j+1}, chromosome 1 + j // 100, position 10 j + 1, alleles A, C) and its stored
    genotype block."""
    def s16(x):
        return struct.pack("<H", len(x)) + x.encode()
    v = s16(f"v{j + 1}") + s16(f"rs{j + 1}") + s16(str(1 + j // 100)) + struct.pack("<IH", 10 * j + 1, nalleles)
    v += b"".join(struct.pack("<I", 1) + a.encode() for a in "ACGT"[:nalleles])
    if comp == 1:
        z = zlib.compress(block, level)
        return v + struct.pack("<II", len(z) + 4, len(block)) + z
    return v + struct.pack("<I", len(block)) + block


def header(n, p, comp, samples=True, layout=2):
    ids = [f"s{i + 1}".encode() for i in range(n)]
    sblock = struct.pack("<II", 8 + sum(2 + len(s) for s in ids), n) + b"".join(struct.pack("<H", len(s)) + s for s in ids) if samples else b""
    flags = comp | (layout << 2) | ((1 << 31) if samples else 0)
    head = struct.pack("<III", 20, p, n) + b"bgen" + struct.pack("<I", flags)
    return struct.pack("<I", len(head) + len(sblock)) + head + sblock


def write_blocks(path, n, blocks, comp=1, samples=True, nalleles=None, level=6):
    """A BGEN file of the given inflated genotype blocks; nalleles: {variant: allele count} where it is not 2."""
    nalleles = nalleles or {}
    with open(path, "wb") as f:
        f.write(header(n, len(blocks), comp, samples))
        for j, blk in enumerate(blocks):
            f.write(variant_record(j, blk, comp, nalleles.get(j, 2), level))


def write_probs(path, kaa, kab, miss, nbits, comp=1, samples=True, sample_file=False):
    """n x p stored probabilities (k_AA, k_AB) / (2^nbits - 1); sample_file: also a .sample file beside it (ids t1..tN)."""
    n, p = kaa.shape
    write_blocks(path, n, [genotype_block(kaa[:, j], kab[:, j], miss[:, j], nbits) for j in range(p)], comp, samples)
    if sample_file:
        with open(str(path)[:-5] + ".sample", "w") as f:
            f.write("ID_1 ID_2 missing\n0 0 0\n" + "".join(f"t{i + 1} t{i + 1} 0\n" for i in range(n)))


def imputed_column(n, nbits, seed, j, hard=0.9, missing=0.01):
    """One variant of imputation-like data: genotypes Binomial(2, maf), maf ~ U(0.01, 0.5); a fraction `hard` of the samples
    are hard calls, the others put 1 - eps (eps ~ U(0, 0.2)) on their genotype and eps on a neighbour (at 16 bits rounded to
    multiples of 3 / 65535, so that the file streams)."""
    rng = np.random.default_rng([seed, j])
    full = (1 << nbits) - 1
    g = rng.binomial(2, rng.uniform(0.01, 0.5), n)
    prob = np.zeros((n, 3))
    prob[np.arange(n), g] = 1.0
    soft = rng.random(n) >= hard
    eps = rng.uniform(0.0, 0.2, n) * soft
    nb = np.where(g == 0, 1, np.where(g == 2, 1, np.where(rng.random(n) < 0.5, 0, 2)))
    prob[np.arange(n), g] -= eps
    prob[np.arange(n), nb] += eps
    step = 3 if nbits == 16 else 1          # 16 bits: probabilities on the grid 3 / 65535 (fractional 16-bit data is read_bgen's)
    kaa = np.rint(prob[:, 0] * full / step).astype(np.int64) * step
    kab = np.minimum(np.rint(prob[:, 1] * full / step).astype(np.int64) * step, full - kaa)
    return kaa, kab, rng.random(n) < missing


def write_imputed(path, n, p, nbits, seed=1, comp=1, threads=16, level=6, hard=0.9):
    """A seeded n x p BGEN of imputation-like genotypes (imputed_column), the blocks built and compressed by a thread pool."""
    def rec(j):
        kaa, kab, miss = imputed_column(n, nbits, seed, j, hard)
        return variant_record(j, genotype_block(kaa, kab, miss, nbits), comp, 2, level)
    with open(path, "wb") as f, ThreadPoolExecutor(threads) as ex:
        f.write(header(n, p, comp, samples=False))
        for j0 in range(0, p, 4 * threads):
            for r in ex.map(rec, range(j0, min(p, j0 + 4 * threads))):
                f.write(r)
