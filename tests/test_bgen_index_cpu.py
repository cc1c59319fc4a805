"""The BGEN header walk of the streamed reader (genotypes.bgen_index; no GPU): the same samples and metadata as read_bgen, an
offset on every genotype block's length field, variant ranges, and read_bgen's refusals of the headers."""
import os
import struct
import zlib

import numpy as np
import pytest

from bgen_files import genotype_block, write_blocks, write_probs
from conftest import GOLD

from mendeliht_amd import genotypes as G
from mendeliht_amd.api import ArgumentError


def seeded(path, n, p, nbits, comp, samples=True, sample_file=False, seed=0):
    rng = np.random.default_rng([seed, nbits, comp, n])
    full = (1 << nbits) - 1
    kaa = rng.integers(0, full + 1, (n, p))
    kab = (rng.random((n, p)) * (full - kaa + 1)).astype(np.int64)
    miss = rng.random((n, p)) < 0.1
    write_probs(path, kaa, kab, miss, nbits, comp=comp, samples=samples, sample_file=sample_file)


def check_offsets(path, idx, nbits=None):
    """every offset is a genotype block's length field: the block it frames inflates to N, K = 2 and the depth written"""
    raw = open(path, "rb").read()
    for v, o in enumerate(idx.offsets):
        clen = struct.unpack_from("<I", raw, o)[0]
        blk = raw[o + 4:o + 4 + clen]
        if idx.compression == 1:
            blk = zlib.decompress(blk[4:])
        assert struct.unpack_from("<IH", blk, 0) == (idx.n, 2), v
        if nbits is not None:
            assert blk[9 + idx.n] == nbits
        nxt = idx.offsets[v + 1] if v + 1 < len(idx.offsets) else len(raw)
        assert o + 4 + clen <= nxt


def same_as_read_bgen(path, idx, sample_path=None):
    _, samples, chrom, pos, ids, ref, alt = G.read_bgen(path, sample_path)
    assert idx.samples == samples
    assert (idx.chrom, idx.pos, idx.ids, idx.ref, idx.alt) == (chrom, pos, ids, ref, alt)
    assert len(idx.offsets) == idx.nvariants == len(chrom)


def test_golden_excerpt():
    path, sp = os.path.join(GOLD, "normal_head.bgen"), os.path.join(GOLD, "normal.sample")
    idx = G.bgen_index(path, sp)
    same_as_read_bgen(path, idx, sp)
    assert idx.n == 1000 and idx.nvariants == 200 and idx.compression == 1
    check_offsets(path, idx, nbits=16)


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("nbits", range(1, 17))
def test_seeded_files(tmp_path, nbits, comp):
    for k, (samples, sample_file) in enumerate(((True, False), (False, False), (False, True), (True, True))):
        path = str(tmp_path / f"f{k}.bgen")
        seeded(path, 13 + k, 7, nbits, comp, samples, sample_file)
        idx = G.bgen_index(path)
        same_as_read_bgen(path, idx)
        check_offsets(path, idx, nbits)
        want = [f"t{i + 1}" for i in range(13 + k)] if sample_file else ([f"s{i + 1}" for i in range(13 + k)] if samples else
                                                                           [str(i + 1) for i in range(13 + k)])
        assert idx.samples == want
        if sample_file:
            os.remove(path[:-5] + ".sample")


def test_variant_ranges(tmp_path):
    path = str(tmp_path / "r.bgen")
    seeded(path, 9, 40, 8, 1)
    whole = G.bgen_index(path)
    for a, b in ((0, 40), (0, 1), (13, 27), (39, 40), (5, 5)):
        idx = G.bgen_index(path, variants=range(a, b))
        assert idx.ids == whole.ids[a:b] and idx.pos == whole.pos[a:b] and idx.chrom == whole.chrom[a:b]
        assert idx.ref == whole.ref[a:b] and idx.alt == whole.alt[a:b]
        assert np.array_equal(idx.offsets, whole.offsets[a:b])
        assert idx.samples == whole.samples and idx.nvariants == 40
    with pytest.raises(ArgumentError):
        G.bgen_index(path, variants=range(0, 10, 2))


def test_header_refusals_are_read_bgens(tmp_path):
    n = 4
    blk = genotype_block(np.full(n, 255), np.zeros(n, np.int64), np.zeros(n, bool), 8)
    cases = {}
    for name, layout, comp in (("zstd", 2, 2), ("layout 1", 1, 1)):
        path = str(tmp_path / f"{name}.bgen")
        write_blocks(path, n, [blk] * 3, comp=comp if comp < 2 else 1)
        raw = bytearray(open(path, "rb").read())
        struct.pack_into("<I", raw, 4 + 20 - 4, comp | (layout << 2) | (1 << 31))
        open(path, "wb").write(bytes(raw))
        cases[name] = path
    path = str(tmp_path / "tri.bgen")
    write_blocks(path, n, [blk] * 5, nalleles={3: 3})
    cases["not biallelic"] = path
    for what, path in cases.items():
        with pytest.raises(ArgumentError) as old:
            G.read_bgen(path)
        with pytest.raises(ArgumentError) as new:
            G.bgen_index(path)
        assert str(new.value) == str(old.value) and what.split()[-1] in str(old.value)
    assert "marker 4 of BGEN is not biallelic" in str(new.value)
