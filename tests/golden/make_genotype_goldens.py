"""Cut tests/golden/normal_head.vcf.gz, normal_head.bgen and normal.sample from MendelIHT.jl's example data (data/normal.*):
the first 200 variants of the VCF and of the BGEN, the whole .sample file.  The BGEN header keeps everything but M (patched
to 200); the sample block and the 200 variant blocks are copied byte for byte.

    python tests/golden/make_genotype_goldens.py MENDELIHT_DATA_DIR
"""
import gzip
import os
import shutil
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KEEP = 200


def cut_vcf(src, dst):
    out, kept = [], 0
    with gzip.open(src, "rt") as f:
        for line in f:
            if not line.startswith("#"):
                if kept == KEEP:
                    break
                kept += 1
            out.append(line)
    with gzip.GzipFile(dst, "wb", mtime=0) as g:          # mtime 0: the same bytes on every run
        g.write("".join(out).encode())


def cut_bgen(src, dst):
    b = open(src, "rb").read()
    off, lh = struct.unpack_from("<II", b, 0)
    flags = struct.unpack_from("<I", b, 4 + lh - 4)[0]
    assert (flags >> 2) & 15 == 2, "layout 2 only"
    pos = off + 4
    for _ in range(KEEP):                                  # skip variant identifying data + genotype block
        for _s in range(3):
            pos += 2 + struct.unpack_from("<H", b, pos)[0]
        pos += 4
        k = struct.unpack_from("<H", b, pos)[0]; pos += 2
        for _a in range(k):
            pos += 4 + struct.unpack_from("<I", b, pos)[0]
        pos += 4 + struct.unpack_from("<I", b, pos)[0]
    head = bytearray(b[:off + 4])
    struct.pack_into("<I", head, 8, KEEP)                 # M
    with open(dst, "wb") as f:
        f.write(bytes(head) + b[off + 4:pos])


if __name__ == "__main__":
    data = sys.argv[1]
    cut_vcf(os.path.join(data, "normal.vcf.gz"), os.path.join(HERE, "normal_head.vcf.gz"))
    cut_bgen(os.path.join(data, "normal.bgen"), os.path.join(HERE, "normal_head.bgen"))
    shutil.copyfile(os.path.join(data, "normal.sample"), os.path.join(HERE, "normal.sample"))
