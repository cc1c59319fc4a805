"""VCF files for the tests: text written from explicit token arrays, and the containers the streamed reader takes -- gzip, gzip of
several members, BGZF with a chosen block size, with or without its empty EOF block."""
import gzip
import struct
import zlib

import numpy as np

HEAD9 = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def vcf_text(tokens, fmt="GT", comments=("##fileformat=VCFv4.2",), samples=None, alt="G", last_newline=True, comment_after=None):
    """The text of a VCF whose record j holds the sample fields tokens[j] (a list of n strings) under FORMAT fmt (one string, or
    one per record).  comment_after: a ## line is put behind that many records."""
    n = len(tokens[0])
    samples = samples or [f"s{i + 1}" for i in range(n)]
    lines = list(comments) + [HEAD9 + "\t" + "\t".join(samples)]
    for j, row in enumerate(tokens):
        if comment_after is not None and j == comment_after:
            lines.append("##a comment in the middle of the records")
        f = fmt if isinstance(fmt, str) else fmt[j]
        lines.append(f"{1 + j // 100}\t{10 * j + 1}\trs{j + 1}\tA\t{alt}\t.\tPASS\t.\t{f}\t" + "\t".join(row))
    return ("\n".join(lines) + ("\n" if last_newline else "")).encode()


GT_TOKENS = np.array(["0/0", "0/1", "1/1", "./.", "0|1", "1|0", "1", "0", ".", "./1", ""])
DS_TOKENS = np.array(["0", "2", ".5", "1.", "0.25", "1.250", "0.0375", "."])


def random_tokens(rng, n, p, pool, missing=0.05, miss="."):
    """p records of n tokens drawn from pool, a share `missing` of them replaced by `miss`"""
    t = pool[rng.integers(0, len(pool), (p, n))]
    t = np.where(rng.random((p, n)) < missing, miss, t)
    return [list(r) for r in t]


def gzip_bytes(data, members=1):
    """data as a gzip file of `members` members (cut at arbitrary places)"""
    cuts = [len(data) * i // members for i in range(members + 1)]
    return b"".join(gzip.compress(data[a:b], 6) for a, b in zip(cuts, cuts[1:]))


def bgzf_bytes(data, block=65280, eof=True):
    """data as BGZF: gzip members of at most `block` inflated bytes with the BC extra field; eof: the empty last block"""
    def member(chunk):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        head = struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(body) + 25)
        return head + body + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    out = [member(data[o:o + block]) for o in range(0, len(data), block)]
    if eof:
        out.append(member(b""))
    return b"".join(out)


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def containers(tmp, name, data, block=4096):
    """the same text in every container the streamed reader takes: [(tag, path)]"""
    return [("text", write(tmp / f"{name}.vcf", data)),
            ("gzip", write(tmp / f"{name}_gz.vcf.gz", gzip_bytes(data))),
            ("gzip3", write(tmp / f"{name}_gz3.vcf.gz", gzip_bytes(data, 3))),
            ("bgzf", write(tmp / f"{name}_bgzf.vcf.gz", bgzf_bytes(data, block))),
            ("bgzf_noeof", write(tmp / f"{name}_bgzf0.vcf.gz", bgzf_bytes(data, block, eof=False)))]
