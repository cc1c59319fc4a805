"""Pass 1 of the streamed VCF reader (mih_vcf_open / mih_vcf_info / mih_vcf_header: host only, no GPU): the container found from
the bytes, n, the record count, the sample ids and the longest line as read_vcf sees them, at every position of a line end
relative to a BGZF block end; the files it refuses, with nothing left open."""
import ctypes as C
import os

import numpy as np
import pytest

from vcf_files import HEAD9, bgzf_bytes, containers, gzip_bytes, random_tokens, vcf_text, write, GT_TOKENS

import mendeliht_amd as M
from mendeliht_amd import genotypes as G


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return M.lib()


def scan(L, path, chunk_bytes=0, threads=0):
    """(rc, bad_record, bad_what) of a refused file, else dict(n, records, container, longest, samples)"""
    v, br, bw = C.c_void_p(None), C.c_int64(-1), C.c_int32(0)
    rc = L.mih_vcf_open(os.fsencode(str(path)), threads, chunk_bytes, C.byref(v), C.byref(br), C.byref(bw))
    if rc != 0:
        assert not v.value
        return rc, br.value, bw.value
    try:
        n, m, kind, longest, need = C.c_int64(0), C.c_int64(0), C.c_int32(-1), C.c_int64(0), C.c_int64(0)
        assert L.mih_vcf_info(v, C.byref(n), C.byref(m), C.byref(kind), C.byref(longest)) == 0
        assert L.mih_vcf_header(v, None, 0, C.byref(need)) == 0
        buf = C.create_string_buffer(need.value)
        assert L.mih_vcf_header(v, buf, need.value, C.byref(need)) == 0
        return dict(n=n.value, records=m.value, container=kind.value, longest=longest.value,
                    samples=buf.raw[:need.value].decode().split("\t")[9:])
    finally:
        assert L.mih_vcf_close(v) == 0


def open_fds():
    return len(os.listdir("/proc/self/fd"))


def test_version_is_0_7(L):
    major, minor = C.c_int(-1), C.c_int(-1)
    assert L.mih_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) == (0, 7)


def test_every_container_gives_read_vcfs_counts(L, tmp_path):
    rng = np.random.default_rng(1)
    data = vcf_text(random_tokens(rng, 13, 9, GT_TOKENS[:6]), samples=[f"id_{i}" for i in range(13)], comment_after=4)
    longest = max(len(ln) for ln in data.split(b"\n"))
    kinds = dict(text=0, gzip=1, gzip3=1, bgzf=2, bgzf_noeof=2)
    for tag, path in containers(tmp_path, "small", data, block=300):
        cols, samples = G.read_vcf(path)[:2]
        got = scan(L, path)
        assert got == dict(n=13, records=len(cols), container=kinds[tag], longest=longest, samples=samples), (tag, got)
    assert scan(L, os.path.join(os.path.dirname(__file__), "golden", "normal_head.vcf.gz"))["records"] == 200


def test_inflate_only_reads_every_byte(L, tmp_path):
    """mih_vcf_inflate, the host half of the ingest that the benchmark times: every chunk of every container, whole text"""
    data = vcf_text(random_tokens(np.random.default_rng(4), 50, 40, GT_TOKENS[:6]))
    for tag, path in containers(tmp_path, "inf", data, block=777):
        for chunk, threads in ((0, 0), (300, 3), (300, 1)):
            v, br, bw, total = C.c_void_p(None), C.c_int64(-1), C.c_int32(0), C.c_int64(0)
            assert L.mih_vcf_open(os.fsencode(path), threads, chunk, C.byref(v), C.byref(br), C.byref(bw)) == 0
            assert L.mih_vcf_inflate(v, threads, C.byref(total)) == 0 and total.value == len(data), (tag, chunk)
            assert L.mih_vcf_inflate(v, threads, C.byref(total)) == 0 and total.value == len(data)       # and again, from the start
            assert L.mih_vcf_close(v) == 0


@pytest.mark.parametrize("last_newline", [True, False])
def test_line_ends_at_every_place_of_a_block(L, tmp_path, last_newline):
    """40-byte record lines, BGZF blocks of 1 .. 64 and 4096 bytes: blocks without a newline, a newline as a block's last byte,
    a ## line that starts a block, a ## line among the records, a last line without its newline"""
    def record(j):                                               # 39 bytes and the newline
        rest = f"\tA\tG\t.\tPASS\t.\tGT\t0/1"
        return f"1\t{j + 1}\t".encode() + b"r" * (39 - len(rest) - len(f"1\t{j + 1}\t")) + rest.encode()
    lines = [b"##" + b"x" * 37, b"##" + b"y" * 37, (HEAD9 + "\ts1").encode()] + [record(j) for j in range(7)]
    lines.insert(6, b"##" + b"z" * 37)
    assert all(len(ln) == 39 for ln in lines if not ln.startswith(b"#CHROM"))
    data = b"\n".join(lines) + (b"\n" if last_newline else b"")
    want = dict(n=1, records=7, container=2, longest=max(len(ln) for ln in lines), samples=["s1"])
    starts = np.cumsum([0] + [len(ln) + 1 for ln in lines])[:-1]
    seen = set()
    for block in list(range(1, 65)) + [4096]:
        for eof in (True, False):
            path = write(tmp_path / f"b{block}_{int(eof)}.vcf.gz", bgzf_bytes(data, block, eof))
            assert scan(L, path, threads=2 if block % 2 else 1) == want, (block, eof)
        if block == 64:
            assert len(G.read_vcf(path)[0]) == 7                 # the writer's output is what the host reader reads, too
        ends = starts[1:] - 1                                    # the newline bytes
        seen |= {"nl last in block"} if np.any((ends + 1) % block == 0) else set()
        seen |= {"## starts a block"} if any(s % block == 0 for s, ln in zip(starts, lines) if ln.startswith(b"##")) else set()
        seen |= {"block without nl"} if block < 40 else set()
    assert seen == {"nl last in block", "## starts a block", "block without nl"}


def test_longest_line_straddling_three_blocks(L, tmp_path):
    toks = [["0/0"] * 4, ["0/1"] * 4, ["1|1:" + "7" * 150] + ["0/0"] * 3, ["./."] * 4]
    data = vcf_text(toks)
    lines = data.split(b"\n")
    k = int(np.argmax([len(ln) for ln in lines]))
    start = sum(len(ln) + 1 for ln in lines[:k])
    block = 100
    assert (start + len(lines[k])) // block - start // block >= 2          # its bytes lie in three blocks or more
    path = write(tmp_path / "long.vcf.gz", bgzf_bytes(data, block))
    assert scan(L, path)["longest"] == len(lines[k]) and scan(L, path)["records"] == 4
    assert scan(L, path, chunk_bytes=64)["longest"] == len(lines[k])


def test_refusals_leave_nothing_open(L, tmp_path):
    data = vcf_text([["0/1", "1/1"], ["0/0", "./."]])
    body = b"\n".join(ln for ln in data.split(b"\n") if not ln.startswith(b"#CHROM"))
    big = vcf_text(random_tokens(np.random.default_rng(2), 2, 400, GT_TOKENS[:6]))
    gz = gzip_bytes(big)
    cases = {
        "nohead.vcf": (body, 0, 7),                              # no #CHROM line: the first record meets none
        "nohead_gz.vcf.gz": (gzip_bytes(body), 0, 7),
        "nohead_bgzf.vcf.gz": (bgzf_bytes(body, 50), 0, 7),
        "onlycomments.vcf": (b"##a\n##b\n", 0, 7),
        "cut.vcf.gz": (gz[:len(gz) // 2], None, 8),              # a truncated gzip member
        "cut_bgzf.vcf.gz": (bgzf_bytes(big, 500)[:-40], None, 8),
        "plain.vcf.gz": (data, 0, 8),                            # plain text under a .gz name
        "zipped.vcf": (gzip_bytes(data), 0, 8),                  # gzip under a .vcf name
        "twice.vcf": (data + data.split(b"\n")[1] + b"\n", 2, 7),   # a second #CHROM line, behind two records
        "latin.vcf": (data.replace(b"##fileformat", b"##caf\xe9\n##fileformat"), 0, 7),   # a ## line the host reader may not decode
    }
    before = open_fds()
    os.mkdir(tmp_path / "dir.vcf")
    os.mkfifo(tmp_path / "pipe.vcf")                             # never opened: an open would wait for a writer
    for name in ("missing.vcf", "missing.vcf.gz", "dir.vcf", "pipe.vcf"):
        got = scan(L, tmp_path / name)
        assert isinstance(got, tuple) and got[0] != 0 and got[1:] == (0, 9), (name, got)
    for name, (raw, record, what) in cases.items():
        got = scan(L, write(tmp_path / name, raw))
        assert isinstance(got, tuple) and got[0] != 0 and got[2] == what, (name, got)
        if record is not None:
            assert got[1] == record, (name, got)
    assert open_fds() == before
    ok = scan(L, write(tmp_path / "fine.vcf", data))
    assert ok["records"] == 2 and open_fds() == before
