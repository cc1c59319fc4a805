"""VCF streamed into the device dosage matrix (genotypes.read_vcf_device, mih_vcf_open / mih_dosage_create_vcf): the matrix is
the one the host reader builds, bit for bit, in every container, at every chunk cut and row count; record ranges and regrids;
parse_genotypes, iht and cross_validate routed through it; the files it does not take go to read_vcf unchanged; bounded host
memory."""
import json
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import FIX, GOLD, ROOT
from test_genotype_readers_cpu import bed_codes
from vcf_files import DS_TOKENS, GT_TOKENS, bgzf_bytes, gzip_bytes, random_tokens, vcf_text, write

import mendeliht_amd as M
from mendeliht_amd import genotypes as G
from mendeliht_amd.api import ArgumentError

pytestmark = pytest.mark.gpu


def old_matrix(path, dosage=False):
    num, den = G.genotype_values(G.read_vcf(path, dosage)[0])
    return M.DosageMatrix(num, den)


def assert_same(x, y):
    assert isinstance(x, M.DosageMatrix) and x.denom == y.denom and (x.n, x.p) == (y.n, y.p)
    assert np.array_equal(x.export(), y.export())
    for a, b in zip(x.mu_sigma(), y.mu_sigma()):
        assert np.array_equal(a, b)


def streamed(path, dosage=False, meta=None, **kw):
    got = G.read_vcf_device(path, dosage, **kw)
    want = meta if meta is not None else G.read_vcf(path, dosage)[1:]
    assert list(got[1:]) == list(want) and all(isinstance(q, int) for q in got[3])
    return got[0]


def test_golden_excerpt(mih):
    path = os.path.join(GOLD, "normal_head.vcf.gz")
    x = streamed(path)
    assert x.denom == 1
    assert_same(x, old_matrix(path))


ROWS = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


@pytest.mark.parametrize("dosage", [False, True])
def test_row_counts(mih, tmp_path, dosage):
    """rows around the 8-row pad, the 64-lane wave, the 256-thread workgroup and the 4 KB segment (1024 GT tokens), 5 records:
    every token form, 5 % missing, one all-missing and one all-zero record"""
    rng = np.random.default_rng(int(dosage))
    for n in ROWS:
        toks = random_tokens(rng, n, 5, DS_TOKENS if dosage else GT_TOKENS)
        toks[1] = ["." if dosage else "./."] * n
        toks[3] = [("0", "0.0", ".000")[i % 3] if dosage else ("0/0", "0|0", "0")[i % 3] for i in range(n)]
        path = write(tmp_path / f"r{n}.vcf", vcf_text(toks, "DS" if dosage else "GT", last_newline=n % 2 == 0))
        x = streamed(path, dosage)
        assert_same(x, old_matrix(path, dosage))
        assert dosage or x.denom == 1


@pytest.fixture(scope="module")
def twelve(tmp_path_factory):
    """12 records with lines of about 1.3 KB, as GT and as DS of mixed widths, and what the host reader makes of them"""
    d = tmp_path_factory.mktemp("cuts")
    rng = np.random.default_rng(3)
    out = {}
    for dosage, pool, n in ((False, GT_TOKENS, 400), (True, DS_TOKENS, 340)):
        data = vcf_text(random_tokens(rng, n, 12, pool), "DS" if dosage else "GT", comment_after=7)
        path = write(d / f"t{int(dosage)}.vcf", data)
        assert 1200 < max(len(ln) for ln in data.split(b"\n") if not ln.startswith(b"#")) < 1500
        out[dosage] = (data, path, old_matrix(path, dosage), G.read_vcf(path, dosage)[1:])
    return d, out


@pytest.mark.parametrize("dosage", [False, True])
def test_chunk_cuts_everywhere(mih, twelve, dosage):
    """chunk_bytes in every multiple of 64 from 256 to 4096: chunks shorter than a line (one record each), cuts behind every
    record count"""
    data, path, want, meta = twelve[1][dosage]
    for chunk in range(256, 4097, 64):
        assert_same(streamed(path, dosage, meta, chunk_bytes=chunk), want)


@pytest.mark.parametrize("dosage", [False, True])
def test_chunk_cuts_in_every_container(mih, twelve, dosage):
    d, out = twelve
    data, _, want, meta = out[dosage]
    files = [write(d / f"c{int(dosage)}.vcf", data), write(d / f"c{int(dosage)}_1.vcf.gz", gzip_bytes(data)),
             write(d / f"c{int(dosage)}_4.vcf.gz", gzip_bytes(data, 4))]
    for block in (37, 4096, 65280):
        files.append(write(d / f"c{int(dosage)}_b{block}.vcf.gz", bgzf_bytes(data, block, eof=block != 4096)))
    for path in files:
        for threads in (1, 8):
            assert_same(streamed(path, dosage, meta, chunk_bytes=1024, threads=threads), want)
        assert_same(streamed(path, dosage, meta), want)          # and the default: the whole file one chunk


def long_field(rng, keys, gt, ds, cut):
    """a sample field under FORMAT `keys`, padded to 40-80 bytes by PL where there is one; cut: subfields kept"""
    val = dict(GT=gt, DS=ds, AD=f"{rng.integers(0, 40)},{rng.integers(0, 40)}", DP=str(rng.integers(1, 99)), GQ="99",
               PL=",".join(str(rng.integers(100, 3000)) for _ in range(rng.integers(7, 12))))
    return ":".join([val[k] for k in keys][:cut])


def test_long_sample_fields_and_changing_formats(mih, tmp_path):
    rng = np.random.default_rng(5)
    n, p = 300, 9
    formats = ["GT:AD:DP:GQ:PL:DS", "GT:DS", "DS:GT", "GT"]
    for name, fmts in (("both", [formats[j % 3] for j in range(p)]), ("gtonly", [formats[(j + 1) % 4] for j in range(p)])):
        toks = []
        for j in range(p):
            keys = fmts[j].split(":")
            row = []
            for i in range(n):
                cut = rng.integers(1, len(keys) + 1) if rng.random() < 0.15 else len(keys)     # fields cut short, before k too
                row.append(long_field(rng, keys, GT_TOKENS[rng.integers(0, 10)], DS_TOKENS[rng.integers(0, 8)], cut))
            toks.append(row)
        data = vcf_text(toks, fmts)
        if name == "both":
            full = [len(f) for f in toks[0] if f.count(":") == 5]
            assert 40 <= min(full) and max(full) <= 80
        path = write(tmp_path / f"{name}.vcf", data)
        for dosage in ((False, True) if name == "both" else (False,)):
            want = old_matrix(path, dosage)
            assert_same(streamed(path, dosage), want)
            assert_same(streamed(path, dosage, chunk_bytes=4096, threads=3), want)
            assert (want.export() == 0xFFFF).mean() > 0.05
    # a GT:DS field that holds only 0/0 is missing under DS
    path = write(tmp_path / "short.vcf", vcf_text([["0/0", "0/1:1.5", "1/1:", "0/0:."]], "GT:DS"))
    x = streamed(path, True)
    assert x.export()[:, 0].tolist() == [0xFFFF, 3, 0xFFFF, 0xFFFF] and x.denom == 2


def test_grid_reductions(mih, tmp_path):
    rng = np.random.default_rng(7)
    pools = {1: ["0", "1", "2", "1.0", "2.000", "."], 2: ["0", "0.5", ".5", "1.50", "2"], 4: ["0.25", "1.75", "1", "0.5"],
             20: ["0.05", "1.95", "0.5", "2", "0.10"], 1000: ["0.001", "1.999", "0.5"], 10000: ["0.0001", "0.5", "1.0000"]}
    for want, pool in pools.items():
        toks = random_tokens(rng, 90, 6, np.array(pool), missing=0.1)
        toks[0][:len(pool)] = pool                               # every token of the pool occurs
        path = write(tmp_path / f"g{want}.vcf", vcf_text(toks, "DS"))
        x = streamed(path, True)
        assert x.denom == want, (want, x.denom)
        assert_same(x, old_matrix(path, True))
    # the gcd across chunks: 11 records of hard calls, the only 0.0001 in the last one, every record its own chunk
    toks = random_tokens(rng, 50, 12, np.array(["0", "1", "2", "1.0"]))
    toks[11][37] = "0.0001"
    path = write(tmp_path / "last.vcf", vcf_text(toks, "DS"))
    for kw in (dict(chunk_bytes=256), dict(chunk_bytes=256, threads=1), {}):
        x = streamed(path, True, **kw)
        assert x.denom == 10000
        assert_same(x, old_matrix(path, True))
    assert streamed(write(tmp_path / "miss.vcf", vcf_text([["."] * 9] * 3, "DS")), True).denom == 1


def test_variant_ranges_regrid_to_the_whole(mih, tmp_path):
    rng = np.random.default_rng(11)
    toks = (random_tokens(rng, 70, 4, np.array(["0", "1", "2"])) + random_tokens(rng, 70, 4, np.array(["0.5", "1", "1.5"]))
            + random_tokens(rng, 70, 4, np.array(["0.05", "1.95", "0.5"])))
    data = vcf_text(toks, "DS")
    meta = G.read_vcf(write(tmp_path / "r.vcf", data), True)[1:]
    for path in (str(tmp_path / "r.vcf"), write(tmp_path / "r.vcf.gz", gzip_bytes(data, 2)), write(tmp_path / "rb.vcf.gz", bgzf_bytes(data, 200))):
        whole = streamed(path, True, meta, chunk_bytes=512)
        assert whole.denom == 20
        mu, s = whole.mu_sigma()
        parts = []
        for (a, b), own in (((0, 4), 1), ((4, 8), 2), ((8, 12), 20)):
            got = G.read_vcf_device(path, True, variants=range(a, b), chunk_bytes=512)
            assert got[1] == meta[0] and [list(m) for m in got[2:]] == [list(m[a:b]) for m in meta[1:]]
            assert got[0].denom == own and got[0].p == b - a
            parts.append((a, b, got[0]))
        lcm = math.lcm(*(x.denom for _, _, x in parts))
        assert lcm == whole.denom
        for a, b, x in parts:
            x.regrid(lcm)
            assert np.array_equal(x.export(), whole.export(a, b - a))
            assert np.array_equal(x.mu_sigma()[0], mu[a:b]) and np.array_equal(x.mu_sigma()[1], s[a:b])
        x = G.read_vcf_device(path, True, variants=range(3, 10))[0]       # a range across the three grids, cut inside chunks
        assert x.denom == 20 and np.array_equal(x.export(), whole.export(3, 7))
    for bad in (range(0, 0), range(5, 5), range(0, 8, 2), range(5, 99), range(12, 13), [0, 1]):
        with pytest.raises(ArgumentError) as e:
            G.read_vcf_device(path, True, variants=bad)
        assert not isinstance(e.value, G._NotStreamable)


def outcome(fn):
    """what fn returns and the warnings it raises, or the exception's type and text"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            got = fn()
        except Exception as e:                                    # noqa: BLE001  (whatever the reader raises is the outcome)
            return type(e), str(e), [str(x.message) for x in w]
    return None, got, [str(x.message) for x in w]


def test_hand_over(mih, tmp_path):
    """one file per reason: read_vcf_device names the record, parse_genotypes gives what the host reader gives"""
    rng = np.random.default_rng(13)

    def text(fmt, pool, bad=None, **kw):
        toks = random_tokens(rng, 4, 6, np.array(pool), missing=0.1)
        if bad is not None:
            toks[3][1] = bad                                     # record 4, sample 2
        return vcf_text(toks, fmt, **kw)
    ds, gt = ["0", "0.5", "1.25", "2"], ["0/0", "0/1", "1|1", "./."]
    cases = [(f"ds{i}", text("DS", ds, tok), True, 4) for i, tok in
             enumerate(["0.03125", "1e-1", "+1", "1/2", " 1", "2.5", "-0.5", "1_0", "nan", "1.2.3", "0.5 ", "0" * 33])]
    cases += [(f"gt{i}", text("GT", gt, tok), False, 4) for i, tok in enumerate(["1/1/1", "0/2", "0/", "01", "0 1", "1/1\r"])]
    cases.append(("crlf", text("GT", gt).replace(b"\n", b"\r\n"), False, 1))
    lines = text("GT", gt).split(b"\n")
    ragged = list(lines)
    ragged[2 + 4] = ragged[2 + 4].rsplit(b"\t", 1)[0]            # record 5 one sample short
    cases.append(("ragged", b"\n".join(ragged), False, 5))
    longer = list(lines)
    longer[2 + 1] += b"\t0/0"                                    # record 2 one sample too many
    cases.append(("longer", b"\n".join(longer), False, 2))
    cases.append(("empty", b"\n".join(lines[:4] + [b""] + lines[4:]), False, 3))       # an empty line is record 3
    cases.append(("alt", text("GT", gt).replace(b"rs3\tA\tG", b"rs3\tA\tG,T"), False, 3))
    cases.append(("nokey", text("GT", gt), True, 1))
    cases.append(("mixedkey", vcf_text(random_tokens(rng, 4, 3, np.array(["0/1:0.5"])), ["GT:DS", "GT", "GT:DS"]), True, 2))
    cases.append(("twice", b"\n".join(lines[:4] + [lines[1]] + lines[4:]), False, 3))     # a second #CHROM line behind two records
    cases.append(("pos", text("GT", gt).replace(b"\t31\trs4", b"\t+31\trs4"), False, 4))
    for name, data, dosage, record in cases:
        for path in (write(tmp_path / f"{name}.vcf", data), write(tmp_path / f"{name}.vcf.gz", bgzf_bytes(data, 97))):
            with pytest.raises(G._NotStreamable, match=f"record {record}: ") as e:
                G.read_vcf_device(path, dosage)
            assert path in str(e.value)

            def old():
                cols, *meta = G.read_vcf(path, dosage)
                num, val = G.genotype_values(cols)
                return [M.DosageMatrix(num, val)] + meta
            want, got = outcome(old), outcome(lambda: list(mih.parse_genotypes(path, dosage)))
            assert got[0] == want[0] and got[2] == want[2], (name, got, want)
            if want[0] is None:
                assert got[1][1:] == want[1][1:], name
                assert_same(got[1][0], want[1][0])
            else:
                assert got[1] == want[1], (name, got, want)
    # the container is taken from the bytes, the host reader opens by name: a mismatch is handed over (and fails there)
    good = text("GT", gt)
    for path in (write(tmp_path / "plain.vcf.gz", good), write(tmp_path / "zipped.vcf", gzip_bytes(good))):
        with pytest.raises(G._NotStreamable, match="record 1: "):
            G.read_vcf_device(path)
        want, got = outcome(lambda: G.read_vcf(path)), outcome(lambda: mih.parse_genotypes(path))
        assert want[0] is not None and got[:2] == want[:2]


def test_hand_over_of_what_is_no_readable_file(mih, tmp_path):
    """a missing path, a directory, a named pipe and a ## line that is not ASCII: the host reader's outcome, whatever it is"""
    import threading
    rng = np.random.default_rng(19)
    good = vcf_text(random_tokens(rng, 4, 6, GT_TOKENS[:6]))
    os.mkdir(tmp_path / "dir.vcf")
    fifo = str(tmp_path / "pipe.vcf")
    os.mkfifo(fifo)
    latin = write(tmp_path / "latin.vcf", good.replace(b"##fileformat", b"##caf\xe9\n##fileformat"))
    utf8 = write(tmp_path / "utf8.vcf", good.replace(b"##fileformat", "##café\n##fileformat".encode()))

    def fed(fn):
        """fn with one writer at the pipe's other end, for the one reader that opens it"""
        def feed():
            with open(fifo, "wb") as f:
                f.write(good)
        t = threading.Thread(target=feed, daemon=True)
        t.start()
        got = outcome(fn)
        t.join(10)
        assert not t.is_alive()
        return got
    for path, piped in ((str(tmp_path / "typo.vcf"), False), (str(tmp_path / "typo.vcf.gz"), False), (str(tmp_path / "dir.vcf"), False),
                        (fifo, True), (latin, False), (utf8, False)):
        with pytest.raises(G._NotStreamable, match="record 1: ") as e:      # opens nothing that is no regular file
            G.read_vcf_device(path)
        assert path in str(e.value)

        def old():
            cols, *meta = G.read_vcf(path)
            num, val = G.genotype_values(cols)
            return [M.DosageMatrix(num, val)] + meta
        run = fed if piped else outcome
        want, got = run(old), run(lambda: list(mih.parse_genotypes(path)))
        assert got[0] == want[0] and got[2] == want[2], (path, got, want)
        if want[0] is None:
            assert got[1][1:] == want[1][1:]
            assert_same(got[1][0], want[1][0])
        else:
            assert got[1] == want[1], (path, got, want)
    assert fed(lambda: len(G.read_vcf(fifo)[0]))[:2] == (None, 6)          # the pipe is a working input, as it was


def test_a_record_longer_than_256_segments(mih, tmp_path):
    """k_vcf_parse sums the tab counts of the record's segments before its own, 256 at a stride: sample text beyond 1 MB (here
    20 000 fields of 60 bytes and more) takes the second stride"""
    rng = np.random.default_rng(23)
    n = 20_000
    toks = [[f"{GT_TOKENS[g]}:12,3:15:99:{pl}:{DS_TOKENS[d]}" for g, d, pl in
             zip(rng.integers(0, 10, n), rng.integers(0, 8, n), np.array(["1234,5678,910," * 3 + "0", "250,1000,2000,3000,400,50000,60000,7,8"])[rng.integers(0, 2, n)])]
            for _ in range(2)]
    data = vcf_text(toks, "GT:AD:DP:GQ:PL:DS")
    assert min(len(ln) for ln in data.split(b"\n")[2:4]) > 257 * 4096
    path = write(tmp_path / "long.vcf", data)
    for dosage in (True, False):
        want = old_matrix(path, dosage)
        assert_same(streamed(path, dosage), want)
        assert_same(streamed(path, dosage, chunk_bytes=4096, threads=2), want)


@pytest.fixture(scope="module")
def pheno_vcf(tmp_path_factory):
    """data/normal's first 300 variants as a BGZF VCF (GT), and its phenotypes"""
    d = tmp_path_factory.mktemp("route")
    codes = bed_codes(os.path.join(FIX, "normal.bed"), 1000)[:, :300]
    toks = np.array(["./.", "0/0", "0|1", "1/1"])[codes + 1].T
    write(d / "g.vcf.gz", bgzf_bytes(vcf_text([list(r) for r in toks]), 65280))
    np.savetxt(d / "phenotypes.txt", np.loadtxt(os.path.join(FIX, "normal_y_fam6.txt")))
    return d


def test_routing(mih, pheno_vcf, monkeypatch):
    d = pheno_vcf
    path = str(d / "g.vcf.gz")
    old_x = old_matrix(path)
    kw = dict(phenotypes=str(d / "phenotypes.txt"), summaryfile=str(d / "s.txt"), betafile=str(d / "b.txt"))

    def not_streamed(*a, **k):
        raise G._NotStreamable("the old reader")
    with monkeypatch.context() as mp:                       # the fit on the old reader's DosageMatrix
        mp.setattr(G, "read_vcf_device", not_streamed)
        old = mih.iht(path, 9, mih.Normal, **kw)

    def no(*a, **k):
        raise AssertionError("read_vcf called for a streamable file")
    monkeypatch.setattr(G, "read_vcf", no)
    x = mih.parse_genotypes(path)[0]
    assert x.denom == 1
    assert_same(x, old_x)
    new = mih.iht(path, 9, mih.Normal, **kw)
    assert new.iter == old.iter and np.array_equal(new.beta, old.beta) and new.logl == old.logl and new.σg == old.σg
    assert np.count_nonzero(new.beta) > 0 and np.array_equal(np.asarray(new.c), np.asarray(old.c))
    mse = mih.cross_validate(path, mih.Normal, path=range(8, 11), q=3, phenotypes=str(d / "phenotypes.txt"),
                             cv_summaryfile=str(d / "cv.txt"), folds=mih.hash_folds(1000, 3), verbose=False)
    assert len(mse) == 3 and np.all(np.isfinite(mse))


def test_bounded_host_memory(mih, tmp_path):
    """100 000 x 2 000 GT as plain text (800 MB): the reader holds its staging, not the text and not an int64 matrix"""
    n, p, distinct = 100_000, 2_000, 16
    rng = np.random.default_rng(9)
    tok = np.frombuffer(b"./.\t0/0\t0/1\t1/1\t", dtype=np.uint8).reshape(4, 4)
    codes = rng.integers(-1, 3, (distinct, n))
    bodies = []
    for g in codes:
        b = tok[g + 1].reshape(-1).copy()
        b[-1] = ord("\n")
        bodies.append(b.tobytes())
    path = str(tmp_path / "m.vcf")
    with open(path, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t")
        f.write(b"\t".join(b"s%d" % i for i in range(n)) + b"\n")
        for j in range(p):
            f.write(f"1\t{j + 1}\trs{j + 1}\tA\tG\t.\tPASS\t.\tGT\t".encode())
            f.write(bodies[j % distinct])
    assert os.path.getsize(path) > 800_000_000
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
got = G.read_vcf_device({path!r})
x = got[0]
grow = (kb('VmHWM') - rss0) / 1024
print(json.dumps(dict(grow_mb=grow, n=x.n, p=x.p, denom=x.denom, samples=len(got[1]), last_id=got[4][-1],
                      sums=[int(x.export(j, 1).astype(np.int64).sum()) for j in (0, 7, {p - 1})])))
""")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert (got["n"], got["p"], got["denom"], got["samples"], got["last_id"]) == (n, p, 1, n, f"rs{p}")
    assert got["sums"] == [int(np.where(codes[j % distinct] < 0, 0xFFFF, codes[j % distinct]).sum()) for j in (0, 7, p - 1)]
    assert got["grow_mb"] <= 768, got
