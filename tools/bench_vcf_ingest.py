"""VCF -> device dosage matrix: the streamed reader (genotypes.read_vcf_device) against inflating alone, and against the host
reader it replaces.  One JSON line per file: GT and 3-decimal DS, each as BGZF and as a single-stream gzip file.

  * n x p (default 500 000 x 1 000), seeded: GT hard calls with 1 % missing; DS imputation-like, 90 % of the entries on a hard
    call, the rest anywhere on the grid 1/1000, 1 % missing.  The streamed ingest's wall time (median of 3) with the records/s
    and text GB/s it makes; the peak RSS growth of the child over the process with the runtime up; "inflate only": the same
    number of threads inflating the same bytes as often as the reader does (twice: its scan and its ingest), no GPU work and no
    look at the text -- and beside it ONE inflate of the file, so that the second pass is visible;
  * n_small x p_small (default 20 000 x 200), where the host reader still copes: parse_genotypes through read_vcf (the old path)
    and through the streamed reader, on the same BGZF file.

    python tools/bench_vcf_ingest.py [--n 500000] [--p 1000] [--threads 8] [--dir /tmp/vcf_bench]
    python tools/bench_vcf_ingest.py --stream-only FILE [--dosage]    # one streamed ingest (for rocprofv3 --kernel-trace --stats)

--two-bit: the streamed ingest is genotypes.read_vcf_snp (hard calls packed into the 2-bit SnpLinAlg) instead of read_vcf_device;
the large files' lines then also carry the device memory the finished matrix holds and the most that was in use while it was
being built (hipMemGetInfo, sampled every 10 ms by a thread), against n x p u16.  With --stream-only --pack N P it times
DosageMatrix.to_snp() of the seeded synthetic N x P matrix over the denominator 1 (hard calls) instead (the pack kernel alone, for rocprofv3).
"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK = 65280                                            # inflated bytes per BGZF block (htslib's)
SLAB = 8                                                 # records generated and compressed per task


def kb(key):
    return int([ln for ln in open("/proc/self/status") if ln.startswith(key + ":")][0].split()[1])


# ---- seeded files ------------------------------------------------------------------------------
DS_TABLE = np.frombuffer(b"".join(f"{v / 1000:.3f}\t".encode() for v in range(2001)) + b".\t\0\0\0\0", dtype=np.uint8).reshape(2002, 6)


def slab_text(dosage, n, j0, j1, seed):
    """records [j0, j1) as text"""
    rng = np.random.default_rng([seed, j0])
    out = []
    for j in range(j0, j1):
        maf = rng.uniform(0.01, 0.5)
        g = rng.binomial(2, maf, n)
        if dosage:
            v = g * 1000
            soft = rng.random(n) < 0.1
            v = np.where(soft, np.clip(v + rng.integers(-400, 401, n), 0, 2000), v)
            v = np.where(rng.random(n) < 0.01, 2001, v)
            flat = DS_TABLE[v].reshape(-1)                          # 6 bytes per entry, the missing one padded with zeros
            body = flat[flat != 0].tobytes()
        else:
            table = np.frombuffer(b"0/0\t0/1\t1/1\t./.\t", dtype="S4")
            body = table[np.where(rng.random(n) < 0.01, 3, g)].tobytes()
        out.append(f"1\t{j + 1}\trs{j + 1}\tA\tG\t.\tPASS\t.\t{'DS' if dosage else 'GT'}\t".encode() + body[:-1] + b"\n")
    return b"".join(out)


def bgzf_member(chunk):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(chunk) + c.flush()
    return (struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(body) + 25) + body
            + struct.pack("<II", zlib.crc32(chunk), len(chunk)))


def write_pair(base, dosage, n, p, seed, threads=16):
    """the same text as BGZF (base + '.bgzf.vcf.gz') and as ONE gzip member (base + '.gz1.vcf.gz': raw deflate segments compressed
    in parallel and joined by sync flushes, as pigz does); returns the text's length"""
    head = ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"s{i}" for i in range(n)) + "\n").encode()

    def task(j0):
        text = (head if j0 == 0 else b"") + slab_text(dosage, n, j0, min(j0 + SLAB, p), seed)
        blocks = b"".join(bgzf_member(text[o:o + BLOCK]) for o in range(0, len(text), BLOCK))
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        seg = c.compress(text) + (c.flush(zlib.Z_FINISH) if j0 + SLAB >= p else c.flush(zlib.Z_FULL_FLUSH))
        return blocks, seg, zlib.crc32(text), len(text), text
    total, crc = 0, 0
    with open(base + ".bgzf.vcf.gz.part", "wb") as fb, open(base + ".gz1.vcf.gz.part", "wb") as fg, ThreadPoolExecutor(threads) as ex:
        fg.write(struct.pack("<BBBBIBB", 0x1f, 0x8b, 8, 0, 0, 0, 0xff))
        starts = list(range(0, p, SLAB))
        for w0 in range(0, len(starts), 2 * threads):            # a window of tasks at a time: bounded memory
            for blocks, seg, _, ln, text in ex.map(task, starts[w0:w0 + 2 * threads]):
                fb.write(blocks)
                fg.write(seg)
                crc = zlib.crc32(text, crc)
                total += ln
        fb.write(bgzf_member(b""))
        fg.write(struct.pack("<II", crc, total & 0xFFFFFFFF))
    os.replace(base + ".bgzf.vcf.gz.part", base + ".bgzf.vcf.gz")
    os.replace(base + ".gz1.vcf.gz.part", base + ".gz1.vcf.gz")
    return total


# ---- inflating alone ---------------------------------------------------------------------------
def inflate_only(path, threads, reps):
    """the library's own workers reading and inflating every chunk of the file, no device and no look at the text
    (mih_vcf_inflate), timed `reps` times once and `reps` times twice in a row; and pass 1 alone (mih_vcf_open).
    (open_s, once_s, twice_s, inflated bytes), medians"""
    import ctypes as C

    import mendeliht_amd as m
    L = m.lib()
    opens, once, twice = [], [], []
    total = C.c_int64(0)

    def one(v):
        t = time.perf_counter()
        assert L.mih_vcf_inflate(v, threads, C.byref(total)) == 0
        return time.perf_counter() - t
    for _ in range(reps):
        v, br, bw = C.c_void_p(None), C.c_int64(-1), C.c_int32(0)
        t = time.perf_counter()
        assert L.mih_vcf_open(os.fsencode(path), threads, 0, C.byref(v), C.byref(br), C.byref(bw)) == 0
        opens.append(time.perf_counter() - t)
        once.append(one(v))
        twice.append(one(v) + one(v))
        L.mih_vcf_close(v)
    return statistics.median(opens), statistics.median(once), statistics.median(twice), total.value


class FreeMemory:
    """free device memory as the HIP runtime of this process reports it; watch(): the least seen until stop()"""

    def __init__(self):
        import ctypes as C
        path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]
        self.hip, self.C = C.CDLL(path), C
        self.low, self.on = None, False

    def now(self):
        f, t = self.C.c_size_t(0), self.C.c_size_t(0)
        assert self.hip.hipMemGetInfo(self.C.byref(f), self.C.byref(t)) == 0
        return f.value

    def watch(self):
        import threading
        self.low, self.on = self.now(), True

        def loop():
            while self.on:
                self.low = min(self.low, self.now())
                time.sleep(0.01)
        self.thread = threading.Thread(target=loop)
        self.thread.start()

    def stop(self):
        self.on = False
        self.thread.join()
        return self.low


def child(path, dosage, threads, reps, two_bit=False):
    import mendeliht_amd as m
    from mendeliht_amd import genotypes as G
    m.DosageMatrix(np.zeros((64, 2), np.uint16), 1).export()          # the runtime is up
    rss0 = kb("VmRSS")
    walls, mem = [], {}
    for _ in range(reps):
        if two_bit:
            free = FreeMemory()
            before = free.now()
            free.watch()
        t = time.perf_counter()
        x = (G.read_vcf_snp if two_bit else G.read_vcf_device)(path, dosage, threads=threads)[0]
        walls.append(time.perf_counter() - t)
        den, n, p = getattr(x, "denom", 1), x.n, x.p
        if two_bit:
            low = free.stop()
            mem = dict(two_bit=True, device_MB_held=round((before - free.now()) / 2 ** 20, 1), device_MB_peak=round((before - low) / 2 ** 20, 1),
                       u16_MB=round(2 * n * p / 2 ** 20, 1))
        del x
    grow = (kb("VmHWM") - rss0) / 1024
    open_s, one, two, text = inflate_only(path, threads, reps)
    w = statistics.median(walls)
    return dict(n=n, p=p, denom=den, threads=threads, stream_s=round(w, 3), stream_s_all=[round(v, 3) for v in walls],
                records_per_s=round(p / w, 1), text_GB_s=round(text / w / 1e9, 3), text_MB=text >> 20, file_MB=os.path.getsize(path) >> 20,
                peak_rss_growth_MB=round(grow, 1), scan_s=round(open_s, 3), inflate_once_s=round(one, 3), inflate_only_s=round(two, 3),
                stream_over_inflate=round(w / two, 3), **mem)


def small(path, dosage):
    import mendeliht_amd as m
    from mendeliht_amd import genotypes as G
    m.DosageMatrix.synthetic(64, 2)
    t = time.perf_counter()
    cols = G.read_vcf(path, dosage)[0]
    num, den = G.genotype_values(cols)
    x_old = m.DosageMatrix(num, den)
    old = time.perf_counter() - t
    del cols, num
    t = time.perf_counter()
    x_new = m.parse_genotypes(path, dosage)[0]
    new = time.perf_counter() - t
    assert x_new.denom == x_old.denom and np.array_equal(x_new.export(0, 3), x_old.export(0, 3))
    return dict(old_s=round(old, 3), new_s=round(new, 3), old_over_new=round(old / new, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=1_000)
    ap.add_argument("--n-small", type=int, default=20_000)
    ap.add_argument("--p-small", type=int, default=200)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fields", default="GT,DS")
    ap.add_argument("--dir", default="/tmp/vcf_bench")
    ap.add_argument("--child", nargs=2, metavar=("FILE", "MODE"))
    ap.add_argument("--stream-only", metavar="FILE")
    ap.add_argument("--dosage", action="store_true")
    ap.add_argument("--two-bit", action="store_true")
    ap.add_argument("--pack", nargs=2, type=int, metavar=("N", "P"))
    a = ap.parse_args()
    if a.pack:
        import mendeliht_amd as m
        n, p = a.pack
        d = m.DosageMatrix.synthetic(n, p, seed=5, denom=1, missing_rate=0.01)      # over the denominator 1 the generator emits hard calls
        walls = []
        for _ in range(a.reps):
            t = time.perf_counter()
            y = d.to_snp(reserve=False)
            walls.append(time.perf_counter() - t)
            if len(walls) < a.reps:
                del y
        bits = np.unpackbits(y.export_bed()[:3], axis=1, bitorder="little").reshape(3, -1, 2)[:, :n]
        same = np.array_equal(np.array([0, 0xFFFF, 1, 2], dtype=np.uint16)[bits[:, :, 0] + 2 * bits[:, :, 1]].T, d.export(0, 3))
        print(json.dumps(dict(n=n, p=p, to_snp_s=[round(v, 4) for v in walls], equals_source=bool(same))))
        return
    if a.stream_only:
        from mendeliht_amd import genotypes as G
        t = time.perf_counter()
        x = (G.read_vcf_snp if a.two_bit else G.read_vcf_device)(a.stream_only, a.dosage, threads=a.threads)[0]
        print(json.dumps(dict(stream_s=round(time.perf_counter() - t, 3), p=x.p, denom=getattr(x, "denom", 1), two_bit=a.two_bit)))
        return
    if a.child:
        out = child(a.child[0], a.dosage, a.threads, a.reps, a.two_bit) if a.child[1] == "stream" else small(a.child[0], a.dosage)
        print(json.dumps(out))
        return
    os.makedirs(a.dir, exist_ok=True)
    for field in a.fields.split(","):
        dosage = field == "DS"
        jobs = []
        for tag, n, p in (("large", a.n, a.p), ("small", a.n_small, a.p_small)):
            base = os.path.join(a.dir, f"{field}_{n}x{p}")
            if not os.path.exists(base + ".gz1.vcf.gz"):
                t = time.perf_counter()
                write_pair(base, dosage, n, p, seed=7 + dosage)
                print(json.dumps(dict(field=field, wrote=base, write_s=round(time.perf_counter() - t, 1))), flush=True)
            jobs += [(tag, kind, base + f".{kind}.vcf.gz") for kind in (("bgzf", "gz1") if tag == "large" else ("bgzf",))]
        for tag, kind, path in jobs:
            cmd = [sys.executable, __file__, "--child", path, "stream" if tag == "large" else "small", "--threads", str(a.threads),
                   "--reps", str(a.reps)] + (["--dosage"] if dosage else []) + (["--two-bit"] if a.two_bit and tag == "large" else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(r.stdout + r.stderr)
            print(json.dumps(dict(field=field, container=kind, size=tag, **json.loads(r.stdout.strip().splitlines()[-1]))), flush=True)


if __name__ == "__main__":
    main()
