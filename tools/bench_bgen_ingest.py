"""BGEN -> device dosage matrix: the streamed reader (genotypes.read_bgen_device) against inflating alone, and against the host
reader it replaces.  One JSON line per bit depth (8 and 16):

  * n x p (default 500 000 x 4 000), seeded imputation-like genotypes, zlib (tests/bgen_files.py: write_imputed): the streamed
    ingest's wall time (median of 3) with the variants/s, decompressed GB/s and u16 GB/s landed in HBM it makes; the peak RSS
    growth of the child process over the process with the runtime up; and an inflate-only time -- the same number of threads
    inflating the same blocks in runs of the same size, no GPU work -- with the ratio stream / inflate;
  * n x p_small (default 500 000 x 200), where the host reader still copes: parse_genotypes through read_bgen (the old path) and
    through the streamed reader, on the same file.

    python tools/bench_bgen_ingest.py [--n 500000] [--p 4000] [--p-small 200] [--threads 8] [--dir /tmp/bgen_bench]
    python tools/bench_bgen_ingest.py --stream-only FILE      # one streamed ingest (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kb(key):
    return int([ln for ln in open("/proc/self/status") if ln.startswith(key + ":")][0].split()[1])


def inflate_only(path, idx, threads, run_bytes=8 << 20):
    """the streamed reader's host work without the GPU: runs of consecutive blocks of ~run_bytes inflated, pread per run"""
    n = idx.n
    first = None
    with open(path, "rb") as f:
        f.seek(int(idx.offsets[0]))
        clen = int.from_bytes(f.read(4), "little")
        first = int.from_bytes(f.read(4), "little") if idx.compression == 1 else clen
    per_run = max(1, run_bytes // max(first, 1))
    offs = list(idx.offsets)
    fd = os.open(path, os.O_RDONLY)

    def run(c0):
        c1 = min(c0 + per_run, len(offs))
        last = int(offs[c1 - 1])
        end = last + 4 + int.from_bytes(os.pread(fd, 4, last), "little")
        raw = os.pread(fd, end - int(offs[c0]), int(offs[c0]))
        got = 0
        for c in range(c0, c1):
            o = int(offs[c]) - int(offs[c0])
            cl = int.from_bytes(raw[o:o + 4], "little")
            dlen = int.from_bytes(raw[o + 4:o + 8], "little")
            got += len(zlib.decompress(raw[o + 8:o + 4 + cl], bufsize=dlen))      # one output buffer of the stored size, as the library
        return got

    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        total = sum(ex.map(run, range(0, len(offs), per_run)))
    dt = time.perf_counter() - t
    os.close(fd)
    assert total >= len(offs) * (10 + n)
    return dt, total


def child(path, threads, reps):
    import numpy as np

    import mendeliht_amd as m
    from mendeliht_amd import genotypes as G
    m.DosageMatrix(np.zeros((64, 2), np.uint16), 1).export()          # the runtime is up
    rss0 = kb("VmRSS")
    idx = G.bgen_index(path)
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        x = G.read_bgen_device(path, threads=threads)[0]
        walls.append(time.perf_counter() - t)
        den, n, p, ld = x.denom, x.n, x.p, (x.n + 7) // 8 * 8
        del x
    grow = (kb("VmHWM") - rss0) / 1024
    inf = [inflate_only(path, idx, threads) for _ in range(reps)]
    dt_inf, dec_bytes = statistics.median(d for d, _ in inf), inf[0][1]
    w = statistics.median(walls)
    return dict(n=n, p=p, denom=den, threads=threads, stream_s=round(w, 3), stream_s_all=[round(v, 3) for v in walls],
                variants_per_s=round(p / w, 1), decompressed_GB_s=round(dec_bytes / w / 1e9, 3),
                u16_landed_GB_s=round(2 * ld * p / w / 1e9, 3), peak_rss_growth_MB=round(grow, 1),
                inflate_only_s=round(dt_inf, 3), stream_over_inflate=round(w / dt_inf, 3), file_MB=os.path.getsize(path) >> 20)


def small(path):
    import mendeliht_amd as m
    from mendeliht_amd import genotypes as G
    m.DosageMatrix.synthetic(64, 2)
    t = time.perf_counter()
    cols, *meta = G.read_bgen(path)
    num, den = G.genotype_values(cols)
    x_old = m.DosageMatrix(num, den)
    old = time.perf_counter() - t
    del cols, num
    t = time.perf_counter()
    x_new = m.parse_genotypes(path)[0]
    new = time.perf_counter() - t
    import numpy as np
    assert x_new.denom == x_old.denom and np.array_equal(x_new.export(0, 3), x_old.export(0, 3))
    return dict(old_s=round(old, 3), new_s=round(new, 3), old_over_new=round(old / new, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=4_000)
    ap.add_argument("--p-small", type=int, default=200)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depths", default="8,16")
    ap.add_argument("--dir", default="/tmp/bgen_bench")
    ap.add_argument("--child", nargs=2, metavar=("FILE", "MODE"))
    ap.add_argument("--stream-only", metavar="FILE")
    a = ap.parse_args()
    if a.stream_only:
        from mendeliht_amd import genotypes as G
        t = time.perf_counter()
        x = G.read_bgen_device(a.stream_only, threads=a.threads)[0]
        print(json.dumps(dict(stream_s=round(time.perf_counter() - t, 3), p=x.p, denom=x.denom)))
        return
    if a.child:
        out = child(a.child[0], a.threads, a.reps) if a.child[1] == "stream" else small(a.child[0])
        print(json.dumps(out))
        return
    from bgen_files import write_imputed
    os.makedirs(a.dir, exist_ok=True)
    for B in (int(b) for b in a.depths.split(",")):
        res = dict(bits=B, compression="zlib")
        for tag, p, mode in (("large", a.p, "stream"), ("small", a.p_small, "small")):
            path = os.path.join(a.dir, f"imputed_{B}bit_{a.n}x{p}.bgen")
            if not os.path.exists(path):
                t = time.perf_counter()
                write_imputed(path + ".part", a.n, p, B, seed=B, threads=16)
                os.replace(path + ".part", path)
                res[f"{tag}_write_s"] = round(time.perf_counter() - t, 1)
            r = subprocess.run([sys.executable, __file__, "--child", path, mode, "--threads", str(a.threads), "--reps", str(a.reps)],
                               capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(r.stdout + r.stderr)
            res[tag] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
