"""Quality control and sample selection on the device (csrc/qc.hip): SnpLinAlg.counts with a row mask, filter with the defaults
and subset dropping a random 5 % of the rows and 10 % of the columns, each the median of 3, on a synthetic matrix with 1 %
missing genotypes -- with the algorithmic bytes (source tiles read, result tiles written, missing lists read and written) and
the GB/s they give beside the 8 TB/s HBM peak.

    python tools/bench_qc.py                      # 500 000 x 200 000 (25 GB)
    python tools/bench_qc.py --floor              # 100 000 x 20 000: subset against the host route, which must be >= 10x slower

The host route is what a caller had before: export_bed() -> numpy -> SnpLinAlg(bed, n')."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mendeliht_amd as m  # noqa: E402

HBM_PEAK = 8.0e12


def median_of(fn, reps=3):
    out, times = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def tile_bytes(n, p):
    return ((p + 31) // 32) * ((n + 127) // 128) * 1024


def host_route(x, rows, cols):
    """export_bed() -> unpack, select, repack with numpy (column blocks of 1024) -> SnpLinAlg."""
    bed = x.export_bed()
    n_out = rows.size
    out = np.zeros((cols.size, (n_out + 3) // 4), dtype=np.uint8)
    for c0 in range(0, cols.size, 1024):
        blk = bed[cols[c0:c0 + 1024]]
        two = np.empty((blk.shape[0], blk.shape[1] * 4), dtype=np.uint8)
        for s in range(4):
            two[:, s::4] = (blk >> (2 * s)) & 3
        sel = np.zeros((blk.shape[0], out.shape[1] * 4), dtype=np.uint8)
        sel[:, :n_out] = two[:, rows]
        out[c0:c0 + 1024] = sel[:, 0::4] | (sel[:, 1::4] << 2) | (sel[:, 2::4] << 4) | (sel[:, 3::4] << 6)
    return m.SnpLinAlg(out, n_out, center=x.center, scale=x.scale, impute=x.impute)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=200_000)
    ap.add_argument("--floor", action="store_true", help="100 000 x 20 000, subset timed against the host route")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (100_000, 20_000) if a.floor else (a.n, a.p)
    res = dict(n=n, p=p)
    t0 = time.perf_counter()
    x = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=0.01)
    res["synthetic_s"] = round(time.perf_counter() - t0, 3)
    rng = np.random.default_rng(a.seed)
    rmask, cmask = rng.random(n) >= 0.05, rng.random(p) >= 0.10
    rows, cols = np.flatnonzero(rmask), np.flatnonzero(cmask)
    x.counts(rmask)                                            # first call: code objects, allocations
    total_missing = int(x.counts()[0][:, 3].sum())
    src = tile_bytes(n, p)
    lists = 4 * total_missing + 8 * (p + 1)

    t, _ = median_of(lambda: x.counts(rmask))
    b = src + lists + n // 4
    res["counts"] = dict(s=round(t, 4), bytes=b, GBps=round(b / t / 1e9, 1), of_peak=round(b / t / HBM_PEAK, 4))

    def run_filter():                                          # (rounds = calls of counts, counted through the instance)
        calls = [0]
        inner = x.counts

        def counting(*args):
            calls[0] += 1
            return inner(*args)
        x.counts = counting
        try:
            return x.filter(), calls[0]
        finally:
            del x.counts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t, (masks, nrounds) = median_of(run_filter)
    res["filter"] = dict(s=round(t, 4), rounds=nrounds, rows_kept=int(masks[0].sum()), cols_kept=int(masks[1].sum()))

    t, sub = median_of(lambda: x.subset(rows, cols, reserve=False))
    kept_missing = int(sub.counts()[0][:, 3].sum())
    b = src + tile_bytes(rows.size, cols.size) + lists + 4 * kept_missing + 8 * (cols.size + 1)
    res["subset"] = dict(s=round(t, 4), shape=list(sub.shape), bytes=b, GBps=round(b / t / 1e9, 1), of_peak=round(b / t / HBM_PEAK, 4))
    if a.floor:
        th, host = median_of(lambda: host_route(x, rows, cols), reps=1)
        same = np.array_equal(host.export_bed(), sub.export_bed()) and all(
            np.array_equal(u, v, equal_nan=True) for u, v in zip(host.mu_sigma(), sub.mu_sigma()))
        res["host_route"] = dict(s=round(th, 3), ratio=round(th / t, 1), floor=10.0, same_matrix=bool(same))
        assert same, "the device subset and the host route disagree"
        assert th / t >= 10.0, f"subset is only {th / t:.1f}x faster than the host route (floor: 10x)"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
