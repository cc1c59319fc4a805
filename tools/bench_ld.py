"""LD pruning of the 2-bit matrix on the device (csrc/ld.hip), medians of 3 whole calls on synthetic matrices: ld_prune as a
whole call, the band kernel's own time (HIP events around its launches, through the profile hook of the handle), the bytes
the kernel asks of memory and the matrix-core instructions it issues, and what share of the HBM peak and of the FP4 matrix rate
of the public specification (8 TB/s, 10 PF/s -- figures this project has not measured) that is.

    python tools/bench_ld.py                      # 500 000 x 200 000, 1 % missing and none: ld_prune(50, 5, 0.2), (512, 50, 0.2)
    python tools/bench_ld.py --ref                # 5 402 x 24 523 (NFBC after QC), all pairs: ld_prune(p, p, 0.2)
    python tools/bench_ld.py --floor              # 100 000 x 20 000, window 50: the device call against the host route, same mask

The host route is what a caller had before: export_bed() -> numpy (the BLAS threads the environment gives, OMP_NUM_THREADS) ->
the same greedy pass (tests/ld_spec.py)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mendeliht_amd as m  # noqa: E402
import ld_spec  # noqa: E402

HBM_PEAK = 8.0e12
FP4_PEAK = 10.0e15


def kernel_counts(n, p, window, missing):
    """(bytes loaded, MFMA wave instructions) of the band kernel over a whole call: every (group, partner) work item walks the
    128-row tiles of both groups -- of the mask image too where the panel has missing genotypes -- with 2 (8) MFMAs a step."""
    ncg, nbp, w = (p + 31) // 32, (n + 127) // 128, min(window, p)
    G = min((w + 30) // 32, ncg - 1)
    items = sum(min(G, ncg - 1 - a) + 1 for a in range(ncg))
    return items * nbp * 1024 * (4 if missing else 2), items * nbp * (8 if missing else 2)


def timed_prune(x, window, step, r2):
    m.profile_passes(x)
    t0 = time.perf_counter()
    keep = x.ld_prune(window, step, r2)
    t = time.perf_counter() - t0
    ms = sum(r["ms"] for r in m.profile_passes(x) if r["kernel"].startswith("k_ld_band"))
    return t, ms, keep


def measure(x, window, step, r2, missing):
    runs = [timed_prune(x, window, step, r2) for _ in range(3)]
    t, ms = statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)
    nbytes, mfma = kernel_counts(x.n, x.p, window, missing)
    flop = mfma * 32 * 32 * 64 * 2.0
    return dict(window=window, step=step, r2=r2, s=round(t, 4), band_kernel_s=round(ms / 1e3, 4), kept=int(runs[-1][2].sum()),
                kernel_bytes=nbytes, mfma=mfma, of_hbm_peak=round(nbytes / (ms / 1e3) / HBM_PEAK, 3),
                of_fp4_peak=round(flop / (ms / 1e3) / FP4_PEAK, 4)), runs[-1][2]


def host_route(x, window, step, r2, chunk=1024):
    """export_bed() -> mean-imputed centred float64 columns, a chunk at a time -> C'C with the BLAS -> the band of r -> the
    greedy pass of ld_spec.  Returns (mask, seconds of the band, seconds of the greedy pass)."""
    t0 = time.perf_counter()
    bed = x.export_bed()
    n, p = x.n, x.p
    w = min(window, p)
    rband = np.full((p, w - 1), np.nan)
    codes_all = np.empty((n, p), dtype=np.int8)
    lut = np.array([0, -1, 1, 2], dtype=np.int8)
    for a in range(0, p, chunk):
        b = min(p, a + chunk + w - 1)
        two = np.empty((b - a, bed.shape[1] * 4), dtype=np.uint8)
        for s in range(4):
            two[:, s::4] = (bed[a:b] >> (2 * s)) & 3
        codes = lut[two[:, :n]].T                                 # (n, b - a)
        codes_all[:, a:b] = codes
        obs = codes >= 0
        g = np.where(obs, codes, 0).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mu = g.sum(axis=0) / obs.sum(axis=0)
        c = np.where(obs, g - np.where(np.isfinite(mu), mu, 0.0)[None, :], 0.0)
        cov = c.T @ c
        d = np.diag(cov)
        with np.errstate(invalid="ignore", divide="ignore"):
            full = cov / np.sqrt(np.outer(d, d))
        full[~(d > 0)] = 0.0
        full[:, ~(d > 0)] = 0.0
        for j in range(a, min(p, a + chunk)):
            k1 = min(p, j + w)
            rband[j, :k1 - j - 1] = full[j - a, j - a + 1:k1 - a]
    t_band = time.perf_counter() - t0
    t0 = time.perf_counter()
    keep = ld_spec.prune(codes_all, window, step, r2, rband)
    return keep, t_band, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=200_000)
    ap.add_argument("--ref", action="store_true", help="5 402 x 24 523, all pairs")
    ap.add_argument("--floor", action="store_true", help="100 000 x 20 000, window 50, timed against the host route")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (5_402, 24_523) if a.ref else (100_000, 20_000) if a.floor else (a.n, a.p)
    calls = [(p, p, 0.2)] if a.ref else [(50, 5, 0.2)] if a.floor else [(50, 5, 0.2), (512, 50, 0.2)]
    res = dict(n=n, p=p)
    for rate in ((0.01,) if a.floor else (0.01, 0.0)):
        t0 = time.perf_counter()
        x = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=rate)
        key = "missing_1pct" if rate else "no_missing"
        res[key] = dict(synthetic_s=round(time.perf_counter() - t0, 3), calls=[])
        x.ld_prune(2, 1, 0.2, panel_cols=32)                      # first call: code objects
        m.profile_enable(x, True)
        for window, step, r2 in calls:
            out, keep = measure(x, window, step, r2, rate > 0)
            res[key]["calls"].append(out)
        if a.floor:
            window, step, r2 = calls[0]
            hkeep, t_band, t_greedy = host_route(x, window, step, r2)
            t = res[key]["calls"][0]["s"]
            same = bool(np.array_equal(hkeep, keep))
            res["host_route"] = dict(band_s=round(t_band, 2), greedy_s=round(t_greedy, 2), ratio=round((t_band + t_greedy) / t, 1),
                                     ratio_band_only=round(t_band / t, 1), same_mask=same, threads=os.environ.get("OMP_NUM_THREADS"))
            assert same, "the device call and the host route disagree on the mask"
        del x
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
