"""The kinship matrix and the related-pair screen on the device (csrc/grm.hip), medians of 3, on a synthetic 2-bit matrix with
1 % missing genotypes: related_pairs(0.125) as a whole call, the symmetric update kernel's own time (HIP events around its
launches, through the profile hook of the handle) and the rate of the f64 matrix pipe that gives, beside the 78.6 TF/s of the
public specification -- a figure this project has not measured.

    python tools/bench_grm.py                     # 50 000 x 100 000
    python tools/bench_grm.py --floor             # 8 000 x 20 000: the device call against the host route, same pairs

The host route is what a caller had before: export_bed() -> numpy standardise -> X @ X.T with the BLAS threads the
environment gives (OMP_NUM_THREADS)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mendeliht_amd as m  # noqa: E402

F64_MATRIX_PEAK = 78.6e12
TILE = 128


def timed_pairs(x, **kw):
    """(seconds of the whole call, ms inside k_grm_update, the result)."""
    m.profile_passes(x)
    t0 = time.perf_counter()
    out = x.related_pairs(0.125, **kw)
    t = time.perf_counter() - t0
    ms = sum(r["ms"] for r in m.profile_passes(x) if r["kernel"] == "k_grm_update")
    return t, ms, out


def host_route(x, minmaf=0.01):
    """export_bed() -> allele counts -> the standardized float64 matrix of the columns with maf >= minmaf -> X X' / 2m."""
    bed = x.export_bed()
    n, p = x.n, x.p
    two = np.empty((p, bed.shape[1] * 4), dtype=np.uint8)
    for s in range(4):
        two[:, s::4] = (bed >> (2 * s)) & 3
    two = two[:, :n]
    miss = two == 1
    g = np.array([0.0, 0.0, 1.0, 2.0])[two]                   # (p, n)
    cnt = n - miss.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(miss, 0.0, g).sum(axis=1) / cnt
        f = mu / 2.0
        keep = np.minimum(f, 1.0 - f) >= minmaf
        s = np.sqrt(mu * (1.0 - mu / 2.0))
        sinv = np.where(s > 0, 1.0 / s, 1.0)
    X = (g[keep] - mu[keep, None]) * sinv[keep, None]
    X[miss[keep]] = 0.0
    phi = (X.T @ X) / (2.0 * int(keep.sum()))
    i, k = np.nonzero(np.triu(phi > 0.125, 1))
    return i, k, np.diag(phi).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000)
    ap.add_argument("--p", type=int, default=100_000)
    ap.add_argument("--floor", action="store_true", help="8 000 x 20 000, timed against the host route")
    ap.add_argument("--panel-cols", type=int, default=0)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (8_000, 20_000) if a.floor else (a.n, a.p)
    res = dict(n=n, p=p, panel_cols=a.panel_cols)
    t0 = time.perf_counter()
    x = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=0.01)
    res["synthetic_s"] = round(time.perf_counter() - t0, 3)
    kept = int(np.count_nonzero(x.maf() >= 0.01))
    x.related_pairs(0.125, cols=np.arange(64))                # first call: code objects
    m.profile_enable(x, True)
    runs = [timed_pairs(x, panel_cols=a.panel_cols) for _ in range(3)]
    t = statistics.median(r[0] for r in runs)
    ms = statistics.median(r[1] for r in runs)
    nt = (n + TILE - 1) // TILE
    flop = nt * (nt + 1) // 2 * TILE * TILE * 2.0 * kept       # what the matrix pipe executes: whole tiles of the lower triangle
    i, k, v, diag = runs[-1][2]
    res["related_pairs"] = dict(s=round(t, 4), cols_kept=kept, pairs=int(i.size), update_kernel_s=round(ms / 1e3, 4),
                                update_TFps=round(flop / (ms / 1e3) / 1e12, 2), of_spec_peak=round(flop / (ms / 1e3) / F64_MATRIX_PEAK, 3),
                                diag_mean=round(float(diag.mean()), 4))
    if a.floor:
        t0 = time.perf_counter()
        hi, hk, hdiag = host_route(x)
        th = time.perf_counter() - t0
        same = np.array_equal(hi, i) and np.array_equal(hk, k)
        res["host_route"] = dict(s=round(th, 3), ratio=round(th / t, 1), same_pairs=bool(same), threads=os.environ.get("OMP_NUM_THREADS"),
                                 max_abs_diff_diag=float(np.max(np.abs(hdiag - diag))))
        assert same, "the device call and the host route disagree on the pairs"
        assert np.max(np.abs(hdiag - diag)) <= 1e-9, "the device call and the host route disagree on the diagonal"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
