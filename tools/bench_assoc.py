"""The marginal association scan on the device (csrc/assoc.hip), medians of 3 whole calls on synthetic matrices: x.score_test
with logistic working weights as a whole call, the class kernel's own time (HIP events around its launch, through the profile
hook of the handle) and the fused X'R pass's, the bytes the class kernel asks of memory and the matrix-core instructions it
issues, what share of the HBM peak and of the FP4 matrix rate of the public specification (8 TB/s, 10 PF/s -- figures this
project has not measured) that is, and the single-residual X'r pass (mih_bench_xtv, m = 1) on the same matrix for comparison.

    python tools/bench_assoc.py                   # 500 000 x 1 000 000, t = 1, c = 2 (3 residuals: one fused pass)
    python tools/bench_assoc.py --c 18            # 19 residuals: the full width of a fused pass
    python tools/bench_assoc.py --floor           # 100 000 x 20 000: the device call against the host route, same statistics

The host route is what a caller had before: export_bed() -> numpy (the BLAS threads the environment gives, OMP_NUM_THREADS) ->
the same score test (X'[A | w o Z] and X^2' w by the BLAS, a chunk of columns at a time)."""
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

HBM_PEAK = 8.0e12
FP4_PEAK = 10.0e15


def kernel_counts(n, p):
    """(bytes loaded, MFMA wave instructions) of the class kernel: every pair of column groups walks its 128-row tiles (1 KB
    each) and, once per pair, the two 1 KB digit operands of the step (those come from the cache); four MFMAs a tile."""
    ncg, nbp = (p + 31) // 32, (n + 127) // 128
    return ncg * nbp * 1024, (ncg + 1) // 2 * nbp * 2048, ncg * nbp * 4


def inputs(n, t, c, seed):
    rng = np.random.default_rng(seed)
    Z = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1)
    mu = 1.0 / (1.0 + np.exp(-0.8 * rng.standard_normal(n)))
    w = mu * (1.0 - mu)
    A = (rng.random((n, t)) < mu[:, None]).astype(np.float64) - mu[:, None]
    wz = w[:, None] * Z
    return A - wz @ np.linalg.solve(Z.T @ wz, Z.T @ A), w, Z


def timed(x, A, w, Z):
    m.profile_passes(x)
    t0 = time.perf_counter()
    res = x.score_test(A, w, Z)
    t = time.perf_counter() - t0
    recs = m.profile_passes(x)
    cls = sum(r["ms"] for r in recs if r["kernel"].startswith("k_assoc_classes"))
    xtv = sum(r["ms"] for r in recs if r["kernel"].startswith("k_xtv"))
    return t, cls, xtv, res


def host_route(x, A, w, Z, chunk=2048):
    """export_bed() -> the standardized float64 columns, a chunk at a time -> the linear and quadratic terms with the BLAS -> z."""
    t0 = time.perf_counter()
    bed = x.export_bed()
    n, p = x.n, x.p
    R = np.concatenate([A, w[:, None] * Z], axis=1)
    t = A.shape[1]
    Linv = np.linalg.inv(np.linalg.cholesky(Z.T @ (w[:, None] * Z)))
    lut = np.array([0, -1, 1, 2], dtype=np.int8)
    z = np.empty((p, t))
    for a in range(0, p, chunk):
        b = min(p, a + chunk)
        two = np.empty((b - a, bed.shape[1] * 4), dtype=np.uint8)
        for s in range(4):
            two[:, s::4] = (bed[a:b] >> (2 * s)) & 3
        codes = lut[two[:, :n]].T
        obs = codes >= 0
        g = np.where(obs, codes, 0).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mu = g.sum(axis=0) / obs.sum(axis=0)
            sinv = 1.0 / np.sqrt(mu * (1.0 - mu / 2.0))
            X = np.where(obs, (g - mu[None, :]) * sinv[None, :], 0.0)
            S = X.T @ R
            Q = (X * X).T @ w
            u = S[:, t:] @ Linv.T
            V = Q - (u * u).sum(axis=1)
            z[a:b] = S[:, :t] / np.sqrt(V)[:, None]
    return z, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=1_000_000)
    ap.add_argument("--t", type=int, default=1)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--floor", action="store_true", help="100 000 x 20 000, timed against the host route")
    ap.add_argument("--missing", type=float, default=None, help="share of missing genotypes (default 0, and 0.01 with --floor)")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (100_000, 20_000) if a.floor else (a.n, a.p)
    rate = a.missing if a.missing is not None else 0.01 if a.floor else 0.0
    t0 = time.perf_counter()
    x = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=rate)
    res = dict(n=n, p=p, t=a.t, c=a.c, missing=rate, synthetic_s=round(time.perf_counter() - t0, 3))
    A, w, Z = inputs(n, a.t, a.c, a.seed)
    x.score_test(A, w, Z)                                          # first call: code objects
    m.profile_enable(x, True)
    runs = [timed(x, A, w, Z) for _ in range(3)]
    m.profile_enable(x, False)
    s, cls, xtv = (statistics.median(r[k] for r in runs) for k in range(3))
    hbm, cache, mfma = kernel_counts(n, p)
    res.update(call_s=round(s, 4), class_kernel_ms=round(cls, 3), fused_pass_ms=round(xtv, 3), class_hbm_bytes=hbm, class_cache_bytes=cache,
               class_mfma=mfma, class_of_hbm_peak=round(hbm / (cls / 1e3) / HBM_PEAK, 3),
               class_of_fp4_peak=round(mfma * 32 * 32 * 64 * 2.0 / (cls / 1e3) / FP4_PEAK, 4))
    ms1, _ = x.bench_xtv(iters=10, warmup=2)
    res["single_residual_pass_ms"] = round(float(ms1), 3)
    if a.floor:
        zh, th = host_route(x, A, w, Z)
        zd = runs[-1][3].z.reshape(p, -1)
        ok = ~np.isnan(zd[:, 0])
        res["host_route"] = dict(s=round(th, 2), ratio=round(th / s, 1), max_abs_z_diff=float(np.abs(zh[ok] - zd[ok]).max()),
                                 threads=os.environ.get("OMP_NUM_THREADS"))
        assert res["host_route"]["max_abs_z_diff"] < 1e-6, "the device call and the host route disagree"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
