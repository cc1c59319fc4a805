"""The transposed image and the dense forward product on the device (csrc/transpose.hip, csrc/xb.hip), medians of 3, on a
synthetic 2-bit matrix with 1 % missing genotypes:

  transpose   x.transpose(reserve=-1) as a whole call (allocation, tiles, scatter of the missing genotypes, statistics, lists), and
              the bytes of both images over that time as a share of the 8 TB/s of the public specification;
  xb          for t = 1, 19, 20, 32: the time inside the pass kernels of x.xb(B) (HIP events around their launches, through the
              profile hook of the row image) beside the same of x.xtv(R) with t residuals on the original handle -- the same
              kernels on a matrix of the same byte count and another aspect ratio; their ratio is the figure of merit -- and the
              whole calls, uploads and allocations included.

    python tools/bench_xb.py                      # 500 000 x 200 000
    python tools/bench_xb.py --n 100000 --p 20000
    python tools/bench_xb.py --floor              # 20 000 x 2 000: both against the host routes

The host routes are what a caller had before: export_bed() -> numpy -> SnpLinAlg of the transposed codes, and the standardised
float64 matrix times B with the BLAS threads the environment gives (OMP_NUM_THREADS)."""
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

HBM_SPEC = 8.0e12
T_LIST = (1, 19, 20, 32)


def image_bytes(n, p):
    return ((p + 31) // 32) * ((n + 127) // 128) * 1024


def pass_ms(h):
    return sum(r["ms"] for r in m.profile_passes(h))


def codes_of(bed, n):
    two = np.empty((bed.shape[0], bed.shape[1] * 4), dtype=np.uint8)
    for s in range(4):
        two[:, s::4] = (bed >> (2 * s)) & 3
    return two[:, :n]                                            # (p, n) PLINK codes


def host_transpose(x):
    """export_bed() -> numpy -> the .bed columns of the transposed codes -> SnpLinAlg."""
    two = codes_of(x.export_bed(), x.n).T                        # (n, p): rows of the new matrix are SNPs
    pad = np.zeros((x.n, (x.p + 3) // 4 * 4), dtype=np.uint8)
    pad[:, :x.p] = two
    bed = (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)
    return m.SnpLinAlg(bed, x.p, center=x.center, scale=x.scale, impute=x.impute)


def host_xb(x, B):
    two = codes_of(x.export_bed(), x.n)
    miss = two == 1
    g = np.array([0.0, 0.0, 1.0, 2.0])[two]
    mu, sinv = x.mu_sigma()
    X = (g - mu[:, None]) * sinv[:, None]
    X[miss] = 0.0
    return X.T @ B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=200_000)
    ap.add_argument("--floor", action="store_true", help="20 000 x 2 000, timed against the host routes")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (20_000, 2_000) if a.floor else (a.n, a.p)
    res = dict(n=n, p=p)
    x = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=0.01, reserve=False)
    x.transpose(reserve=-1)                                      # first call: code objects
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        xt = x.transpose(reserve=-1)
        ts.append(time.perf_counter() - t0)
        del xt
    t = statistics.median(ts)
    moved = image_bytes(n, p) + image_bytes(p, n)
    res["transpose"] = dict(s=round(t, 4), bytes_moved=moved, of_hbm_spec=round(moved / t / HBM_SPEC, 4))
    rng = np.random.default_rng(a.seed)
    x.row_image(True)
    m.profile_enable(x, True)
    m.profile_enable(x._rows, True)
    x.xb(rng.standard_normal(p))
    x.xtv(rng.standard_normal((n, 2)))
    res["xb"] = {}
    for t_cols in T_LIST:
        B, R = rng.standard_normal((p, t_cols)), rng.standard_normal((n, t_cols))
        runs = []
        for _ in range(3):
            pass_ms(x._rows), pass_ms(x)
            t0 = time.perf_counter()
            x.xb(B)
            t1 = time.perf_counter()
            kb = pass_ms(x._rows)
            t2 = time.perf_counter()
            x.xtv(R)
            t3 = time.perf_counter()
            runs.append((t1 - t0, kb, t3 - t2, pass_ms(x)))
        call_b, k_b, call_t, k_t = (statistics.median(r[i] for r in runs) for i in range(4))
        res["xb"][t_cols] = dict(xb_pass_ms=round(k_b, 3), xtv_pass_ms=round(k_t, 3), ratio=round(k_b / k_t, 3) if k_t else None,
                                 xb_call_s=round(call_b, 4), xtv_call_s=round(call_t, 4))
    if a.floor:
        t0 = time.perf_counter()
        ht = host_transpose(x)
        th = time.perf_counter() - t0
        same = np.array_equal(ht.export_bed(), x._rows.export_bed())
        res["host_transpose"] = dict(s=round(th, 3), ratio=round(th / t, 1), same_codes=bool(same))
        B = rng.standard_normal((p, 19))
        t0 = time.perf_counter()
        want = host_xb(x, B)
        th = time.perf_counter() - t0
        got = x.xb(B, center=True, scale=True, impute=True)
        res["host_xb"] = dict(s=round(th, 3), ratio=round(th / res["xb"][19]["xb_call_s"], 1), threads=os.environ.get("OMP_NUM_THREADS"),
                              max_abs_diff=float(np.max(np.abs(got - want))))
        assert same, "the device transpose and the host route disagree"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
