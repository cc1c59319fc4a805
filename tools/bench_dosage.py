"""X'r on the 16-bit dosage matrix: mih_bench_xtv on DosageMatrix.synthetic(500 000, 100 000, denom=255) -- a 100 GB image
(400 GB as Float64, beyond one device) -- for one residual and a fused pass of m = 8.  Prints ms, TB/s of the algorithmic
bytes (2 n p + 8 m (n + p)) and the fraction of 8 TB/s.

    python tools/bench_dosage.py [--n N] [--p P] [--iters K]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mendeliht_amd as m  # noqa: E402

HBM_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=100_000)
    ap.add_argument("--denom", type=int, default=255)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    x = m.DosageMatrix.synthetic(a.n, a.p, seed=2024, denom=a.denom)
    for rhs in (1, 8):
        ms, checksum = x.bench_xtv_batched(rhs, iters=a.iters, warmup=2)
        tbs = x.algorithmic_bytes(rhs) / (ms * 1e-3) / 1e12
        print(json.dumps({"n": a.n, "p": a.p, "denom": a.denom, "m": rhs, "ms": round(ms, 3), "ms_per_residual": round(ms / rhs, 3),
                          "TB_s": round(tbs, 3), "frac_of_8TBs": round(tbs / HBM_TBS, 3), "checksum": checksum}), flush=True)


if __name__ == "__main__":
    main()
