"""The leading principal components on the device (csrc/pca.hip), medians of 3, on the synthetic 2-bit matrix of bench_grm.py
(1 % missing genotypes) with planted population structure added: --planted of its columns are overwritten with genotypes of
k + 1 populations (sizes proportional to 1, 2, 3, ..., Balding-Nichols frequencies with F_ST = 0.1), so that the k leading
eigenvalues stand clear of the bulk.  Reported: pca(k) as a whole call, the Phi Q kernel's time per product (HIP events around
its launches, through the profile hook of the handle), its bytes/s beside the 8 TB/s of the HBM specification and its flop/s
beside the 59 TF/s this project measured in k_grm_update, the update kernel's share of the call, and the iteration count.

    python tools/bench_pca.py                     # 50 000 x 100 000
    python tools/bench_pca.py --floor             # 8 000 x 20 000: the device call against grm() -> numpy.linalg.eigh

The host route is what a caller had before: x.grm() brings Phi home and numpy.linalg.eigh solves it with the BLAS threads the
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

HBM_PEAK = 8.0e12
GRM_UPDATE_RATE = 59e12
TILE = 128


def planted_bed(n, cols, k, rng):
    """PLINK columns (cols, ceil(n / 4)) of k + 1 populations: 0 -> 00, 1 -> 10, 2 -> 11."""
    pops = k + 1
    share = np.arange(1, pops + 1, dtype=np.float64)
    edges = np.floor(np.cumsum(share) / share.sum() * n + 0.5).astype(int)
    label = np.searchsorted(edges, np.arange(n), side="right").clip(0, pops - 1)
    anc = rng.uniform(0.1, 0.9, cols)
    fst = 0.1
    f = rng.beta(anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst, size=(pops, cols))
    code = np.zeros((cols, (n + 3) // 4 * 4), dtype=np.uint8)
    code[:, :n] = np.array([0, 2, 3], dtype=np.uint8)[rng.binomial(2, f[label]).T]
    return code[:, 0::4] | (code[:, 1::4] << 2) | (code[:, 2::4] << 4) | (code[:, 3::4] << 6)


def timed_pca(x, k, **kw):
    """(seconds of the whole call, ms of every k_pca_spmm launch, ms inside k_grm_update, the result)."""
    m.profile_passes(x)
    t0 = time.perf_counter()
    out = x.pca(k, **kw)
    t = time.perf_counter() - t0
    recs = m.profile_passes(x)
    return (t, [r["ms"] for r in recs if r["kernel"] == "k_pca_spmm"], sum(r["ms"] for r in recs if r["kernel"] == "k_grm_update"), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000)
    ap.add_argument("--p", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--planted", type=int, default=2_000, help="columns overwritten with population structure")
    ap.add_argument("--floor", action="store_true", help="8 000 x 20 000, timed against grm() -> numpy.linalg.eigh")
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (8_000, 20_000) if a.floor else (a.n, a.p)
    k = a.k
    res = dict(n=n, p=p, k=k, planted=a.planted)
    t0 = time.perf_counter()
    bed = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=0.01).export_bed()
    rng = np.random.default_rng(a.seed)
    at = np.sort(rng.choice(p, size=min(a.planted, p), replace=False))
    bed[at] = planted_bed(n, at.size, k, rng)
    x = m.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    del bed
    res["build_s"] = round(time.perf_counter() - t0, 3)
    kept = int(np.count_nonzero(x.maf() >= 0.01))
    x.pca(1, cols=np.arange(64), max_iter=2)                  # first call: code objects
    m.profile_enable(x, True)
    runs = [timed_pca(x, k, block=a.block) for _ in range(3)]
    t = statistics.median(r[0] for r in runs)
    out = runs[-1][3]
    per = statistics.median(ms for r in runs for ms in r[1])
    upd = statistics.median(r[2] for r in runs)
    n_pad = (n + TILE - 1) // TILE * TILE
    b = a.block or -(-max(2 * k, k + 8) // 16) * 16
    bp = -(-min(b, n) // 16) * 16
    nbytes = 8.0 * n_pad * n_pad
    flop = 2.0 * n_pad * n_pad * bp
    res["pca"] = dict(s=round(t, 4), cols_kept=kept, iters=out.iters, converged=out.converged, block=bp,
                      values=[round(float(v), 6) for v in out.values], max_residual=float(out.residuals.max()),
                      grm_update_s=round(upd / 1e3, 4), products=len(runs[-1][1]), product_ms=round(per, 4),
                      products_s=round(sum(runs[-1][1]) / 1e3, 4),
                      product_TBps=round(nbytes / (per / 1e3) / 1e12, 3), of_hbm_peak=round(nbytes / (per / 1e3) / HBM_PEAK, 3),
                      product_TFps=round(flop / (per / 1e3) / 1e12, 2), of_grm_update_rate=round(flop / (per / 1e3) / GRM_UPDATE_RATE, 3))
    if a.floor:
        t0 = time.perf_counter()
        phi = x.grm()
        t_grm = time.perf_counter() - t0
        w, v = np.linalg.eigh(phi)
        th = time.perf_counter() - t0
        w, v = w[::-1][:k], v[:, ::-1][:, :k]
        dv = float(np.max(np.abs(w - out.values)))
        sub = float(np.linalg.norm(out.vectors - v @ (v.T @ out.vectors)))
        res["host_route"] = dict(s=round(th, 3), grm_s=round(t_grm, 3), eigh_s=round(th - t_grm, 3), ratio=round(th / t, 1),
                                 threads=os.environ.get("OMP_NUM_THREADS"), max_abs_diff_values=dv, subspace_distance=sub)
        assert dv <= 1e-8 * w[0], "the device call and the host route disagree on the eigenvalues"
        assert sub <= 1e-6, "the device call and the host route disagree on the subspace"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
