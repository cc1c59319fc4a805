"""The REML null model of the mixed-model scan on the device (csrc/lmm.hip), medians of 3 whole calls, on the synthetic 2-bit
matrix of bench_pca.py (1 % missing genotypes, --planted columns of population structure) with a phenotype of heritability
one half: y = X_c b / sqrt(|c|) + e over 500 causal columns.  Reported: lmm_null as a whole call, its REML and CG iterations,
the time of k_lmm_vmul per product (HIP events around its launches, through the profile hook of the handle) and its bytes/s
beside the 8 TB/s of the HBM specification, the update kernel's share of the call -- and k_pca_spmm per product at the same
block width (a pca() call with that block), so that the epilogue of k_lmm_vmul can be read off.

    python tools/bench_lmm.py                     # 50 000 x 100 000
    python tools/bench_lmm.py --floor             # 8 000 x 20 000: the device call against grm() -> the dense-solve spec in numpy

The host route is what a caller had before: x.grm() brings Phi home and tests/lmm_spec.py's dense-solve form fits the model
with the BLAS threads the environment gives (OMP_NUM_THREADS)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mendeliht_amd as m  # noqa: E402
from bench_pca import planted_bed  # noqa: E402

HBM_PEAK = 8.0e12
TILE = 128


def decode(bed, n):
    """Mean-imputed, standardised allele counts (n x cols) of PLINK columns."""
    two = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n]
    g = np.array([0.0, np.nan, 1.0, 2.0])[two].T
    mu = np.nanmean(g, axis=0)
    g = np.where(np.isnan(g), mu[None, :], g) - mu[None, :]
    sd = g.std(axis=0)
    return g / np.where(sd > 0, sd, 1.0)[None, :]


def timed_null(x, y, z, **kw):
    """(seconds of the whole call, ms of every k_lmm_vmul launch of the widest block, ms inside k_grm_update, the result)."""
    m.profile_passes(x)
    t0 = time.perf_counter()
    out = x.lmm_null(y, z, **kw)
    t = time.perf_counter() - t0
    recs = m.profile_passes(x)
    wide = max((r["residuals"] for r in recs if r["kernel"] == "k_lmm_vmul"), default=0)
    return (t, [r["ms"] for r in recs if r["kernel"] == "k_lmm_vmul" and r["residuals"] == wide], sum(r["ms"] for r in recs if r["kernel"] == "k_grm_update"),
            out, wide, sum(1 for r in recs if r["kernel"] == "k_lmm_vmul"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000)
    ap.add_argument("--p", type=int, default=100_000)
    ap.add_argument("--planted", type=int, default=2_000, help="columns overwritten with population structure")
    ap.add_argument("--floor", action="store_true", help="8 000 x 20 000, timed against grm() -> the dense-solve spec in numpy")
    ap.add_argument("--probes", type=int, default=30)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (8_000, 20_000) if a.floor else (a.n, a.p)
    res = dict(n=n, p=p, planted=a.planted, probes=a.probes)
    t0 = time.perf_counter()
    bed = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=0.01).export_bed()
    rng = np.random.default_rng(a.seed)
    at = np.sort(rng.choice(p, size=min(a.planted, p), replace=False))
    bed[at] = planted_bed(n, at.size, 3, rng)
    causal = np.sort(rng.choice(p, size=500, replace=False))
    xc = decode(bed[causal], n)
    y = xc @ rng.standard_normal(500) / np.sqrt(500.0) + rng.standard_normal(n)
    z = np.column_stack([np.ones(n), rng.standard_normal((n, 2))])
    y = y + z @ np.array([1.0, 0.5, -0.5])
    x = m.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    del bed, xc
    res["build_s"] = round(time.perf_counter() - t0, 3)
    x.kinship_solve(np.ones(n), 1.0, 1.0, cols=np.arange(64), max_iter=2)          # first calls: code objects
    x.pca(1, cols=np.arange(64), max_iter=2)
    m.profile_enable(x, True)
    runs = [timed_null(x, y, z, probes=a.probes) for _ in range(3)]
    t = statistics.median(r[0] for r in runs)
    out, wide = runs[-1][3], runs[-1][4]
    per = statistics.median(ms for r in runs for ms in r[1])
    spread = [round(statistics.median(r[1]), 4) for r in runs]
    n_pad = (n + TILE - 1) // TILE * TILE
    nbytes = 8.0 * n_pad * n_pad
    res["lmm_null"] = dict(s=round(t, 4), all_s=[round(r[0], 4) for r in runs], reml_iters=out.iters, state=out.state, cg_iters=out.cg_iters,
                           products=runs[-1][5], tau=[float(v) for v in out.tau], h2=round(out.h2, 4), gamma=round(out.gamma, 4), ratio_cv=round(out.ratio_cv, 4),
                           worst_residual=out.worst_residual, block=wide, vmul_ms=round(per, 4), vmul_ms_by_run=spread,
                           vmul_TBps=round(nbytes / (per / 1e3) / 1e12, 3), of_hbm_peak=round(nbytes / (per / 1e3) / HBM_PEAK, 3),
                           grm_update_s=round(statistics.median(r[2] for r in runs) / 1e3, 4))
    # k_pca_spmm at the same block width, the two kernels alternating: three pca calls of six products each
    spmm = []
    for _ in range(3):
        m.profile_passes(x)
        x.pca(10, block=wide, max_iter=6)
        spmm.append(statistics.median(r["ms"] for r in m.profile_passes(x) if r["kernel"] == "k_pca_spmm"))
    res["k_pca_spmm"] = dict(block=wide, ms=round(statistics.median(spmm), 4), ms_by_run=[round(v, 4) for v in spmm])
    if a.floor:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import lmm_spec as L
        t0 = time.perf_counter()
        phi = x.grm()
        t_grm = time.perf_counter() - t0
        G = x._marker_genotypes(out.marker_cols)
        f = L.reml(phi, y, z, nprobes=a.probes, G=G, solver="dense")
        th = time.perf_counter() - t0
        res["host_route"] = dict(s=round(th, 3), grm_s=round(t_grm, 3), reml_s=round(th - t_grm, 3), ratio=round(th / t, 1),
                                 threads=os.environ.get("OMP_NUM_THREADS"), iters=f.iters, state=f.state, tau=[float(v) for v in f.tau],
                                 max_rel_diff_tau=float(np.max(np.abs(f.tau - out.tau) / f.tau)), rel_diff_gamma=abs(f.gamma - out.gamma) / f.gamma)
        assert f.iters == out.iters and f.state == out.state, "the device call and the host route disagree on the iterations"
        assert res["host_route"]["max_rel_diff_tau"] <= 1e-6, "the device call and the host route disagree on tau"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
