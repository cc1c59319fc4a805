"""The set-based tests on the device (csrc/assoc_sets.hip), medians of 3 whole calls on synthetic 2-bit matrices: x.set_test with a
logistic null model (an intercept and one covariate, 1 % cases) over consecutive windows of `--size` variants as a whole call, the
plain scan (x.score_test) on the same inputs, and the own times of k_assoc_set_gram and k_assoc_set_eig (HIP events around their
launches, through the profile hook of the handle); from those the rows x members the Gram kernel decodes per second and the f64
matrix-core rate it reaches over the padded blocks.

    python tools/bench_assoc_sets.py               # 500 000 x 1 000 000, 20 000 sets of 50
    python tools/bench_assoc_sets.py --small       # 100 000 x 20 000, 400 sets of 50
    python tools/bench_assoc_sets.py --floor       # 20 000 x 200, 4 sets of 50: the device call against export_bed() -> the numpy
                                                   # statement (tests/sets_spec.py)
    python tools/bench_assoc_sets.py --skato       # any of the shapes: beside the plain set call, the call with SKAT-O on the
                                                   # default grid (csrc/assoc_skato.hip), its two kernels and the ratio of the calls"""
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
from tools.bench_assoc_spa import inputs  # noqa: E402


def timed(x, null, Z, sets, skato=False):
    m.profile_passes(x)
    t0 = time.perf_counter()
    res = x.set_test(null.A, null.w, Z, sets, skato=skato)
    t = time.perf_counter() - t0
    recs = m.profile_passes(x)
    ms = lambda name: sum(r["ms"] for r in recs if r["kernel"] == name)
    return t, ms("k_assoc_set_gram"), ms("k_assoc_set_eig"), res, ms("k_assoc_set_rho"), ms("k_assoc_set_skato")


def host_route(x, null, Z, sets):
    """export_bed() -> allele counts -> the numpy statement of the scan and of the set tests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import assoc_spec as S
    import sets_spec as T
    t0 = time.perf_counter()
    bed = np.asarray(x.export_bed())
    n = x.n
    two = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n]
    codes = np.array([0, -1, 1, 2], dtype=np.int64)[two].T.copy()
    sp = S.score(codes, (1, 1, 1), null.A, null.w, Z)
    ptr, col = sets
    res = T.set_test(sp, null.w, [col[ptr[s]:ptr[s + 1]] for s in range(ptr.size - 1)])
    return res, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=1_000_000)
    ap.add_argument("--sets", type=int, default=20_000)
    ap.add_argument("--size", type=int, default=50)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--cases", type=float, default=0.01)
    ap.add_argument("--small", action="store_true", help="100 000 x 20 000, 400 sets")
    ap.add_argument("--floor", action="store_true", help="20 000 x 200, 4 sets, timed against the host route")
    ap.add_argument("--skato", action="store_true", help="time the call with SKAT-O on the default grid as well")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p, ns = (20_000, 200, 4) if a.floor else (100_000, 20_000, 400) if a.small else (a.n, a.p, a.sets)
    ns = min(ns, p // a.size)
    x = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=0.01 if a.floor else 0.0)
    y, Z, null = inputs(n, a.c, a.cases, a.seed)
    sets = (np.arange(ns + 1, dtype=np.int64) * a.size, np.arange(ns * a.size, dtype=np.int32))
    res = dict(n=n, p=p, c=a.c, sets=ns, size=a.size, cases=int(y.sum()), null_converged=bool(null.converged))
    x.set_test(null.A, null.w, Z, sets)                                       # first call: code objects
    plain = []
    for _ in range(3):
        t0 = time.perf_counter()
        x.score_test(null.A, null.w, Z)
        plain.append(time.perf_counter() - t0)
    m.profile_enable(x, True)
    runs = [timed(x, null, Z, sets) for _ in range(3)]
    oruns = [timed(x, null, Z, sets, skato=True) for _ in range(4)][1:] if a.skato else []      # (the first call loads the code objects)
    m.profile_enable(x, False)
    s, gms, ems = (statistics.median(r[k] for r in runs) for k in range(3))
    last = runs[-1][3]
    mem = float(last.m_used.sum())
    pad = float(((last.m_used + 15) // 16 * 16).astype(np.float64).sum())
    blocks = float((((last.m_used + 15) // 16) * ((last.m_used + 15) // 16 + 1) // 2).sum())
    res.update(plain_call_s=round(statistics.median(plain), 4), call_s=round(s, 4), gram_kernel_ms=round(gms, 3), eig_kernel_ms=round(ems, 3),
               members=int(mem), states=[int(v) for v in np.bincount(last.skat_state, minlength=6)],
               decoded_per_s=round(n * pad / max(gms, 1e-9) * 1e3, 0),
               gram_f64_flops_per_s=round(2.0 * 256.0 * blocks * (-(-n // 32) * 32) / max(gms, 1e-9) * 1e3, 0))
    if a.skato:
        so, rms, ims = (statistics.median(r[k] for r in oruns) for k in (0, 4, 5))
        o = oruns[-1][3]
        assert np.array_equal(o.neglog10p_skat, last.neglog10p_skat, equal_nan=True) and np.array_equal(o.lambdas, last.lambdas, equal_nan=True)
        res.update(skato_call_s=round(so, 4), rho_kernel_ms=round(rms, 3), skato_kernel_ms=round(ims, 3), skato_over_sets=round(so / s, 3),
                   skato_states=[int(v) for v in np.bincount(o.skato_state, minlength=5)],
                   skato_rho_counts=[int((o.skato_rho == r).sum()) for r in (0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0)])
    if a.floor:
        ref, th = host_route(x, null, Z, sets)
        same = np.array_equal(ref["skat_state"], last.skat_state) and np.array_equal(ref["m_used"], last.m_used)
        one = last.skat_state == 1
        rel = float(np.max(np.abs(ref["neglog10p_skat"][one] - last.neglog10p_skat[one]) / ref["neglog10p_skat"][one])) if one.any() else 0.0
        res["host_route"] = dict(s=round(th, 2), ratio=round(th / s, 1), states_equal=bool(same), max_rel_diff=rel)
        assert same and rel < 1e-8, "the device call and the host route disagree"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
