"""The Firth-penalised association scan on the device (csrc/assoc_firth.hip), medians of 3 whole calls on synthetic 2-bit
matrices: x.score_test_firth with a logistic null model (an intercept and one covariate, 1 % cases, cutoff 2.0) as a whole call,
the plain scan (x.score_test) and the saddlepoint call (x.score_test_spa) on the same inputs, k_assoc_firth's and k_assoc_spa's
own times (HIP events around their launches, through the profile hook of the handle), the number of flagged columns, the mean
number of evaluations of (K1 .. K4) per column, and from those the row evaluations per second and the bytes per second
k_assoc_firth reads from its slabs.

    python tools/bench_assoc_firth.py               # 500 000 x 1 000 000
    python tools/bench_assoc_firth.py --small       # 100 000 x 20 000
    python tools/bench_assoc_firth.py --floor       # 20 000 x 200 with 1 % missing: the device call against export_bed() -> the
                                                    # numpy statement (tests/firth_spec.py, the columns spread over 16 threads)"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mendeliht_amd as m  # noqa: E402


def inputs(n, c, share, seed):
    """y with `share` cases under a logistic model of the covariates, and its fitted null model."""
    rng = np.random.default_rng(seed)
    Z = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1)
    lin = np.log(share / (1.0 - share)) + 0.3 * Z[:, 1:].sum(axis=1)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)
    null = m.fit_null(y, Z, m.Bernoulli())
    return y, Z, null


def timed(x, null, Z, cutoff, firth):
    """One whole call with the hook on: (seconds, kernel ms, flagged columns, solves, evaluations, result)."""
    m.profile_passes(x)
    t0 = time.perf_counter()
    if firth:
        res = x.score_test_firth(null.A, null.w, Z, null.eta, cutoff=cutoff)
    else:
        res = x.score_test_spa(null.A, null.w, Z, null.eta, cutoff=cutoff)
    t = time.perf_counter() - t0
    recs = m.profile_passes(x)
    k = [r for r in recs if r["kernel"] == ("k_assoc_firth" if firth else "k_assoc_spa")]
    e = [r for r in recs if r["kernel"] == ("assoc_firth_evals" if firth else "assoc_spa_evals")]
    return t, sum(r["ms"] for r in k), (k[0]["operands"] if k else 0), (e[0]["residuals"] if e else 0), (e[0]["operands"] if e else 0), res


def host_route(x, null, Z, cutoff, threads=16):
    """export_bed() -> allele counts -> the numpy statement of the plain scan and of the Firth pass, the flagged columns spread
    over `threads` threads."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import assoc_spec as S
    import firth_spec as F
    t0 = time.perf_counter()
    bed = np.asarray(x.export_bed())
    n, p = x.n, x.p
    two = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n]
    codes = np.array([0, -1, 1, 2], dtype=np.int64)[two].T.copy()
    sp = S.score(codes, (1, 1, 1), null.A, null.w, Z)
    flagged = [j for j in range(p) if not np.isnan(sp["z"][j, 0]) and abs(sp["z"][j, 0]) >= cutoff]
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda j: F.firth(sp, null.eta, Z, cutoff, columns=[j]), flagged))
    base = F.firth(sp, null.eta, Z, np.inf)
    beta, nlp, state = base["beta_firth"], base["neglog10p_firth"], base["state"]
    for j, r in zip(flagged, parts):
        beta[j], nlp[j], state[j] = r["beta_firth"][j], r["neglog10p_firth"][j], r["state"][j]
    return beta, nlp, state, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--p", type=int, default=1_000_000)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--cases", type=float, default=0.01)
    ap.add_argument("--cutoff", type=float, default=2.0)
    ap.add_argument("--small", action="store_true", help="100 000 x 20 000")
    ap.add_argument("--floor", action="store_true", help="20 000 x 200, timed against the host route")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n, p = (20_000, 200) if a.floor else (100_000, 20_000) if a.small else (a.n, a.p)
    x = m.SnpLinAlg.synthetic(n, p, seed=a.seed, missing_rate=0.01 if a.floor else 0.0)
    y, Z, null = inputs(n, a.c, a.cases, a.seed)
    res = dict(n=n, p=p, c=a.c, cases=int(y.sum()), cutoff=a.cutoff, null_converged=bool(null.converged))
    x.score_test_firth(null.A, null.w, Z, null.eta, cutoff=a.cutoff)          # first calls: code objects
    x.score_test_spa(null.A, null.w, Z, null.eta, cutoff=a.cutoff)
    plain = []
    for _ in range(3):
        t0 = time.perf_counter()
        x.score_test(null.A, null.w, Z)
        plain.append(time.perf_counter() - t0)
    m.profile_enable(x, True)
    runs = [timed(x, null, Z, a.cutoff, True) for _ in range(3)]
    spa_runs = [timed(x, null, Z, a.cutoff, False) for _ in range(3)]
    m.profile_enable(x, False)
    s, kms = (statistics.median(r[k] for r in runs) for k in range(2))
    ss, skms = (statistics.median(r[k] for r in spa_runs) for k in range(2))
    _, _, flagged, solves, evals, last = runs[-1]
    _, _, _, tails, spa_evals, _ = spa_runs[-1]
    st = np.bincount(last.firth_state, minlength=3)
    rows = float(n) * (evals + 2 * solves)            # the evaluations, the pass at the root and the pass that forms c_i of every column
    spa_rows = float(n) * (spa_evals + tails + flagged)
    res.update(plain_call_s=round(statistics.median(plain), 4), call_s=round(s, 4), firth_kernel_ms=round(kms, 3), flagged=int(flagged),
               evals_per_column=round(evals / max(solves, 1), 2), states=[int(v) for v in st],
               row_evals_per_s=round(rows / max(kms, 1e-9) * 1e3, 0), slab_bytes_per_s=round(8.0 * rows / max(kms, 1e-9) * 1e3, 0),
               spa_call_s=round(ss, 4), spa_kernel_ms=round(skms, 3), spa_evals_per_column=round(spa_evals / max(flagged, 1), 2),
               spa_row_evals_per_s=round(spa_rows / max(skms, 1e-9) * 1e3, 0), firth_over_spa_kernel=round(kms / max(skms, 1e-9), 3))
    if a.floor:
        beta, nlp, state, th = host_route(x, null, Z, a.cutoff)
        same = np.array_equal(state, last.firth_state)
        one = (state == 1) & (last.firth_state == 1)
        rel = float(np.max(np.abs(nlp[one] - last.neglog10p_firth[one]) / nlp[one])) if one.any() else 0.0
        relb = float(np.max(np.abs(beta[one] - last.beta_firth[one]) / np.abs(beta[one]))) if one.any() else 0.0
        res["host_route"] = dict(s=round(th, 2), ratio=round(th / s, 1), states_equal=bool(same), max_rel_diff_neglog10p=rel, max_rel_diff_beta=relb,
                                 threads=16)
        assert rel < 1e-9 and relb < 1e-9, "the device call and the host route disagree"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
