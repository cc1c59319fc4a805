"""A digest of three debias=true fits (Normal k = 7 and 20, Poisson k = 40) on a seeded synthetic matrix: everything a fit returns,
hashed.  Run it on two builds of the PRODUCT library -- MENDELIHT_HIP_LIB=<other build>/libmendeliht_hip.so selects one -- to show
that a change to csrc/debias.hip left the refit's bits alone (the hook of mih_probe_debias_glm is compiled into the measurement
build only)."""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mendeliht_amd as m
x = m.SnpLinAlg.synthetic(3001, 2000, seed=11, missing_rate=0.01)
rng = np.random.default_rng(5)
for k, fam in ((7, "normal"), (20, "normal"), (40, "poisson")):
    supp = np.sort(rng.choice(x.p, k, replace=False))
    eta = x.xv_sparse(supp, rng.standard_normal(k) / np.sqrt(k))
    if fam == "normal":
        y, kw = 2 * eta + 0.5 + rng.standard_normal(x.n), {}
    else:
        y, kw = rng.poisson(np.exp(0.8 * eta)).astype(float), dict(d=m.Poisson(), l=m.LogLink())
    res = m.fit_iht(y, x, None, k=k, debias=True, verbose=False, **kw)
    h = hashlib.sha256()
    for a in (res.beta, res.c, np.asarray(res.trace["logl"]), np.asarray(res.trace["tol"]), np.asarray(res.mu)):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    print(os.environ.get("MENDELIHT_HIP_LIB", m.library_path()), fam, "k", k, "iter", res.iter, h.hexdigest()[:32], flush=True)
