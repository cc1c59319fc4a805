"""A digest of the association scan: one line per case, a label and a SHA-256 over the bytes of everything the call returned.
Run it on two builds or two trees to show that a change to csrc/assoc*.hip, or to the association methods of api.py, left every
bit alone: the lines must be identical.  It uses the public Python API only, on seeded inputs of the smallest shapes at which
each path is taken (score_test over both row-slice plans, an even and an odd count of column groups, one and several traits and
covariates; the per-column solvers at n = 257, single rows only, and n = 1025, four at a time plus a tail; sets on both sides of
the 16-member block and the 64-member LDS limit), on every handle kind."""
import hashlib, itertools, os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mendeliht_amd as m

FIX = os.path.join(ROOT, "tests", "fixtures")
ASSOC_FIELDS = ("z", "beta", "se", "neglog10p", "wsum", "neglog10p_spa", "spa_state", "t_hat", "beta_firth", "se_firth",
                "neglog10p_firth", "firth_state", "firth_evals")
SET_FIELDS = ("set_ptr", "set_col", "omega", "m_used", "burden_z", "neglog10p_burden", "skat_q", "neglog10p_skat", "skat_state", "lambdas")


def feed(h, name, a):
    h.update(name.encode())
    if a is None:
        h.update(b"<none>")
        return
    a = np.ascontiguousarray(a)
    h.update(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())


def feed_null(h, null):
    for one in (null if isinstance(null, list) else [null]):
        for f in ("gamma", "eta", "mu", "phi", "A", "w", "dev", "iters", "converged"):
            feed(h, "null." + f, None if getattr(one, f) is None else np.asarray(getattr(one, f)))


def feed_assoc(h, res):
    for f in ASSOC_FIELDS:
        feed(h, f, getattr(res, f))
    if res.null is not None:
        feed_null(h, res.null)


def feed_sets(h, res):
    for f in SET_FIELDS:
        feed(h, f, getattr(res, f))
    for k, c in enumerate(res.cov or []):
        feed(h, f"cov{k}", c)
    feed_assoc(h, res.assoc)


def show(label, fill, res):
    h = hashlib.sha256()
    fill(h, res)
    print(label, h.hexdigest(), flush=True)


def bed_columns(rng, n, p, miss, mono=()):
    """p columns of PLINK 2-bit codes (0 and 3 homozygous, 2 heterozygous, 1 missing), four rows a byte; mono: columns of one class"""
    codes = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=(p, 4 * ((n + 3) // 4)), p=[0.5, miss, 0.3, 0.2 - miss])
    codes[:, n:] = 0
    for j in mono:
        codes[j, :n] = 3
    return (codes[:, 0::4] | (codes[:, 1::4] << 2) | (codes[:, 2::4] << 4) | (codes[:, 3::4] << 6)).astype(np.uint8)


def handles(n, p, seed, mono=()):
    """(label, matrix) of every handle kind; the constructors are cheap at these sizes"""
    rng = np.random.default_rng(seed)
    bed = bed_columns(rng, n, p, 0.03, mono)
    yield "snp", m.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    yield "snp_raw", m.SnpLinAlg(bed, n, center=False, scale=False, impute=True)
    d = rng.standard_normal((n, p))
    for j in mono:
        d[:, j] = 1.0
    yield "f64", m.DenseMatrix(d)
    yield "f32", m.DenseMatrix(d.astype(np.float32))
    yield "dosage", m.DosageMatrix.synthetic(n, p, seed=seed, denom=255, missing_rate=0.02)


def logistic(rng, n, c):
    """covariates with an intercept, a linear predictor, and A = y - mu, w = mu (1 - mu) of a Bernoulli draw"""
    Z = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
    eta = 0.4 * rng.standard_normal(n) - 1.0
    mu = 1.0 / (1.0 + np.exp(-eta))
    y = (rng.random(n) < mu).astype(np.float64)
    return Z, eta, y, y - mu, mu * (1.0 - mu)


def score_cases():
    for n, p in itertools.product((257, 1025), (33, 65)):
        for kind, x in handles(n, p, 100 + n + p):
            full = kind == "snp"              # the 2-bit handle with missing genotypes takes every combination, the others one of each
            for t, c, wt, sl in itertools.product((1, 3), (1, 5), (False, True), (0, 128)):
                if not full and (c == 1 or sl == 128):
                    continue
                rng = np.random.default_rng(1000 * t + 10 * c + wt)
                Z, eta, y, A1, w = logistic(rng, n, c)
                A = A1 if t == 1 else np.column_stack([A1] + [rng.standard_normal(n) for _ in range(t - 1)])
                res = x.score_test(A, w if wt else None, Z, slice_rows=sl, wsum=True)
                show(f"score_test {kind} n={n} p={p} t={t} c={c} w={int(wt)} slice_rows={sl}", feed_assoc, res)


def solver_cases():
    for n in (257, 1025):
        for kind, x in handles(n, 33, 200 + n):
            rng = np.random.default_rng(n)
            Z, eta, y, A, w = logistic(rng, n, 3)
            for cutoff in (0.0, 2.0):
                show(f"score_test_spa {kind} n={n} cutoff={cutoff}", feed_assoc, x.score_test_spa(A, w, Z, eta, cutoff=cutoff))
                for spa in (False, True):
                    show(f"score_test_firth {kind} n={n} cutoff={cutoff} spa={int(spa)}", feed_assoc,
                         x.score_test_firth(A, w, Z, eta, cutoff=cutoff, spa=spa))


def set_cases():
    n, p = 257, 130
    rng = np.random.default_rng(3)
    sizes = (1, 16, 17, 64, 65, 128)
    sets = [np.sort(rng.choice(p, k, replace=False)) for k in sizes]
    sets.append(np.array([3, 7, 11, 40]))                 # column 7 is monomorphic, column 11 gets a zero omega
    omega = [rng.random(s.size) + 0.1 for s in sets]
    omega[-1][2] = 0.0
    Z, eta, y, A, w = logistic(rng, n, 3)
    for kind, x in handles(n, p, 300, mono=(7,)):
        for wt in (False, True):
            show(f"set_test {kind} w={int(wt)}", feed_sets, x.set_test(A, w if wt else None, Z, sets, omega, cov=True))
        show(f"set_test {kind} no sets", feed_sets, x.set_test(A, w, Z, [], cov=True))


def top_layer_cases():
    n, p = 257, 65
    rng = np.random.default_rng(4)
    bed = bed_columns(rng, n, p, 0.03)
    Z, eta, yb, A, w = logistic(rng, n, 3)
    Y = np.column_stack([Z @ [0.3, 0.5, -0.2] + rng.standard_normal(n), rng.standard_normal(n)])
    sets = [np.arange(0, 20), np.arange(15, 40), np.array([50])]
    for label, x in (("scaled", m.SnpLinAlg(bed, n, center=True, scale=True, impute=True)),
                     ("raw", m.SnpLinAlg(bed, n, center=False, scale=False, impute=True))):
        show(f"assoc {label} Normal t=2", feed_assoc, x.assoc(Y, Z))
        show(f"assoc {label} Normal t=1", feed_assoc, x.assoc(Y[:, 0], Z))
        show(f"assoc {label} Bernoulli", feed_assoc, x.assoc(yb, Z, d=m.Bernoulli()))
        show(f"assoc {label} Bernoulli spa firth", feed_assoc, x.assoc(yb, Z, d=m.Bernoulli(), spa=True, firth=True, spa_cutoff=1.0, firth_cutoff=1.0))
        show(f"assoc_sets {label} Normal beta", feed_sets, x.assoc_sets(Y[:, 0], Z, sets, cov=True))
        show(f"assoc_sets {label} Bernoulli beta", feed_sets, x.assoc_sets(yb, Z, sets, d=m.Bernoulli(), max_maf=0.45))


def file_cases():
    """the bytes of what gwas and gwas_sets write for the shipped example: its .bed as a PLINK trio with made-up .fam and .bim"""
    import shutil
    n = 1000
    y = np.loadtxt(os.path.join(FIX, "normal_y_fam6.txt"))
    p = m.read_bed(os.path.join(FIX, "normal.bed"), n).shape[0]
    cov = os.path.join(FIX, "covariates.txt")
    with tempfile.TemporaryDirectory() as tmp:
        for trait, fam6 in (("normal", [repr(float(v)) for v in y]), ("bernoulli", [str(int(v > np.median(y))) for v in y])):
            prefix = os.path.join(tmp, trait)
            shutil.copy(os.path.join(FIX, "normal.bed"), prefix + ".bed")
            with open(prefix + ".fam", "w") as f:
                f.writelines(f"{i + 1} 1 0 0 1 {fam6[i]}\n" for i in range(n))
            with open(prefix + ".bim", "w") as f:
                f.writelines(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n" for j in range(p))
        setfile = os.path.join(tmp, "sets.txt")
        with open(setfile, "w") as f:
            for name, cols in (("geneA", range(9410, 9420)), ("geneB", range(100, 170)), ("geneC", range(5, 6))):
                f.writelines(f"{name} snp{j + 1}\n" for j in cols)
        runs = (("gwas Normal", lambda out: m.gwas(os.path.join(tmp, "normal"), m.Normal, covariates=cov, outfile=out)),
                ("gwas Bernoulli", lambda out: m.gwas(os.path.join(tmp, "bernoulli"), m.Bernoulli, covariates=cov, outfile=out)),
                ("gwas Bernoulli spa", lambda out: m.gwas(os.path.join(tmp, "bernoulli"), m.Bernoulli, covariates=cov, outfile=out, spa=True)),
                ("gwas Bernoulli firth", lambda out: m.gwas(os.path.join(tmp, "bernoulli"), m.Bernoulli, covariates=cov, outfile=out, firth=True,
                                                            spa_cutoff=3.0)),
                ("gwas Bernoulli spa firth", lambda out: m.gwas(os.path.join(tmp, "bernoulli"), m.Bernoulli, covariates=cov, outfile=out,
                                                                spa=True, firth=True)),
                ("gwas_sets Normal", lambda out: m.gwas_sets(os.path.join(tmp, "normal"), m.Normal, setfile, covariates=cov, outfile=out)))
        for label, run in runs:
            out = os.path.join(tmp, "out.txt")
            run(out)
            print(label, hashlib.sha256(open(out, "rb").read()).hexdigest(), flush=True)
        try:                                              # both passes on one selection: unequal cutoffs are refused, and only then
            m.gwas(os.path.join(tmp, "bernoulli"), m.Bernoulli, covariates=cov, outfile="", spa=True, firth=True, spa_cutoff=3.0)
            print("gwas unequal cutoffs accepted", flush=True)
        except m.MendelIHTError as e:
            print("gwas unequal cutoffs refused", hashlib.sha256(f"{type(e).__name__}: {e}".encode()).hexdigest(), flush=True)


if __name__ == "__main__":
    score_cases()
    solver_cases()
    set_cases()
    top_layer_cases()
    file_cases()
