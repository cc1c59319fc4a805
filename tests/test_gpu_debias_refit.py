"""The GLM refit of debias! (csrc/debias.hip) on its own.  A fit reaches it only after five IHT steps, with supports of at most 15
columns in every other test, and is then judged through a whole trajectory; here the measurement build's mih_probe_debias_glm calls
debias_glm_device directly and hands back what its FIRST solve consumed -- the reduced Gram with the right-hand side in its last
column, the working weights and the working response -- and this process holds them against references that owe nothing to the
kernels:

  (a) panel and Gram, exact: Normal / identity (W = 1, target = y, no libm).  The panel is rebuilt on the host from the PLINK codes
      and the handle's own mu and sinv (one subtraction, one multiplication), from the casts of a dense matrix, from dosage_x; every
      entry of the upper triangle of the Gram is compared with the exact rational sum, within gamma * sum_i |P_ia w_i P_ib|,
      gamma = (ceil(n / 64) + 64 + 2) 2^-53 counted from k_db_gram / k_db_gram_reduce (gpu_helpers.debias_gamma), nothing measured.
      k on both sides of the 16-column tile (m = k + 1 = 16: one full tile; 17: the target alone in the second; 33, 34: three tiles
      and the pair (0, 2)), n on both sides of the 64 row slices and of the 64-row chunk (n = 17: 47 empty slices; 4097: per = 65, a
      second chunk of one row; 4161: per = 66), n no multiple of 16, supports with column 0, column p - 1 in a ragged 32-column
      group and adjacent columns, the four uses of (center, scale, impute) with 2 % missing, dense f64 / f32 and a DosageMatrix.
  (b) weighted Gram: for every family and link, the same comparison with the device's OWN w0 and t0 -- the Gram kernel apart from libm.
  (c) closed forms: w0 and t0 entry by entry against GLM.jl's formulas in mpmath at 50 digits; the device is allowed 4 x the worst
      relative error of the same formulas in numpy float64 on the host plus one ulp.
  (d) the refit: beta against oracle.debias_glm at rtol 1e-9 for 13 (family, link) x 3 shapes (the oracle reproduces every case under
      other row orders to 1e-12 max|beta|: tests/test_debias_refit_cpu.py); two calls on the same input agree bit for bit.
  (e) errors: ProbitLink, an all-zero support column, n < k (each raised by the oracle too), bad arguments; a good call follows each.

(c) as measured on an MI355X: the worst error over the 257 responses, in ulps of the exact value, of the device and of the same
formulas in numpy float64 on the host (the yardstick).  Most of it is the condition of the form, not the libm: the rounding of
eta0 moves exp(eta0), and y - mu cancels (Poisson / log: y - exp(log(y + 0.1))), alike on both sides.  No form misses.

    family / link        w0 device  w0 host   t0 device  t0 host
    normal / identity       0.00      0.00       0.00      0.00
    normal / log            2.93      2.98       0.79      0.77
    bernoulli / logit       0.00      0.00       0.04      0.04
    bernoulli / cloglog     0.44      0.44       0.28      0.28
    bernoulli / cauchit     2.19      2.19       1.14      1.14
    poisson / log           1.60      1.60       3.35      3.35
    poisson / sqrt          0.00      0.00       0.63      0.63
    negbin / log, r = 4     1.33      1.57       0.67      0.67
    negbin / log, r = 0.5   1.38      1.38       0.67      0.67
    gamma / log             0.00      0.00       0.77      0.73
    gamma / inverse         4.18      4.18       0.74      0.74
    invgauss / log          2.13      2.52       0.71      0.79
    invgauss / invsquare    4.38      4.38       2.69      2.69
"""
import numpy as np
import pytest

from gpu_helpers import (DEBIAS_DIST, DEBIAS_FLAGS, DEBIAS_FORMS, DEBIAS_KS, DEBIAS_LINK, DEBIAS_NS, DEBIAS_P, DEBIAS_SHAPES, _pack, _run_probe_snippet,
                         debias_form_errors, debias_forms_f64, debias_forms_mp, debias_gram_jobs, debias_gram_misses, debias_gram_problem,
                         debias_oracle_beta, debias_panel_dosage, debias_panel_snp, debias_refit_cases, debias_refit_problem)

pytestmark = pytest.mark.gpu

# jobs from <out>.in.npz: job j = one matrix and one (or, twice = 1, two) calls of mih_probe_debias_glm; then the argument errors
_SNIPPET = r"""
import ctypes as C
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import mendeliht_amd as m
from mendeliht_amd import api
assert m.using_probes()
L = api.lib()
inp = np.load(sys.argv[2] + ".in.npz")
out = {}

def err():
    buf = C.create_string_buffer(512)
    L.mih_last_error(buf, 512)
    return buf.value.decode(errors="replace")

def call(x, idx, y, dist, link, nbr, tag):
    k, n = idx.size, x.n
    beta, gram, w0, t0 = np.full(k, np.nan), np.full((k + 1) * (k + 1), np.nan), np.full(n, np.nan), np.full(n, np.nan)
    it = C.c_int32(-1)
    rc = L.mih_probe_debias_glm(x._h, api._p(idx), k, api._p(y), dist, link, nbr, api._p(beta), api._p(gram), api._p(w0), api._p(t0), C.byref(it))
    out[tag + "rc"], out[tag + "msg"], out[tag + "it"] = np.int64(rc), np.array(err() if rc else ""), np.int64(it.value)
    out[tag + "beta"], out[tag + "gram"], out[tag + "w0"], out[tag + "t0"] = beta, gram, w0, t0

x = None
for j in range(int(inp["njobs"])):
    kind, n, c, s, i, dist, link, twice, den = (int(v) for v in inp[f"j{j}_meta"])
    data = inp[f"j{j}_data"]
    if kind == 0:
        x = m.SnpLinAlg(data, n, center=c, scale=s, impute=i)
        out[f"j{j}_mu"], out[f"j{j}_sinv"] = x.mu_sigma()
    elif kind == 3:
        x = m.DosageMatrix(data, den)
    else:
        x = m.DenseMatrix(data)
        assert x.dtype == (np.float32 if kind == 2 else np.float64)
    idx = np.ascontiguousarray(inp[f"j{j}_idx"], dtype=np.int64)
    y = np.ascontiguousarray(inp[f"j{j}_y"], dtype=np.float64)
    call(x, idx, y, dist, link, float(inp[f"j{j}_nbr"]), f"j{j}_")
    if twice:
        call(x, idx, y, dist, link, float(inp[f"j{j}_nbr"]), f"j{j}_again_")
if int(inp["argchecks"]):
    # bad arguments on the last matrix (a good job), then the good call once more
    k, n = idx.size, x.n
    beta = np.zeros(k)
    f = lambda h, ix, kk, yy, b, d=0, l=0: int(L.mih_probe_debias_glm(h, ix, kk, yy, d, l, 1.0, b, None, None, None, None))
    far, neg = idx.copy(), idx.copy()
    far[-1] = x.p; neg[0] = -1
    out["arg_rc"] = np.array([f(None, api._p(idx), k, api._p(y), api._p(beta)), f(x._h, None, k, api._p(y), api._p(beta)),
                              f(x._h, api._p(idx), k, None, api._p(beta)), f(x._h, api._p(idx), k, api._p(y), None),
                              f(x._h, api._p(idx), 0, api._p(y), api._p(beta)), f(x._h, api._p(idx), -3, api._p(y), api._p(beta)),
                              f(x._h, api._p(far), k, api._p(y), api._p(beta)), f(x._h, api._p(neg), k, api._p(y), api._p(beta)),
                              f(x._h, api._p(idx), k, api._p(y), api._p(beta), 6, 0), f(x._h, api._p(idx), k, api._p(y), api._p(beta), 0, 9)], dtype=np.int64)
    out["arg_good_rc"] = np.int64(f(x._h, api._p(idx), k, api._p(y), api._p(beta)))       # every output but beta may be null
    out["arg_good_beta"] = beta
np.savez(sys.argv[2], **out)
"""

_KIND = {"snp": 0, "f64": 1, "f32": 2, "dosage": 3}


class _Job:
    def __init__(self, kind, data, n, idx, y, flags=None, dist="normal", link="identity", nb_r=1.0, twice=False, den=0, tag=""):
        self.kind, self.data, self.n, self.idx, self.y, self.flags = kind, data, n, np.asarray(idx, dtype=np.int64), y, flags
        self.dist, self.link, self.nb_r, self.twice, self.den, self.tag = dist, link, nb_r, twice, den, tag
        self.k = self.idx.size

    def store(self, inp, j):
        c, s, i = self.flags or (0, 0, 0)
        inp[f"j{j}_meta"] = np.array([_KIND[self.kind], self.n, c, s, i, DEBIAS_DIST[self.dist], DEBIAS_LINK[self.link], int(self.twice), self.den], dtype=np.int64)
        inp[f"j{j}_data"] = _pack(self.data) if self.kind == "snp" else self.data
        inp[f"j{j}_idx"], inp[f"j{j}_y"], inp[f"j{j}_nbr"] = self.idx, self.y, np.float64(self.nb_r)


class _Out:
    """What one call gave back."""
    def __init__(self, got, tag):
        self.rc, self.msg, self.iters = int(got[tag + "rc"]), str(got[tag + "msg"]), int(got[tag + "it"])
        self.beta, self.gram, self.w0, self.t0 = got[tag + "beta"], got[tag + "gram"], got[tag + "w0"], got[tag + "t0"]


def _run(jobs, out_file, argchecks=False):
    inp = {"njobs": np.int64(len(jobs)), "argchecks": np.int64(argchecks)}
    for j, jb in enumerate(jobs):
        jb.store(inp, j)
    np.savez(str(out_file) + ".in.npz", **inp)
    return _run_probe_snippet(_SNIPPET, out_file, timeout=600)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_NOT_PD = "not positive definite"


# ---------------------------------------------------------------- (a), (e): one process ----------------------------------------------------------------
def _gram_job(spec):
    kind, n, k, flags, seed = spec
    data, idx, y = debias_gram_problem(kind, n, k, flags, seed)
    if kind == "dosage":
        return _Job(kind, data[0], n, idx, y, den=data[1], twice=(seed % 3 == 0), tag=str(spec))
    return _Job(kind, data, n, idx, y, flags=flags, twice=(seed % 3 == 0), tag=str(spec))


@pytest.fixture(scope="module")
def gram_run(tmp_path_factory):
    """The jobs of (a) in the order of debias_gram_jobs, each n < k job (an error) followed by a good one by that order; then the error
    paths of (e), each followed by a good call; then the argument errors."""
    specs = debias_gram_jobs()
    jobs = [_gram_job(s) for s in specs]
    rng = np.random.default_rng(20285)
    n, p = 300, 40
    X = np.asfortranarray(rng.standard_normal((n, p)))
    X[:, 7] = 0.0
    y = rng.standard_normal(n)
    yb = (rng.random(n) < 0.5).astype(np.float64)
    good = np.array([0, 3, 39, 31, 32, 12], dtype=np.int64)
    extra = [_Job("f64", X, n, good, yb, dist="bernoulli", link="probit", tag="probit"),
             _Job("f64", X, n, good, yb, dist="bernoulli", link="logit", tag="after probit"),
             _Job("f64", X, n, np.array([0, 7, 39]), y, tag="zero column"),
             _Job("f64", X, n, good, y, tag="after zero column")]
    got = _run(jobs + extra, tmp_path_factory.mktemp("debias") / "gram.npz", argchecks=True)
    return specs, jobs, extra, got


def _panel_of(job, got, j):
    if job.kind == "snp":
        return debias_panel_snp(job.data, job.idx, got[f"j{j}_mu"], got[f"j{j}_sinv"], *job.flags)
    if job.kind == "dosage":
        return debias_panel_dosage(job.data, job.den, job.idx)
    return np.asarray(job.data)[:, job.idx].astype(np.float64)


@pytest.mark.parametrize("j", range(len(debias_gram_jobs())), ids=lambda j: "{}-n{}-k{}-{}-{}".format(*debias_gram_jobs()[j]).replace(" ", ""))
def test_panel_and_gram_exact(gram_run, j):
    specs, jobs, _, got = gram_run
    job, out = jobs[j], _Out(got, f"j{j}_")
    n, k = job.n, job.k
    if n < k:
        assert out.rc == 2 and _NOT_PD in out.msg, (out.rc, out.msg)
        assert jobs[j + 1].n >= 63 and _Out(got, f"j{j + 1}_").rc == 0           # a good call follows in the same process
    elif n >= 63:
        assert out.rc == 0, out.msg
    else:
        assert out.rc == 0 or (out.rc == 2 and _NOT_PD in out.msg), (out.rc, out.msg)      # (17 centred rows have rank 16)
    # the first solve's inputs: W = 1 and target = y, bit for bit (mueta = 1, var = 1, mu = eta = y: y + (y - y) / 1)
    assert np.array_equal(_bits(out.t0), _bits(job.y)) and np.array_equal(_bits(out.w0), _bits(np.ones(n)))
    P = np.column_stack([_panel_of(job, got, j), job.y])
    bad, worst = debias_gram_misses(out.gram, P, np.ones(n), n)
    print(f"{job.tag}: worst Gram error {worst:.3g} of the bound")
    assert not bad, (job.tag, len(bad), bad[:4])
    if out.rc == 0 and n >= 1000:
        # Normal / identity converges to the least-squares solution; cond(P'P) is at most e^8 = 3000 here (the dense columns'
        # scales span e^-2 .. e^2), so the normal equations carry about cond x gamma = 3000 x 1.5e-14 < 1e-10: 1e-9 is the refit's
        # parity figure
        ls = np.linalg.lstsq(P[:, :k], job.y, rcond=None)[0]
        assert np.max(np.abs(out.beta - ls)) <= 1e-9 * np.max(np.abs(ls)), job.tag
    if job.twice:
        again = _Out(got, f"j{j}_again_")
        assert again.rc == out.rc
        G, G2 = out.gram.reshape(k + 1, k + 1, order="F"), again.gram.reshape(k + 1, k + 1, order="F")
        up = np.triu_indices(k + 1)
        assert np.array_equal(_bits(G[up]), _bits(G2[up])) and (out.rc != 0 or np.array_equal(_bits(out.beta), _bits(again.beta)))


def test_gram_jobs_cover_every_tile_slice_and_flag_edge():
    specs = debias_gram_jobs()
    snp = [(n, k) for kind, n, k, _, _ in specs if kind == "snp"]
    assert {k for n, k in snp if n == 4097} == set(DEBIAS_KS) and {n for n, k in snp if k == 17} == set(DEBIAS_NS)
    assert {f for kind, _, _, f, _ in specs if kind == "snp"} == set(DEBIAS_FLAGS) and {kind for kind, *_ in specs} == {"snp", "f64", "f32", "dosage"}
    assert any(n < k for n, k in snp) and DEBIAS_P % 32 != 0


def test_error_paths_match_the_oracle_and_leave_the_library_usable(gram_run, oracle):
    specs, jobs, extra, got = gram_run
    base = len(jobs)
    probit, after_probit, zero, after_zero = (_Out(got, f"j{base + t}_") for t in range(4))
    assert probit.rc == 2 and "ProbitLink" in probit.msg
    assert zero.rc == 2 and _NOT_PD in zero.msg
    assert after_probit.rc == 0 and after_zero.rc == 0 and np.isfinite(after_probit.beta).all() and np.isfinite(after_zero.beta).all()
    ox = oracle.Mat.from_dense(extra[0].data)
    for jb, (dist, link) in ((extra[0], ("bernoulli", "probit")), (extra[2], ("normal", "identity"))):
        mask = np.zeros(ox.p, np.uint8); mask[jb.idx] = 1
        with pytest.raises(RuntimeError):
            oracle.debias_glm(ox, mask, jb.y, dist, link)
    for jb, out in ((extra[1], after_probit), (extra[3], after_zero)):          # the good calls are right, too
        mask = np.zeros(ox.p, np.uint8); mask[jb.idx] = 1
        want = oracle.debias_glm(ox, mask, jb.y, jb.dist, jb.link)[jb.idx]
        np.testing.assert_allclose(out.beta, want, rtol=1e-9)
    below = [j for j, jb in enumerate(jobs) if jb.n < jb.k]
    assert len(below) >= 2
    for j in below:
        with pytest.raises(RuntimeError):
            debias_oracle_beta(oracle, jobs[j].data, jobs[j].flags, jobs[j].idx, jobs[j].y, "normal", "identity", 1.0)
    # null matrix / idx / y / beta, k = 0, k < 0: MIH_BAD_ARG; an index = p or < 0: MIH_BAD_DIM; a distribution or link code out of range
    assert got["arg_rc"].tolist() == [2, 2, 2, 2, 2, 2, 1, 1, 2, 2]
    assert int(got["arg_good_rc"]) == 0 and np.array_equal(_bits(got["arg_good_beta"]), _bits(after_zero.beta))


# ---------------------------------------------------------------- (b), (c), (d): one process ----------------------------------------------------------------
@pytest.fixture(scope="module")
def refit_run(tmp_path_factory):
    cases = debias_refit_cases()
    jobs = []
    for dist, link, nb_r, n, k, attempt in cases:
        code, csi, idx, y = debias_refit_problem(dist, link, nb_r, n, k, attempt)
        jobs.append(_Job("snp", code, n, idx, y, flags=csi, dist=dist, link=link, nb_r=nb_r, twice=(n == 257), tag=f"{dist}/{link}/r{nb_r} n{n} k{k}"))
    got = _run(jobs, tmp_path_factory.mktemp("debias") / "refit.npz")
    return cases, jobs, got


_CASE_IDS = ["{}-{}-r{}-n{}-k{}".format(*c[:5]) for c in debias_refit_cases()]


@pytest.mark.parametrize("j", range(len(_CASE_IDS)), ids=lambda j: _CASE_IDS[j])
def test_refit_against_the_oracle_and_weighted_gram_exact(refit_run, oracle, j):
    """(d) and (b) for one case."""
    cases, jobs, got = refit_run
    job, out = jobs[j], _Out(got, f"j{j}_")
    n, k = job.n, job.k
    assert out.rc == 0, (job.tag, out.msg)
    assert np.isfinite(out.w0).all() and np.isfinite(out.t0).all() and (out.w0 > 0.0).all()
    P = np.column_stack([debias_panel_snp(job.data, job.idx, got[f"j{j}_mu"], got[f"j{j}_sinv"], *job.flags), out.t0])
    bad, worst = debias_gram_misses(out.gram, P, out.w0, n)                    # (b): the device's own weights and target
    print(f"{job.tag}: worst Gram error {worst:.3g} of the bound, {out.iters} IRLS iterations")
    assert not bad, (job.tag, len(bad), bad[:4])
    want = debias_oracle_beta(oracle, job.data, job.flags, job.idx, job.y, job.dist, job.link, job.nb_r)
    np.testing.assert_allclose(out.beta, want, rtol=1e-9, atol=0, err_msg=job.tag)      # (d)
    if job.twice:
        again = _Out(got, f"j{j}_again_")
        up = np.triu_indices(k + 1)
        assert again.rc == 0 and again.iters == out.iters and np.array_equal(_bits(out.beta), _bits(again.beta))
        assert np.array_equal(_bits(out.gram.reshape(k + 1, k + 1, order="F")[up]), _bits(again.gram.reshape(k + 1, k + 1, order="F")[up]))
        assert np.array_equal(_bits(out.w0), _bits(again.w0)) and np.array_equal(_bits(out.t0), _bits(again.t0))


def test_refit_cases_cover_every_family_link_and_shape():
    cases = debias_refit_cases()
    assert {(d, l, r) for d, l, r, *_ in cases} == set(DEBIAS_FORMS) and len(DEBIAS_FORMS) == 13
    assert {(n, k) for _, _, _, n, k, _ in cases} == set(DEBIAS_SHAPES) and len(cases) == 39


@pytest.mark.parametrize("f", range(len(DEBIAS_FORMS)), ids=lambda f: "{}-{}-r{}".format(*DEBIAS_FORMS[f]))
def test_closed_forms_entry_by_entry(refit_run, f):
    """(c): w0 and t0 of the n = 257 case against mpmath.  The yardstick is the same formulas in numpy float64 on the host: the device
    gets 4 x the host's worst relative error plus one ulp of the value, per (family, link), for the weight and the response apart."""
    cases, jobs, got = refit_run
    dist, link, nb_r = DEBIAS_FORMS[f]
    (j,) = [t for t, c in enumerate(cases) if c[:4] == (dist, link, nb_r, 257)]
    job, out = jobs[j], _Out(got, f"j{j}_")
    if dist in ("poisson", "negbin"):
        assert (job.y == 0.0).sum() >= 3                                       # the y + 0.1 and 1 / 6 starts
    W, T = debias_forms_mp(dist, link, nb_r, job.y)
    hw, ht = debias_forms_f64(dist, link, nb_r, job.y)
    report = []
    for name, dev, host, exact in (("w0", out.w0, hw, W), ("t0", out.t0, ht, T)):
        drel, dulps, ulp = debias_form_errors(dev, exact)
        hrel, hulps, _ = debias_form_errors(host, exact)
        ex = np.array([abs(float(v)) for v in exact])
        report.append(f"{name} device {dulps.max():.2f} host {hulps.max():.2f}")
        allowed = 4.0 * hrel.max() * ex + ulp
        err = drel * ex
        worst = int(np.argmax(err - allowed))
        assert np.all(err <= allowed), (dist, link, nb_r, name, f"row {worst}: y {job.y[worst]!r} device {dev[worst]!r} host {host[worst]!r} "
                                        f"exact {float(exact[worst])!r}; device {dulps.max():.2f} ulps, host {hulps.max():.2f} ulps")
    print(f"{dist}/{link}/r{nb_r}: ulps of the exact value, " + ", ".join(report))
