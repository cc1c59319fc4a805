"""The p univariate regressions of initialize_beta! (csrc/iht_var.hip: init_beta_regress_device and its kernels k_ib_rhs, k_ib_mask,
k_ib_counts, k_ib_solve, k_ib_dense_sxx, k_ib_dosage_sxx, k_ib_sum) on their own.  Every fit with init_beta calls them, and a fit
keeps the k largest of the p slopes and one mean of the intercepts, at rtol 1e-5: a wrong count in a few columns or a wrong
correction for missing rows changes nothing such a fit asserts.  Here the measurement build's mih_probe_init_beta calls
init_beta_regress_device directly and hands back its intermediates, and this process holds them against tests/init_beta_spec.py
(exact rationals; its docstring has the statement and the derivation of the solve's bound; tests/test_init_beta_spec_cpu.py
asserts, for every case, the conditions relied on here):

  (a) counts: cnt[2j + k] = the training rows of column j with dosage k + 1, exactly.
  (b) X'R: S row 0 against the exact sum_T x, row 1 + t against the exact sum_T x y_t, within the bound the association tests hold
      this pass to (assoc_spec._xtv_bound_snp with R = [w | w o Y]; _xtv_bound_dense for dense and dosage handles).
  (c) dense / dosage sum of squares against the exact sum_T x^2 within init_beta_spec.sxx_gamma(n) sum_T x^2.
  (d) the solve: beta and icpt against the statement in mpmath fed with the device's OWN S (and the exact Sxx of the integer counts,
      or the device's own sxx), within init_beta_spec.solve_bound; exactly +-2 where the reference slope is beyond; the all-zero
      column exactly (0, Sy); a column constant over the training rows (d = 0 exactly, the branch undetermined) finite and clamped.
  (e) icpt_sum[t] against the exact sum of the device's own plane t within init_beta_spec.icpt_sum_gamma(p) sum |icpt|.
  (f) bits: a second call; plane t of an m-trait call against the one-trait call on Y[:, t]; the handle's X'v before and after.
  (g) refusals: every argument error is MIH_BAD_ARG, writes nothing, and a good call follows it.
  (h) whole fits on the product library across the count-block edge (n = 8320: two blocks of k_ib_counts), against the oracle.

Shapes (init_beta_spec.snp_cases / dense_cases).  2-bit: n = 17 (a dword and a row), 128 (a tile), 129, 8192 (exactly the 64 tiles
of one block of k_ib_counts), 8193, 8320 (a row / a tile into a second block), 16500 (three blocks, a ragged tail); p = 1, 32, 33,
65 (a ragged / full last column group, 1 to 3 groups); all n at p = 33, all p at n = 129 and 8320, the four corners.  Masks: all,
random80, one_out (the last row), blocks (n > 8192: the whole first count block held out -- the `&& red[kk][mm]` branch --, every
other 16-row word of the next tile, one whole tile further on).  The four flag sets and 0 / 3 % missing cycle over them.  Planted
where p >= 32: (a) an all-zero column, (b) a column whose missing rows are all held out and one whose missing rows are all
training rows (nm of k_ib_solve against the column's whole missing list), (c) a column non-zero in held-out rows only (its counts
must be 0), (d) a column with slope 3 (the clamp).  m = 2, 17, 32 at (129, 33) and (8320, 65): 33 right-hand sides take more
than one fused pass.  Under `blocks` n = 8193 leaves ONE training row: every column is constant over it, so that case checks
(a), (b), (e), (f) and only finiteness and the clamp of (d).  Dense f64 / f32 and dosage: n = 255, 256, 257, 1000 around the
256-row stride of the sum-of-squares kernels, p = 5, m = 1 and 3, masks all and random80.

Measured on an MI355X: the largest err / bound of each check over the cases of a kind (a record; no tolerance depends on it).
Every count, the all-zero columns, the clamped slopes (one per case with planted columns, more at n = 17) and all bits were exact.

    cases                              count       X'R       sxx      beta      icpt  icpt_sum
    2-bit, m = 1, all                     17     0.023         -      0.28      0.39       0.1
    2-bit, m = 1, random80                17     0.018         -      0.34      0.56       0.1
    2-bit, m = 1, one_out                 17     0.016         -      0.61      0.61      0.12
    2-bit, m = 1, blocks                   8     0.011         -      0.25      0.32     0.059
    2-bit, m = 2 / 17 / 32, random80       6      0.02         -      0.55      0.59      0.15
    2-bit, m = 2 / 17 / 32, blocks         3     0.013         -      0.25       0.2     0.087
    dense f64                             16     0.005      0.15      0.37      0.54     0.088
    dense f32                             16    0.0054       0.2      0.54      0.55     0.091
    dosage                                16    0.0094      0.23      0.25      0.47     0.067
"""
from fractions import Fraction

import numpy as np
import pytest

import assoc_spec as A
import gpu_helpers as H
import init_beta_spec as S
from conftest import hash_folds, make_bed
from gpu_helpers import _mv_problem, _run_probe_snippet, _sim
from test_gpu_hardcall_pack import bed_of

pytestmark = pytest.mark.gpu

BAD_ARG = 2
_KIND = {"snp": 0, "f64": 1, "f32": 2, "dosage": 3}
CASES = S.snp_cases() + S.dense_cases()

# jobs from <out>.in.npz: job j = one matrix, the call, the call again, the m one-trait calls where m > 1, X'v before and after; then
# the argument errors on a small matrix of their own
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
FILL = 7.5

def call(x, w, Yt, mm, tag=None, h="x", nulls=()):
    p = x.p
    a = dict(S=np.full((1 + max(mm, 1), p), FILL), cnt=np.full(2 * p, 77, dtype=np.int32), sxx=np.full(p, FILL),
             beta=np.full((max(mm, 1), p), FILL), icpt=np.full((max(mm, 1), p), FILL), sum=np.full(max(mm, 1), FILL))
    ptr = {k: (None if k in nulls else api._p(v)) for k, v in a.items()}
    rc = L.mih_probe_init_beta(None if h is None else x._h, None if w is None else api._p(w), None if Yt is None else api._p(Yt), mm,
                               ptr["S"], ptr["cnt"], ptr["sxx"], ptr["beta"], ptr["icpt"], ptr["sum"])
    if tag is not None:
        out[tag + "rc"] = np.int64(rc)
        for k, v in a.items():
            out[tag + k] = v
    return int(rc), a

def untouched(a):
    return all((v == (77 if k == "cnt" else FILL)).all() for k, v in a.items())

def same(a, b, keys):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)

def make(kind, data, n, c, s, i, den):
    if kind == 0:
        return m.SnpLinAlg(data, n, center=bool(c), scale=bool(s), impute=bool(i))
    if kind == 3:
        return m.DosageMatrix(data, den)
    x = m.DenseMatrix(data)
    assert x.dtype == (np.float32 if kind == 2 else np.float64)
    return x

for j in range(int(inp["njobs"])):
    kind, n, mm, c, s, i, den = (int(v) for v in inp[f"j{j}_meta"])
    x = make(kind, inp[f"j{j}_data"], n, c, s, i, den)
    if kind in (0, 3):
        out[f"j{j}_mu"], out[f"j{j}_sinv"] = x.mu_sigma()
    w = np.ascontiguousarray(inp[f"j{j}_w"], dtype=np.float64)
    Yt = np.ascontiguousarray(inp[f"j{j}_Yt"], dtype=np.float64)          # m x n: plane t = trait t
    v = np.ascontiguousarray(inp[f"j{j}_v"], dtype=np.float64)
    out[f"j{j}_xtv0"] = x.xtv(v)
    call(x, w, Yt, mm, f"j{j}_")
    call(x, w, Yt, mm, f"j{j}_again_")
    if mm > 1:
        singles = [call(x, w, np.ascontiguousarray(Yt[t]), 1)[1] for t in range(mm)]
        for k in ("S", "beta", "icpt", "sum"):
            out[f"j{j}_single_{k}"] = np.stack([a[k] for a in singles])
    out[f"j{j}_xtv1"] = x.xtv(v)

if int(inp["argchecks"]):
    n, mm = int(inp["arg_n"]), 2
    x = make(0, inp["arg_data"], n, 1, 1, 1, 0)
    w, Yt = np.ascontiguousarray(inp["arg_w"]), np.ascontiguousarray(inp["arg_Yt"])
    rc0, good = call(x, w, Yt, mm)
    half, two, nanw, none = w.copy(), w.copy(), w.copy(), np.zeros(n)
    half[3], two[n - 1], nanw[0] = 0.5, 2.0, np.nan
    ynan, yinf = Yt.copy(), Yt.copy()
    ynan[1, n - 1], yinf[0, 0] = np.nan, -np.inf
    # (a non-finite Y is refused in a held-out row too: row n - 1 is held out)
    bad = [dict(h=None), dict(w=None), dict(Yt=None), dict(nulls=("beta",)), dict(mm=0), dict(mm=-1), dict(mm=33), dict(w=half), dict(w=two),
           dict(w=nanw), dict(w=none), dict(Yt=ynan), dict(Yt=yinf)]
    rcs, clean, after = [], [], []
    for kw in bad:
        args = dict(w=w, Yt=Yt, mm=mm)
        args.update(kw)
        rc, a = call(x, args["w"], args["Yt"], args["mm"], h=args.get("h", "x"), nulls=args.get("nulls", ()))
        rcs.append(rc)
        clean.append(untouched(a))
        rc, a = call(x, w, Yt, mm)                           # a good call follows each
        after.append(rc == 0 and same(a, good, ("S", "cnt", "beta", "icpt", "sum")))
    out["arg_rc0"], out["arg_rcs"], out["arg_clean"], out["arg_after"] = np.int64(rc0), np.array(rcs), np.array(clean), np.array(after)
    rc, a = call(x, w, Yt, mm, nulls=("S", "cnt", "sxx", "icpt", "sum"))          # every output but beta may be null
    out["arg_only_beta"] = np.array([rc == 0, a["beta"].tobytes() == good["beta"].tobytes(), untouched({k: a[k] for k in ("S", "cnt", "sxx", "icpt", "sum")})])
    for k in ("beta", "icpt"):
        out["arg_good_" + k] = good[k]
np.savez(sys.argv[2], **out)
"""


def _matrix_data(inp):
    kind = inp.case.kind
    if kind == "snp":
        return bed_of(inp.codes)
    if kind == "dosage":
        return np.asfortranarray(inp.num)
    return np.asfortranarray(inp.X.astype(np.float32) if kind == "f32" else inp.X)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """All cases and the argument errors in ONE child process on the measurement build."""
    store = {"njobs": np.int64(len(CASES)), "argchecks": np.int64(1)}
    for j, case in enumerate(CASES):
        inp = S.inputs(case)
        c, s, i = case.flags or (0, 0, 0)
        store[f"j{j}_meta"] = np.array([_KIND[case.kind], case.n, case.m, c, s, i, getattr(inp, "den", 0)], dtype=np.int64)
        store[f"j{j}_data"], store[f"j{j}_w"], store[f"j{j}_Yt"] = _matrix_data(inp), inp.w, np.ascontiguousarray(inp.Y.T)
        store[f"j{j}_v"] = np.random.default_rng(case.seed).standard_normal(case.n)
    arg = S.inputs(next(c for c in S.snp_cases() if (c.n, c.p, c.m, c.mask) == (129, 33, 2, "random80")))
    w = arg.w.copy()
    w[-1] = 0.0
    store["arg_n"], store["arg_data"], store["arg_w"], store["arg_Yt"] = np.int64(arg.case.n), bed_of(arg.codes), w, np.ascontiguousarray(arg.Y.T)
    out_file = tmp_path_factory.mktemp("init_beta") / "out.npz"
    np.savez(str(out_file) + ".in.npz", **store)
    return _run_probe_snippet(_SNIPPET, out_file, timeout=300)


def _ratio(err, tol):
    """max err / bound over arrays of Fractions / floats (0 where both are 0); asserts nothing."""
    worst = 0.0
    for e, t in zip(err, tol):
        if e != 0:
            worst = max(worst, float(e) / float(t) if t > 0 else float("inf"))
    return worst


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("j", range(len(CASES)), ids=lambda j: CASES[j].id)
def test_regressions_against_the_statement(run, j):
    case, got = CASES[j], run
    inp = S.inputs(case)
    n, p, m, snp = case.n, case.p, case.m, case.kind == "snp"
    tag = f"j{j}_"
    assert int(got[tag + "rc"]) == 0 and int(got[tag + "again_rc"]) == 0
    Sd, cnt, sxx, beta, icpt, isum = (got[tag + k] for k in ("S", "cnt", "sxx", "beta", "icpt", "sum"))
    T = inp.w != 0
    R = np.concatenate([inp.w[:, None], inp.w[:, None] * inp.Y], axis=1)
    # the reference side from the handle's own statistics (they are host_stats' / dosage_host_stats' bit for bit: then the exact
    # evaluation the CPU test checked is reused as it is)
    if snp:
        stats = (got[tag + "mu"], got[tag + "sinv"])
        host = A.host_stats(inp.codes)
        ex = inp.exact if _bits(stats[0]) == _bits(host[0]) and _bits(stats[1]) == _bits(host[1]) else S.exact_of(inp, stats=stats)
        # (a)
        want = S.train_counts(inp.codes, inp.w)
        assert np.array_equal(cnt.reshape(p, 2), want[1:3].T), (case.id, np.argwhere(cnt.reshape(p, 2) != want[1:3].T)[:4].tolist())
        assert (sxx == 7.5).all()                                       # ignored for a 2-bit handle
        if "c" in inp.planted:
            assert (cnt.reshape(p, 2)[inp.planted["c"]] == 0).all() and (inp.codes[:, inp.planted["c"]] > 0).any()
        tolS = A._xtv_bound_snp(inp.codes, case.flags, stats, R)       # p x (1 + m)
    else:
        X = H.standardized(inp.num, inp.den, got[tag + "mu"], got[tag + "sinv"]) if case.kind == "dosage" else inp.X
        ex = inp.exact if _bits(X) == _bits(inp.X) else S.exact_of(inp, X=X)
        assert (cnt == 77).all()                                        # ignored for a dense / dosage handle
        tolS = A._xtv_bound_dense(X, R)
    # (b)
    wantS = [ex.Sx] + ex.Sxy
    errS = [[abs(Fraction(float(Sd[r, c])) - wantS[r][c]) for c in range(p)] for r in range(1 + m)]
    assert np.isfinite(Sd).all()
    bad = [(r, c, float(errS[r][c]), float(tolS[c, r])) for r in range(1 + m) for c in range(p) if not errS[r][c] <= tolS[c, r]]
    assert not bad, (case.id, "X'R", bad[:4])
    r_xtr = _ratio([e for row in errS for e in row], [tolS[c, r] for r in range(1 + m) for c in range(p)])
    # (c)
    r_sxx = 0.0
    if not snp:
        g = S.sxx_gamma(n)
        errq = [abs(Fraction(float(sxx[c])) - ex.Sxx[c]) for c in range(p)]
        assert all(e <= Fraction(g) * q for e, q in zip(errq, ex.Sxx)), (case.id, "sxx", [float(e / q) / g for e, q in zip(errq, ex.Sxx)])
        r_sxx = _ratio(errq, [g * float(q) for q in ex.Sxx])
    # (d)
    free = set(S.undetermined(inp))
    r_b1 = r_b0 = 0.0
    clamped = 0
    assert np.isfinite(beta).all() and np.isfinite(icpt).all() and (np.abs(beta) <= 2.0).all()
    for t in range(m):
        Sy = ex.Sy[t]
        assert float(Sy) == float(np.sum(inp.Y[T, t])) and Fraction(float(Sy)) == Sy           # (exact in any order)
        for c in range(p):
            if c in free:
                continue
            if inp.planted.get("a") == c:
                assert beta[t, c] == 0.0 and icpt[t, c] == float(Sy), (case.id, "all-zero column", t, beta[t, c], icpt[t, c])
                continue
            q = ex.Sxx[c] if snp else Fraction(float(sxx[c]))
            b0, b1, d = S.solve_mp(ex.N, float(Sd[0, c]), float(Sd[1 + t, c]), q, Sy)
            assert d is not None and d > 0, (case.id, t, c)
            db0, db1 = S.solve_bound(ex.N, Sd[0, c], Sd[1 + t, c], q, Sy, b0, b1, d, S.E_XX_SNP if snp else 0.0)
            if abs(b1) > 2:
                assert beta[t, c] == (2.0 if b1 > 0 else -2.0), (case.id, "clamp", t, c, beta[t, c], float(b1))
                clamped += 1
            else:
                e1 = S.err(beta[t, c], b1)
                assert e1 <= db1, (case.id, "beta", t, c, beta[t, c], float(b1), e1, db1)
                r_b1 = max(r_b1, e1 / db1)
            e0 = S.err(icpt[t, c], b0)
            assert e0 <= db0, (case.id, "icpt", t, c, icpt[t, c], float(b0), e0, db0)
            r_b0 = max(r_b0, e0 / db0)
    if "jstar" in inp.planted and not free >= {inp.planted["jstar"]}:
        assert beta[0, inp.planted["jstar"]] == 2.0 and clamped >= 1
    # (e)
    gs = S.icpt_sum_gamma(p)
    errs = [abs(Fraction(float(isum[t])) - S.fsum_exact(icpt[t])) for t in range(m)]
    tols = [gs * float(np.abs(icpt[t]).sum()) for t in range(m)]
    assert all(e <= tl for e, tl in zip(errs, tols)), (case.id, "icpt_sum", [float(e) for e in errs], tols)
    r_sum = _ratio(errs, tols)
    # (f)
    for k in ("S", "cnt", "sxx", "beta", "icpt", "sum"):
        assert _bits(got[tag + k]) == _bits(got[tag + "again_" + k]), (case.id, "second call", k)
    assert _bits(got[tag + "xtv0"]) == _bits(got[tag + "xtv1"]), (case.id, "the handle changed")
    if m > 1:
        s1, b1s, i1, u1 = (got[tag + "single_" + k] for k in ("S", "beta", "icpt", "sum"))
        for t in range(m):
            assert _bits(s1[t, 0]) == _bits(Sd[0]) and _bits(s1[t, 1]) == _bits(Sd[1 + t]), (case.id, "plane against one-trait call: S", t)
            assert _bits(b1s[t, 0]) == _bits(beta[t]) and _bits(i1[t, 0]) == _bits(icpt[t]) and _bits(u1[t]) == _bits(isum[t:t + 1]), (case.id, "plane", t)
    print(f"init_beta {case.id}: err / bound  X'R {r_xtr:.3g}  sxx {r_sxx:.3g}  beta {r_b1:.3g}  icpt {r_b0:.3g}  icpt_sum {r_sum:.3g}  clamped {clamped}")


def test_refusals_write_nothing_and_a_good_call_follows(run):
    """null h / w / Y / beta; m = 0, -1, 33; a w entry 0.5, 2, NaN; no training row; NaN and -inf in Y: MIH_BAD_ARG before any launch."""
    got = run
    assert int(got["arg_rc0"]) == 0
    assert got["arg_rcs"].tolist() == [BAD_ARG] * 13
    assert got["arg_clean"].all() and got["arg_after"].all()
    assert got["arg_only_beta"].all()
    assert np.isfinite(got["arg_good_beta"]).all() and np.isfinite(got["arg_good_icpt"]).all()


# ---- (h) whole fits on the product library across the count-block edge ---------------------------------------------------------------
@pytest.fixture(scope="module")
def two_block_pair(mih, oracle):
    """n = 8320 (a second block of k_ib_counts, one tile long), p = 96, 3 % missing, an 80 % train mask."""
    rng = np.random.default_rng(8320)
    n, p = 8320, 96
    cols = make_bed(rng, n, p, 0.03)
    x = mih.SnpLinAlg(cols, n, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, n)
    train = (rng.random(n) < 0.8).astype(np.uint8)
    return x, ox, train


def test_fits_with_and_without_a_train_mask_across_the_count_block_edge(mih, oracle, two_block_pair):
    x, ox, train = two_block_pair
    rng = np.random.default_rng(8321)
    n = x.n
    z = np.column_stack([np.ones(n), rng.standard_normal(n)])
    y = _sim(oracle, ox, rng, 5, 0.7) + z @ np.array([0.5, 1.0]) + rng.standard_normal(n)
    for kw in (dict(), dict(train=train)):
        res = mih.fit_iht(y, x, z, k=6, init_beta=True, verbose=False, **kw)
        o = oracle.fit_iht(ox, y, z, k=6, init_beta=True, **kw)
        assert res.iter == o["iter"], kw.keys()
        assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
        np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(res.c, o["c"], rtol=1e-5)
        np.testing.assert_allclose(res.trace["logl"], o["logl_trace"], rtol=1e-9)
    folds = hash_folds(n, 3)
    mse = mih.cv_iht(y, x, z, path=[3, 5, 7], q=3, folds=folds, init_beta=True, verbose=False)
    omse, _ = oracle.cv_iht(ox, y, z, path=[3, 5, 7], q=3, folds=folds, init_beta=True)
    np.testing.assert_allclose(mse, omse, rtol=1e-5)


def test_three_trait_fit_with_a_train_mask_across_the_count_block_edge(mih, oracle, two_block_pair):
    x, ox, train = two_block_pair
    Y, Z = _mv_problem(oracle, ox, np.random.default_rng(8322), 3, 9, 2)
    res = mih.fit_iht(Y, x, Z, k=9, init_beta=True, train=train, verbose=False)
    o = oracle.fit_mv(ox, Y, Z, k=9, init_beta=True, train=train)
    assert res.iter == o["iter"] and list(res.trace["backtracks"]) == list(o["bt_trace"])
    assert np.array_equal(res.beta != 0, o["B"] != 0)
    np.testing.assert_allclose(res.beta, o["B"], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(res.c, o["C"], rtol=1e-5)
    np.testing.assert_allclose(res.trace["logl"], o["logl_trace"], rtol=1e-9)
