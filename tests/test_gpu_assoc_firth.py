"""The Firth-penalised association scan on the device (csrc/assoc_firth.hip: mih_assoc_score_firth; score_test_firth, assoc and
gwas with firth=True) against the numpy statement tests/firth_spec.py.

firth_state must equal the spec's on every column whose decision is clear (firth_spec.clear(): the cutoff, the evaluation limit
and the guard on K2(b_hat), each with a margin; tests/test_firth_spec_cpu.py holds the share of the others below 10 %; they are
left out, not redrawn).  z, beta, se and neglog10p are mih_assoc_score's bit for bit; beta_firth, se_firth and neglog10p_firth
are beta, se and neglog10p bit for bit where the state is 0 or 2, and within firth_spec.device_tolerance of the spec where it
is 1 -- 16 x the spec's own error against mpmath on these inputs (measured on the CPU) plus the plain scan's bound on z carried
through the exact sensitivities of the root.  All Firth outputs, firth_evals included, are compared bit for bit between
slice_rows 0, 128, 256 and n and with a second call; firth_evals is not compared with the spec's.  With spa=True the
saddlepoint outputs are score_test_spa's bit for bit.

Shapes: those of the saddlepoint test (spa_spec.edge_cases() and EXTRA_CASES) -- fewer rows than a wave, the 256 rows one pass
of the workgroup covers and its neighbours, two and four passes; one column, one more than a column group, several; 1 to 19
covariates; every flag triple; the three handle kinds.  k_assoc_firth's unroll is k_assoc_spa's: rows four at a time from
n = 769 on and the last 0 .. 3 singly, so 1000, 1024 and 2500 are the shapes either side of its one threshold and it has no
other."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import assoc_spec as S
import firth_spec as F
import gpu_helpers as H
import spa_spec as P
from conftest import FIX
from mendeliht_amd.api import ArgumentError
from test_gpu_assoc import bits, handle
from test_gpu_assoc_spa import prepared, spa_bits

pytestmark = pytest.mark.gpu

BAD_ARG = 2
_SPEC = {}


def spec_of(case, cutoff=P.CUTOFF):
    """The Firth spec of a case on top of the shared inputs of the saddlepoint test, computed once."""
    if (case, cutoff) not in _SPEC:
        codes, eta, A, w, Z, sp, dz, _ = prepared(case)
        _SPEC[(case, cutoff)] = F.firth(sp, eta, Z, cutoff)
    return _SPEC[(case, cutoff)]


def firth_bits(r):
    return bits(r.beta_firth, r.se_firth, r.neglog10p_firth, r.firth_state, r.firth_evals)


def hold(got, plain, sp, dz, res, cutoff, what, cols=None):
    """The issue's assertions on the columns cols (None: all) whose decision is clear; returns the max err / tolerance of the
    three outputs over the state-1 columns."""
    p = sp["z"].shape[0]
    cols = np.arange(p) if cols is None else cols
    cols = np.array([j for j in cols if F.clear(sp, res, j, cutoff, dz)], dtype=np.int64)
    assert got.firth_state.dtype == np.uint8 and got.firth_evals.dtype == np.int32
    assert np.array_equal(got.firth_state[cols], res["state"][cols]), (what, cols[got.firth_state[cols] != res["state"][cols]][:6].tolist())
    nan = np.isnan(sp["z"][:, 0])
    for a in (got.z, got.beta, got.se, got.neglog10p, got.beta_firth, got.se_firth, got.neglog10p_firth):
        assert np.array_equal(np.isnan(a)[cols], nan[cols]), what
    assert bits(got.z, got.beta, got.se, got.neglog10p) == bits(plain.z, plain.beta, plain.se, plain.neglog10p), what
    every = np.arange(p)
    rest = every[got.firth_state != 1]
    assert bits(got.beta_firth[rest], got.se_firth[rest], got.neglog10p_firth[rest]) == bits(got.beta[rest], got.se[rest], got.neglog10p[rest]), what
    assert np.array_equal(got.firth_evals == 0, got.firth_state == 0) and (got.firth_evals <= F.MAX_EVALS).all(), what
    one = cols[got.firth_state[cols] == 1]
    tol = F.device_tolerance(sp, res, dz)
    worst = []
    for name, g, want, t in (("beta_firth", got.beta_firth, res["beta_firth"], tol[0]), ("se_firth", got.se_firth, res["se_firth"], tol[1]),
                             ("neglog10p_firth", got.neglog10p_firth, res["neglog10p_firth"], tol[2])):
        err = np.abs(g[one] - want[one])
        worst.append(float((err / t[one]).max()) if one.size else 0.0)
    print(f"firth {what}: {one.size} penalised columns, {int((got.firth_state[cols] == 2).sum())} refused, {p - cols.size} unclear, "
          f"max err / tolerance beta {worst[0]:.3g} se {worst[1]:.3g} neglog10p {worst[2]:.3g}, evaluations max {int(got.firth_evals.max())}")
    for name, g, want, t in (("beta_firth", got.beta_firth, res["beta_firth"], tol[0]), ("se_firth", got.se_firth, res["se_firth"], tol[1]),
                             ("neglog10p_firth", got.neglog10p_firth, res["neglog10p_firth"], tol[2])):
        err = np.abs(g[one] - want[one])
        assert (err <= t[one]).all(), (what, name, one[~(err <= t[one])][:4].tolist(), worst)
    return worst


# ---- 1. edge shapes, 2-bit handles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", P.EDGE_P)
def test_edge_shapes(mih, p):
    cases = [c for c in P.edge_cases() if c[1] == p]
    assert len(cases) == len(P.EDGE_N)
    for case in cases:
        n = case[0]
        codes, eta, A, w, Z, sp, dz, _ = prepared(case)
        res = spec_of(case)
        x = handle(mih, codes, case[4])
        v = np.random.default_rng(case[5]).standard_normal(n)
        before = x.xtv(v)
        plain = x.score_test(A, w, Z)
        got = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF)
        assert got.neglog10p_spa is None and got.spa_state is None and got.t_hat is None
        hold(got, plain, sp, dz, res, P.CUTOFF, case)
        # cutoff = inf: no column is tried, the whole output is the plain scan's
        none = x.score_test_firth(A, w, Z, eta, cutoff=math.inf)
        assert (none.firth_state == 0).all() and (none.firth_evals == 0).all(), case
        assert bits(none.z, none.beta, none.se, none.neglog10p, none.beta_firth, none.se_firth, none.neglog10p_firth) == \
            bits(plain.z, plain.beta, plain.se, plain.neglog10p, plain.beta, plain.se, plain.neglog10p), case
        # bits: the row slices, a second call, and the handle is only read
        first = firth_bits(got)
        for sr in (0, 128, 256, n):
            again = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF, slice_rows=sr)
            assert firth_bits(again) == first and bits(again.z, again.neglog10p) == bits(got.z, got.neglog10p), (case, sr)
        # both passes in one call: the saddlepoint outputs are score_test_spa's, the Firth outputs the same
        both = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF, spa=True)
        assert firth_bits(both) == first and spa_bits(both) == spa_bits(x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF)), case
        assert bits(x.xtv(v)) == bits(before), case


def test_rows_taken_four_at_a_time(mih):
    """A pass of k_assoc_firth loads a thread's rows four at a time and the last 0 .. 3 singly: n <= 768 (the shapes above but one)
    has single rows only; n = 2500 gives every thread two groups of four and one or two single rows, n = 1024 one group and none."""
    for case in P.EXTRA_CASES:
        codes, eta, A, w, Z, sp, dz, _ = prepared(case)
        x = handle(mih, codes, case[4])
        got = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF)
        hold(got, x.score_test(A, w, Z), sp, dz, spec_of(case), P.CUTOFF, case)
        both = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF, slice_rows=256, spa=True)
        assert firth_bits(both) == firth_bits(got) and spa_bits(both) == spa_bits(x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF)), case


def test_every_column_tried_with_cutoff_zero(mih):
    """cutoff = 0 tries every non-degenerate column."""
    case = [c for c in P.edge_cases() if c[:2] == (513, 150)][0]
    codes, eta, A, w, Z, sp, dz, _ = prepared(case)
    res = spec_of(case, 0.0)
    x = handle(mih, codes, case[4])
    got = x.score_test_firth(A, w, Z, eta, cutoff=0.0)
    assert np.array_equal(got.firth_state == 0, sp["deg"]) and (got.firth_state != 0).sum() == 147
    hold(got, x.score_test(A, w, Z), sp, dz, res, 0.0, case + ("cutoff 0",))


def test_boundary_columns_get_a_finite_estimate(mih):
    """Where every carrier is a case the saddlepoint is refused (state 2) and the device's Firth pass gives state 1."""
    for case in [c for c in P.edge_cases() if c[1] >= 31 and c[2] == 1][:3]:
        codes, eta, A, w, Z, sp, dz, spa = prepared(case)
        assert spa["state"][7] == 2
        x = handle(mih, codes, case[4])
        got = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF, spa=True)
        assert got.spa_state[7] == 2 and got.firth_state[7] == 1 and math.isfinite(got.beta_firth[7])
        assert got.neglog10p_firth[7] < got.neglog10p[7] and got.beta_firth[7] * got.beta[7] > 0


# ---- 2. dosage and dense handles -----------------------------------------------------------------------------------------------------------
def _dense_problem(case, X):
    """The spec of a dense matrix X with the case's null model; the columns the plain scan's spec keeps."""
    codes, eta, A, w, Z, _, _, _ = prepared(case)
    sp = S.score_dense(X, A, w, Z)
    dz = S.bound(sp, None, None, A, w, Z)[0]
    res = F.firth(sp, eta, Z, P.CUTOFF)
    ok = np.array([sp["V"][j] / sp["Q"][j] >= S.MIN_V_OVER_Q for j in range(X.shape[1])])
    return eta, A, w, Z, sp, dz, res, np.flatnonzero(ok)


SIDE_SHAPES = [(65, 33), (257, 150), (1000, 33)]


@pytest.mark.parametrize("np_", SIDE_SHAPES)
def test_dense_handles(mih, np_):
    case = [c for c in P.edge_cases() if c[:2] == np_][0]
    codes = prepared(case)[0]
    keep = np.flatnonzero(~S.degenerate(codes))                  # (a constant dense column has V = 0 up to rounding: not a case of this test)
    X = S.xtilde(codes, case[4])[:, keep]
    for dt in (np.float64, np.float32):
        Xd = np.asfortranarray(X.astype(dt))
        eta, A, w, Z, sp, dz, res, ok = _dense_problem(case, Xd.astype(np.float64))
        assert ok.size >= 0.9 * keep.size
        x = mih.DenseMatrix(Xd)
        got = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF)
        hold(got, x.score_test(A, w, Z), sp, dz, res, P.CUTOFF, case + (dt.__name__,), cols=ok)
        assert firth_bits(x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF, slice_rows=128)) == firth_bits(got)


@pytest.mark.parametrize("np_", SIDE_SHAPES)
def test_dosage_handles(mih, np_):
    case = [c for c in P.edge_cases() if c[:2] == np_][0]
    codes = prepared(case)[0]
    keep = np.flatnonzero(~S.degenerate(codes))
    den = 100
    rng = np.random.default_rng(case[5])
    num = codes[:, keep] * den
    num = np.where((num > 0) & (num < 2 * den), num + rng.integers(-30, 31, num.shape), num)      # fractional dosages around 1
    num = np.where(codes[:, keep] < 0, 0xFFFF, num).astype(np.uint16)
    mun, sc, _, _ = H.dosage_host_stats(num, den)
    X = np.where(num == 0xFFFF, 0.0, (num.astype(np.float64) - mun[None, :]) * sc[None, :])
    eta, A, w, Z, sp, dz, res, ok = _dense_problem(case, X)
    assert ok.size >= 0.9 * keep.size
    x = mih.DosageMatrix(num, den)
    got = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF)
    hold(got, x.score_test(A, w, Z), sp, dz, res, P.CUTOFF, case + ("dosage",), cols=ok)
    both = x.score_test_firth(A, w, Z, eta, cutoff=P.CUTOFF, slice_rows=128, spa=True)
    assert firth_bits(both) == firth_bits(got) and spa_bits(both) == spa_bits(x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF))


# ---- 3. end to end on the shipped example -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped(mih, normal_data):
    n = normal_data["n"]
    bed = mih.read_bed(normal_data["bed"], n)
    y = normal_data["y"]
    yb = (y > np.quantile(y, 0.93)).astype(np.float64)               # 7 % cases
    return mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True), yb, normal_data["z"]


def test_assoc_with_firth_on_the_shipped_example(mih, shipped):
    x, yb, z = shipped
    res = x.assoc(yb, z, d=mih.Bernoulli(), firth=True)
    null = res.null
    assert null.converged and res.neglog10p_spa is None and res.spa_state is None
    direct = x.score_test_firth(null.A, null.w, z, null.eta, cutoff=2.0)
    assert bits(res.z, res.beta, res.se, res.neglog10p) + firth_bits(res) == bits(direct.z, direct.beta, direct.se, direct.neglog10p) + firth_bits(direct)
    plain = x.assoc(yb, z, d=mih.Bernoulli())
    assert plain.beta_firth is None and plain.se_firth is None and plain.neglog10p_firth is None and plain.firth_state is None and plain.firth_evals is None
    assert bits(plain.z, plain.neglog10p) == bits(res.z, res.neglog10p)
    tried = ~np.isnan(res.z) & (np.abs(res.z) >= 2.0)
    assert np.array_equal(res.firth_state != 0, tried) and (res.firth_state == 1).sum() >= 0.99 * tried.sum() > 100
    one = res.firth_state == 1
    assert (np.sign(res.beta_firth[one]) == np.sign(res.beta[one])).all()
    assert np.isfinite(res.beta_firth[one]).all() and (res.se_firth[one] > 0).all() and (res.neglog10p_firth[one] >= 0).all()
    assert res.top(5).tolist() == plain.top(5).tolist()              # top() is unchanged: by |z| without the saddlepoint pass
    # both passes in one call, on one selection
    both = x.assoc(yb, z, d=mih.Bernoulli(), spa=True, firth=True)
    spa = x.assoc(yb, z, d=mih.Bernoulli(), spa=True)
    assert firth_bits(both) == firth_bits(res) and spa_bits(both) == spa_bits(spa)
    assert both.top(5).tolist() == spa.top(5).tolist()
    other = x.assoc(yb, z, d=mih.Bernoulli(), firth=True, firth_cutoff=3.0)
    sel = other.firth_state != 0
    assert np.array_equal(sel, ~np.isnan(res.z) & (np.abs(res.z) >= 3.0))
    assert bits(other.beta_firth[sel], other.neglog10p_firth[sel]) == bits(res.beta_firth[sel], res.neglog10p_firth[sel])
    with pytest.raises(ArgumentError, match="Bernoulli"):
        x.assoc(yb, z, d=mih.Normal(), firth=True)
    with pytest.raises(ArgumentError, match="logit"):
        x.assoc(yb, z, d=mih.Bernoulli(), l=mih.ProbitLink(), firth=True)
    with pytest.raises(ArgumentError, match="one trait"):
        x.assoc(np.stack([yb, yb], axis=1), z, d=mih.Bernoulli(), firth=True)
    with pytest.raises(ArgumentError, match="firth_cutoff"):
        x.assoc(yb, z, d=mih.Bernoulli(), spa=True, firth=True, spa_cutoff=2.0, firth_cutoff=3.0)


def test_gwas_with_firth(mih, shipped, normal_data, tmp_path):
    import shutil
    x, yb, z = shipped
    n, p = normal_data["n"], x.p
    prefix = str(tmp_path / "binary")
    shutil.copy(normal_data["bed"], prefix + ".bed")
    with open(prefix + ".fam", "w") as f:
        f.writelines(f"{i + 1} 1 0 0 1 {int(yb[i])}\n" for i in range(n))
    with open(prefix + ".bim", "w") as f:
        f.writelines(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n" for j in range(p))
    cov = os.path.join(FIX, "covariates.txt")
    out0, out1, out2 = str(tmp_path / "plain.txt"), str(tmp_path / "firth.txt"), str(tmp_path / "both.txt")
    mih.gwas(prefix, mih.Bernoulli, covariates=cov, outfile=out0)
    res1 = mih.gwas(prefix, mih.Bernoulli, covariates=cov, outfile=out1, firth=True)
    res2 = mih.gwas(prefix, mih.Bernoulli, covariates=cov, outfile=out2, firth=True, spa=True)
    ref = x.assoc(yb, z, d=mih.Bernoulli(), firth=True)
    assert np.array_equal(res1.firth_state, ref.firth_state) and res1.neglog10p_spa is None and res2.neglog10p_spa is not None
    assert np.allclose(res1.beta_firth, ref.beta_firth, rtol=1e-9, atol=1e-9, equal_nan=True)
    a = open(out0).read().splitlines()
    b = open(out1).read().splitlines()
    c = open(out2).read().splitlines()
    head = ["chr", "pos", "SNPid", "ref", "alt", "z", "beta", "se", "neglog10p"]
    tail = ["beta_firth", "se_firth", "neglog10p_firth", "firth_state"]
    assert a[0].split("\t") == head and b[0].split("\t") == head + tail and c[0].split("\t") == head + ["neglog10p_spa", "spa_state"] + tail
    assert [ln.split("\t")[:9] for ln in b] == [ln.split("\t") for ln in a] and len(b) == p + 1
    assert [ln.split("\t")[11:] for ln in c] == [ln.split("\t")[9:] for ln in b]
    j = int(np.flatnonzero(res1.firth_state == 1)[0])
    row = b[j + 1].split("\t")
    assert [float(v) for v in row[9:12]] == [res1.beta_firth[j], res1.se_firth[j], res1.neglog10p_firth[j]] and int(row[12]) == 1


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(mih):
    case = [c for c in P.edge_cases() if c[:2] == (257, 33)][0]
    codes, eta, A, w, Z, sp, dz, spa = prepared(case)
    res = spec_of(case)
    n, p, c = case[:3]
    x = handle(mih, codes, case[4])
    L = mih.lib()
    Zf = np.asfortranarray(Z)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(h=None, A_=A, w_=w, Z_=Zf, c_=c, eta_=eta, cutoff=P.CUTOFF, sr=0, null_out=(), with_spa=True):
        # z, beta, se, neglog10p, beta_firth, se_firth, neglog10p_firth, firth_state, firth_evals, neglog10p_spa, spa_state, t_hat
        out = [np.full(p, 7.0) for _ in range(7)] + [np.full(p, 7, dtype=np.uint8), np.full(p, 7, dtype=np.int32), np.full(p, 7.0),
                                                      np.full(p, 7, dtype=np.uint8), np.full(2 * p, 7.0)]
        ps = [ptr(o) for o in out]
        for k in null_out:
            ps[k] = None
        if not with_spa:
            ps[9] = None
        rc = L.mih_assoc_score_firth(x._h if h is None else h, ptr(A_), ptr(w_), ptr(Z_), c_, ptr(eta_), C.c_double(cutoff), sr, *ps)
        return rc, out

    def refused(**kw):
        rc, out = call(**kw)
        assert all((o == 7).all() for o in out), ("outputs written", kw.keys())
        return rc

    def bad(v, i, val):
        b = np.array(v, order="F", copy=True)
        b.reshape(-1, order="F")[i] = val
        return b
    assert refused(h=C.c_void_p(None)) == BAD_ARG
    for k in range(8):                                                           # a null plain or Firth output
        assert refused(null_out=(k,)) == BAD_ARG, k
    assert refused(null_out=(10,)) == BAD_ARG                                    # neglog10p_spa given: spa_state is required
    assert refused(w_=None) == BAD_ARG and refused(eta_=None) == BAD_ARG and refused(A_=None) == BAD_ARG and refused(Z_=None) == BAD_ARG
    for cc in (0, -1, 65):
        assert refused(c_=cc) == BAD_ARG, cc
    assert refused(w_=bad(w, 5, np.nan)) == BAD_ARG and refused(w_=bad(w, 5, -1e-300)) == BAD_ARG
    assert refused(A_=bad(A, 3, np.inf)) == BAD_ARG and refused(Z_=bad(Zf, 1, np.nan)) == BAD_ARG
    assert refused(eta_=bad(eta, 0, np.nan)) == BAD_ARG and refused(eta_=bad(eta, n - 1, np.inf)) == BAD_ARG and refused(eta_=bad(eta, 7, -np.inf)) == BAD_ARG
    assert refused(cutoff=-1e-300) == BAD_ARG and refused(cutoff=-math.inf) == BAD_ARG and refused(sr=-1) == BAD_ARG
    assert refused(cutoff=math.nan, with_spa=False) == BAD_ARG
    buf = C.create_string_buffer(512)
    L.mih_last_error(buf, 512)
    assert b"cutoff" in buf.value and b"mih_assoc_score_firth" in buf.value
    clear = np.array([F.clear(sp, res, j, P.CUTOFF, dz) for j in range(p)])
    rc, out = call(null_out=(8, 11))                                             # firth_evals and t_hat may be NULL
    assert rc == 0 and not any((o == 7.0).all() for o in out[:7]) and (out[8] == 7).all() and (out[11] == 7.0).all()
    assert np.array_equal(out[7][clear], res["state"][clear]) and np.array_equal(out[10], spa["state"])
    rc, out = call(with_spa=False)                                               # no saddlepoint pass: its outputs are not touched
    assert rc == 0 and (out[9] == 7.0).all() and (out[10] == 7).all() and (out[11] == 7.0).all()
    assert np.array_equal(out[7][clear], res["state"][clear]) and np.array_equal(out[8] == 0, out[7] == 0)
    rc, out = call(with_spa=False, null_out=(10, 11))                            # ... and spa_state is not required
    assert rc == 0 and np.array_equal(out[7][clear], res["state"][clear])
    rc, out = call(cutoff=math.inf)
    assert rc == 0 and (out[7] == 0).all() and (out[8] == 0).all() and (out[10] == 0).all() and np.isnan(out[11]).all()
    assert bits(out[4], out[5], out[6]) == bits(out[1], out[2], out[3])
