"""The saddlepoint-corrected association scan on the device (csrc/assoc_spa.hip: mih_assoc_score_spa; score_test_spa, assoc and
gwas with spa=True) against the numpy statement tests/spa_spec.py.

state must equal the spec's everywhere: spa_spec.edge_inputs redraws the few columns whose decision is not clear (its clear():
the guard, the evaluation limit, |r|, the cutoff and the end of the range, each with a margin; tests/test_spa_spec_cpu.py holds
the redrawn share below 10 %).  z, beta, se and neglog10p are mih_assoc_score's bit for bit; neglog10p_spa is neglog10p bit
for bit where state is 0 or 2, and within spa_spec.device_tolerance of the spec where state is 1 -- 16 x the spec's own
error against mpmath on these inputs (measured on the CPU) plus the plain scan's bound on z through the slope of the tail.  All
SPA outputs are compared bit for bit between slice_rows 0, 128, 256 and n and with a second call.  t_hat has NaN exactly where
the spec has (on the columns of state 0 and 1), and is compared loosely (1e-9: the root is a by-product, no bound is claimed for it).

Shapes: fewer rows than a wave, the 256 rows one pass of the workgroup covers and its neighbours, two and four passes; one
column, one more than a column group, several; 1 to 19 covariates; every flag triple; the three handle kinds.  The kernel's one
n-dependent path -- rows four at a time from n = 769 on -- has 1000 among the shapes and a test of its own (1024, 2500)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import assoc_spec as S
import gpu_helpers as H
import spa_spec as P
from conftest import FIX
from mendeliht_amd.api import ArgumentError
from test_gpu_assoc import bits, handle

pytestmark = pytest.mark.gpu

BAD_ARG = 2


@functools.lru_cache(maxsize=None)
def prepared(case):
    """The inputs of a case and the spec's answer, computed once and shared."""
    codes, y, eta, A, w, Z, _ = P.edge_inputs(case)
    sp = S.score(codes, case[4], A, w, Z)
    dz = S.bound(sp, codes, case[4], A, w, Z)[0]
    res = P.spa(sp, eta, Z, P.CUTOFF)
    for a in (codes, eta, A, w, Z):
        a.setflags(write=False)
    return codes, eta, A, w, Z, sp, dz, res


def spa_bits(r):
    return bits(r.neglog10p_spa, r.spa_state, r.t_hat)


def hold(got, plain, sp, dz, res, what, cols=None):
    """Assertions 1 - 5 of the issue on the columns cols (None: all); returns max err / tolerance over the state-1 columns."""
    p = sp["z"].shape[0]
    cols = np.arange(p) if cols is None else cols
    assert got.spa_state.dtype == np.uint8 and got.t_hat.shape == (p, 2)
    assert np.array_equal(got.spa_state[cols], res["state"][cols]), (what, np.flatnonzero(got.spa_state != res["state"])[:6].tolist())
    nan = np.isnan(sp["z"][:, 0])
    for a in (got.z, got.beta, got.se, got.neglog10p, got.neglog10p_spa):
        assert np.array_equal(np.isnan(a)[cols], nan[cols]), what
    assert bits(got.z, got.beta, got.se, got.neglog10p) == bits(plain.z, plain.beta, plain.se, plain.neglog10p), what
    one = cols[got.spa_state[cols] == 1]
    rest = cols[got.spa_state[cols] != 1]
    assert bits(got.neglog10p_spa[rest]) == bits(got.neglog10p[rest]), what
    sure = cols[got.spa_state[cols] != 2]          # (a refused column may sit exactly at the end of its range: which tails were tried is rounding's)
    assert np.array_equal(np.isnan(got.t_hat[sure]), np.isnan(res["t_hat"][sure])), what
    tol = P.device_tolerance(sp, res, dz)
    err = np.abs(got.neglog10p_spa[one] - res["neglog10p_spa"][one])
    worst = float((err / tol[one]).max()) if one.size else 0.0
    print(f"spa {what}: {one.size} saddlepoint columns, {int((got.spa_state[cols] == 2).sum())} refused, max err / tolerance = {worst:.3g}, "
          f"max relative error {float((err / res['neglog10p_spa'][one]).max()) if one.size else 0.0:.3g}")
    assert (err <= tol[one]).all(), (what, one[err > tol[one]][:4].tolist(), worst)
    ok = ~np.isnan(res["t_hat"][one])
    assert np.allclose(got.t_hat[one][ok], res["t_hat"][one][ok], rtol=1e-9, atol=0), what
    return worst


# ---- 1. edge shapes, 2-bit handles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", P.EDGE_P)
def test_edge_shapes(mih, p):
    cases = [c for c in P.edge_cases() if c[1] == p]
    assert len(cases) == len(P.EDGE_N)
    for case in cases:
        n = case[0]
        codes, eta, A, w, Z, sp, dz, res = prepared(case)
        x = handle(mih, codes, case[4])
        v = np.random.default_rng(case[5]).standard_normal(n)
        before = x.xtv(v)
        plain = x.score_test(A, w, Z)
        got = x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF)
        hold(got, plain, sp, dz, res, case)
        # cutoff = inf: no column is tried, the whole output is the plain scan's
        none = x.score_test_spa(A, w, Z, eta, cutoff=math.inf)
        assert (none.spa_state == 0).all() and np.isnan(none.t_hat).all(), case
        assert bits(none.z, none.beta, none.se, none.neglog10p, none.neglog10p_spa) == bits(plain.z, plain.beta, plain.se, plain.neglog10p, plain.neglog10p), case
        # bits: the row slices, a second call, and the handle is only read
        first = spa_bits(got)
        for sr in (0, 128, 256, n):
            again = x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF, slice_rows=sr)
            assert spa_bits(again) == first and bits(again.z, again.neglog10p) == bits(got.z, got.neglog10p), (case, sr)
        assert bits(x.xtv(v)) == bits(before), case


def test_rows_taken_four_at_a_time(mih):
    """A pass of k_assoc_spa loads a thread's rows four at a time and the last 0 .. 3 singly: n <= 768 (the shapes above but one)
    has single rows only; n = 2500 gives every thread two groups of four and one or two single rows, n = 1024 one group and none."""
    for case in P.EXTRA_CASES:
        codes, eta, A, w, Z, sp, dz, res = prepared(case)
        x = handle(mih, codes, case[4])
        got = x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF)
        hold(got, x.score_test(A, w, Z), sp, dz, res, case)
        assert spa_bits(x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF, slice_rows=256)) == spa_bits(got), case


def test_every_column_tried_with_cutoff_zero(mih):
    """cutoff = 0 tries every non-degenerate column: the columns whose decision is clear at this cutoff too are held to the spec."""
    case = [c for c in P.edge_cases() if c[:2] == (513, 150)][0]
    codes, eta, A, w, Z, sp, dz, _ = prepared(case)
    res = P.spa(sp, eta, Z, 0.0)
    clear = np.array([P.clear(sp, res, j, 0.0, dz) for j in range(150)])
    assert clear.mean() >= 0.9
    x = handle(mih, codes, case[4])
    got = x.score_test_spa(A, w, Z, eta, cutoff=0.0)
    assert np.array_equal(got.spa_state == 0, sp["deg"])
    hold(got, x.score_test(A, w, Z), sp, dz, res, case + ("cutoff 0",), cols=np.flatnonzero(clear))


# ---- 2. dosage and dense handles -----------------------------------------------------------------------------------------------------------
def _dense_problem(case, X):
    """The spec of a dense matrix X with the case's null model; the columns whose decision is clear."""
    codes, eta, A, w, Z, _, _, _ = prepared(case)
    sp = S.score_dense(X, A, w, Z)
    dz = S.bound(sp, None, None, A, w, Z)[0]
    res = P.spa(sp, eta, Z, P.CUTOFF)
    ok = np.array([sp["V"][j] / sp["Q"][j] >= S.MIN_V_OVER_Q and P.clear(sp, res, j, P.CUTOFF, dz) for j in range(X.shape[1])])
    return eta, A, w, Z, sp, dz, res, np.flatnonzero(ok)


@pytest.mark.parametrize("np_", [(65, 33), (257, 150), (1000, 33)])
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
        hold(x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF), x.score_test(A, w, Z), sp, dz, res, case + (dt.__name__,), cols=ok)


@pytest.mark.parametrize("np_", [(64, 33), (511, 33)])
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
    got = x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF)
    hold(got, x.score_test(A, w, Z), sp, dz, res, case + ("dosage",), cols=ok)
    assert spa_bits(x.score_test_spa(A, w, Z, eta, cutoff=P.CUTOFF, slice_rows=128)) == spa_bits(got)


# ---- 3. end to end on the shipped example -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped(mih, normal_data):
    n = normal_data["n"]
    bed = mih.read_bed(normal_data["bed"], n)
    y = normal_data["y"]
    yb = (y > np.quantile(y, 0.93)).astype(np.float64)               # 7 % cases
    return mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True), yb, normal_data["z"]


def test_assoc_with_spa_on_the_shipped_example(mih, shipped):
    x, yb, z = shipped
    res = x.assoc(yb, z, d=mih.Bernoulli(), spa=True)
    null = res.null
    assert null.converged
    direct = x.score_test_spa(null.A, null.w, z, null.eta, cutoff=2.0)
    assert bits(res.z, res.beta, res.se, res.neglog10p) + spa_bits(res) == bits(direct.z, direct.beta, direct.se, direct.neglog10p) + spa_bits(direct)
    plain = x.assoc(yb, z, d=mih.Bernoulli())
    assert plain.neglog10p_spa is None and plain.spa_state is None and plain.t_hat is None
    assert bits(plain.z, plain.neglog10p) == bits(res.z, res.neglog10p)
    tried = ~np.isnan(res.z) & (np.abs(res.z) >= 2.0)
    assert np.array_equal(res.spa_state != 0, tried) and (res.spa_state == 1).sum() >= 0.9 * tried.sum() > 100
    one = res.spa_state == 1
    assert np.median(res.neglog10p[one] - res.neglog10p_spa[one]) > 0            # 7 % cases: the normal tail overstates
    order = res.top(5)
    ok = np.flatnonzero(~np.isnan(res.neglog10p_spa))
    assert order.tolist() == ok[np.lexsort((ok, -res.neglog10p_spa[ok]))][:5].tolist()
    other = x.assoc(yb, z, d=mih.Bernoulli(), spa=True, spa_cutoff=3.0)
    assert np.array_equal(other.spa_state != 0, ~np.isnan(res.z) & (np.abs(res.z) >= 3.0))
    sel = other.spa_state != 0
    assert bits(other.neglog10p_spa[sel]) == bits(res.neglog10p_spa[sel])
    with pytest.raises(ArgumentError, match="Bernoulli"):
        x.assoc(yb, z, d=mih.Normal(), spa=True)
    with pytest.raises(ArgumentError, match="logit"):
        x.assoc(yb, z, d=mih.Bernoulli(), l=mih.ProbitLink(), spa=True)


def test_gwas_with_and_without_spa(mih, shipped, normal_data, tmp_path):
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
    out0, out1 = str(tmp_path / "plain.txt"), str(tmp_path / "spa.txt")
    res0 = mih.gwas(prefix, mih.Bernoulli, covariates=cov, outfile=out0)
    res1 = mih.gwas(prefix, mih.Bernoulli, covariates=cov, outfile=out1, spa=True)
    ref = x.assoc(yb, z, d=mih.Bernoulli(), spa=True)
    assert np.array_equal(res1.spa_state, ref.spa_state)
    assert np.allclose(res1.neglog10p_spa, ref.neglog10p_spa, rtol=1e-9, atol=1e-9, equal_nan=True)
    # without the option: the bytes of the file as it always was
    want = "chr\tpos\tSNPid\tref\talt\tz\tbeta\tse\tneglog10p\n" + "".join(
        f"1\t{j + 1}\tsnp{j + 1}\t1\t2\t{float(res0.z[j])!r}\t{float(res0.beta[j])!r}\t{float(res0.se[j])!r}\t{float(res0.neglog10p[j])!r}\n"
        for j in range(p))
    a = open(out0).read()
    assert res0.neglog10p_spa is None and len(a.splitlines()) == p + 1
    assert a == want
    b = open(out1).read().splitlines()
    assert b[0].split("\t") == ["chr", "pos", "SNPid", "ref", "alt", "z", "beta", "se", "neglog10p", "neglog10p_spa", "spa_state"]
    assert [ln.split("\t")[:9] for ln in b] == [ln.split("\t") for ln in a.splitlines()]
    j = int(res1.top(1)[0])
    row = b[j + 1].split("\t")
    assert float(row[9]) == res1.neglog10p_spa[j] and int(row[10]) == res1.spa_state[j]


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(mih):
    case = [c for c in P.edge_cases() if c[:2] == (257, 33)][0]
    codes, eta, A, w, Z, sp, dz, res = prepared(case)
    n, p, c = case[:3]
    x = handle(mih, codes, case[4])
    L = mih.lib()
    Zf = np.asfortranarray(Z)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(h=None, A_=A, w_=w, Z_=Zf, c_=c, eta_=eta, cutoff=P.CUTOFF, sr=0, null_out=None, t_hat=True):
        out = [np.full(p, 7.0) for _ in range(5)] + [np.full(p, 7, dtype=np.uint8), np.full(2 * p, 7.0)]
        ps = [ptr(o) for o in out]
        if null_out is not None:
            ps[null_out] = None
        if not t_hat:
            ps[6] = None
        rc = L.mih_assoc_score_spa(x._h if h is None else h, ptr(A_), ptr(w_), ptr(Z_), c_, ptr(eta_), C.c_double(cutoff), sr, *ps)
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
    for k in range(6):
        assert refused(null_out=k) == BAD_ARG, k
    assert refused(w_=None) == BAD_ARG and refused(eta_=None) == BAD_ARG and refused(A_=None) == BAD_ARG and refused(Z_=None) == BAD_ARG
    for cc in (0, -1, 65):
        assert refused(c_=cc) == BAD_ARG, cc
    assert refused(w_=bad(w, 5, np.nan)) == BAD_ARG and refused(w_=bad(w, 5, -1e-300)) == BAD_ARG
    assert refused(A_=bad(A, 3, np.inf)) == BAD_ARG and refused(Z_=bad(Zf, 1, np.nan)) == BAD_ARG
    assert refused(eta_=bad(eta, 0, np.nan)) == BAD_ARG and refused(eta_=bad(eta, n - 1, np.inf)) == BAD_ARG and refused(eta_=bad(eta, 7, -np.inf)) == BAD_ARG
    assert refused(cutoff=-1e-300) == BAD_ARG and refused(cutoff=-math.inf) == BAD_ARG and refused(sr=-1) == BAD_ARG
    assert refused(cutoff=math.nan) == BAD_ARG
    buf = C.create_string_buffer(512)
    L.mih_last_error(buf, 512)
    assert b"cutoff" in buf.value
    rc, out = call(t_hat=False)                                                   # t_hat may be NULL
    assert rc == 0 and not any((o == 7.0).all() for o in out[:5]) and (out[6] == 7.0).all()
    assert np.array_equal(out[5], res["state"])
    rc, out = call(cutoff=math.inf)
    assert rc == 0 and (out[5] == 0).all() and np.isnan(out[6]).all()
