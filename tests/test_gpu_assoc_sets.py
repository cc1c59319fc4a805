"""The set-based tests on the device (csrc/assoc_sets.hip: mih_assoc_sets; set_test and assoc_sets of the matrix classes) against the
numpy statement tests/sets_spec.py.

(a) z, beta, se and neglog10p are score_test's bit for bit.  (b) m_used, skat_state and the NaN patterns equal the spec's:
sets_spec.edge_inputs redraws the few sets whose decision is not clear (tests/test_sets_spec_cpu.py holds their share below 10 %).
(c) cov: the diagonal is V bit for bit, the rest within sets_spec.cov_bound.  (d) lambda within sets_spec.lambda_bound of
numpy.linalg.eigvalsh of the spec's M.  (e) burden_z, neglog10p_burden and neglog10p_skat within sets_spec.device_tolerance, built
from the spec alone.  (f) every set output is the same bits across slice_rows 0, 128, 256 and n, in a second call, with the list of
sets reversed and with a set alone in its call.  (g) x.xtv(v) has the same bits before and after.  (h) the refusals.  (i) nsets = 0.
(j) assoc_sets with Beta weights on a scaled and an unscaled handle.

Shapes: n below one k-step of the f64 MFMA and no multiple of 4 (15), one decode chunk (32) and one more row (33), several chunks
with a tail; p = 150; sets of 1, 2, 15, 16, 17, 33, 64, 65, 127 and 128 entries -- the block edges of the 16 x 16 tiling, the edge
of the eigen-solver's LDS path (64 / 65) and its order limit; overlapping sets, a degenerate column in a set, a set of degenerate
columns only, an omega = 0 entry, a duplicated column; 0 and 3 % missing; every flag triple; the three handle kinds."""
import ctypes as C
import functools
import math
import os
import shutil

import numpy as np
import pytest

import assoc_spec as S
import gpu_helpers as H
import sets_spec as T
from conftest import FIX
from mendeliht_amd.api import ArgumentError
from test_gpu_assoc import bits, handle

pytestmark = pytest.mark.gpu

BAD_ARG = 2


@functools.lru_cache(maxsize=None)
def prepared(case):
    """The inputs of a case, the spec's answer and the scan's bounds, computed once and shared."""
    codes, A, w, Z, sets, omega, sp, res, _ = T.edge_inputs(case)
    bounds = T.scan_bounds(sp, codes, case[4], A, w, Z)
    for a in (codes, A, Z) + (() if w is None else (w,)):
        a.setflags(write=False)
    return codes, A, w, Z, sets, omega, sp, res, bounds


def set_bits(r, s=None):
    """The bits of every set output (of set s alone: its slices)."""
    if s is None:
        return bits(r.m_used, r.burden_z, r.neglog10p_burden, r.skat_q, r.neglog10p_skat, r.skat_state, r.lambdas, *r.cov)
    lo, hi = r.set_ptr[s], r.set_ptr[s + 1]
    return bits(r.m_used[s], r.burden_z[s], r.neglog10p_burden[s], r.skat_q[s], r.neglog10p_skat[s], r.skat_state[s], r.lambdas[lo:hi], r.cov[s])


def hold(got, sp, w, res, bounds, what):
    """Assertions (b) - (e) on every set; returns the worst err / tolerance of (c), (d) and (e)."""
    assert got.m_used.dtype == np.int32 and got.skat_state.dtype == np.uint8
    assert np.array_equal(got.m_used, res["m_used"]), (what, got.m_used.tolist(), res["m_used"].tolist())
    assert np.array_equal(got.skat_state, res["skat_state"]), (what, got.skat_state.tolist(), res["skat_state"].tolist())
    for name, a in (("burden_z", got.burden_z), ("neglog10p_burden", got.neglog10p_burden), ("neglog10p_skat", got.neglog10p_skat),
                    ("skat_q", got.skat_q), ("lambdas", got.lambdas)):
        assert np.array_equal(np.isnan(a), np.isnan(res[name])), (what, name)
    worst = dict(cov=0.0, lam=0.0, bz=0.0, bp=0.0, skat=0.0)
    V = got.cov_diag_want
    for s, d in enumerate(res["detail"]):
        m = len(d["cols"])
        full = got.cov[s]
        assert np.array_equal(np.isnan(full), np.isnan(res["cov"][s])), (what, s)
        if m == 0:
            continue
        K = full[np.ix_(d["mem"], d["mem"])]
        assert bits(np.diag(K)) == bits(V[d["cols"]]), (what, s, "the diagonal is not the scan's V")
        assert np.array_equal(K, K.T), (what, s)
        dK = T.cov_bound(sp, w, d, bounds)
        off = ~np.eye(m, dtype=bool)
        err = np.abs(K - d["K"])
        assert (err[off] <= dK[off]).all(), (what, s, "cov", float((err[off] / dK[off]).max()))
        if off.any():
            worst["cov"] = max(worst["cov"], float((err[off] / dK[off]).max()))
        tz, tb, ts, dlam = T.device_tolerance(sp, d, bounds, dK)
        lam = got.lambdas[got.set_ptr[s]:got.set_ptr[s] + m]
        assert (np.diff(lam) <= 0).all() and (lam >= 0).all(), (what, s)
        el = np.abs(lam - d["lam"]).max()
        assert el <= dlam, (what, s, "lambda", el, dlam)
        worst["lam"] = max(worst["lam"], el / dlam)
        assert abs(got.skat_q[s] - d["Q"]) <= T.q_bound(sp, d, bounds), (what, s, "Q")
        if not math.isnan(res["burden_z"][s]):
            eb, ep = abs(got.burden_z[s] - res["burden_z"][s]), abs(got.neglog10p_burden[s] - res["neglog10p_burden"][s])
            assert eb <= tz and ep <= tb, (what, s, "burden", eb, tz, ep, tb)
            worst["bz"], worst["bp"] = max(worst["bz"], eb / tz), max(worst["bp"], ep / tb)
        if d["tail"]["state"] in (1, 2):
            es = abs(got.neglog10p_skat[s] - res["neglog10p_skat"][s])
            assert es <= ts, (what, s, "skat", d["tail"]["state"], es, ts)
            worst["skat"] = max(worst["skat"], es / ts)
    print(f"sets {what}: states {np.bincount(got.skat_state, minlength=6).tolist()}, max err / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


def run(x, A, w, Z, sets, omega, **kw):
    r = x.set_test(A, w, Z, [np.asarray(s) for s in sets], [np.asarray(o) for o in omega], cov=True, **kw)
    return r


# ---- 1. edge shapes, 2-bit handles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(T.EDGE_CASES)))
def test_edge_shapes(mih, k):
    case = T.EDGE_CASES[k]
    codes, A, w, Z, sets, omega, sp, res, bounds = prepared(case)
    n = codes.shape[0]
    x = handle(mih, codes, case[4])
    v = np.random.default_rng(k).standard_normal(n)
    before = x.xtv(v)
    plain = x.score_test(A, w, Z)
    got = run(x, A, w, Z, sets, omega)
    assert bits(got.assoc.z, got.assoc.beta, got.assoc.se, got.assoc.neglog10p) == bits(plain.z, plain.beta, plain.se, plain.neglog10p), case     # (a)
    # the scan's V is no output of its own: the one-column sets return it (their 1 x 1 cov), every other set's diagonal must be those bits
    ones = x.set_test(A, w, Z, [np.array([j]) for j in range(T.EDGE_P)], cov=True)
    got.cov_diag_want = np.array([c[0, 0] for c in ones.cov])
    assert np.array_equal(np.isnan(got.cov_diag_want), np.isnan(sp["V"]))
    ok = ~np.isnan(sp["V"])
    assert (np.abs(got.cov_diag_want[ok] - sp["V"][ok]) <= bounds[1][ok]).all(), case
    hold(got, sp, w, res, bounds, case)                                                                        # (b) - (e)
    # one-member sets with omega = 1: both tests give the scan's p, SKAT in state 2
    assert bits(ones.neglog10p_burden[ok]) == bits(plain.neglog10p[ok]) and bits(ones.neglog10p_skat[ok]) == bits(plain.neglog10p[ok]), case
    assert (ones.skat_state[ok] == 2).all() and (ones.skat_state[~ok] == 0).all() and np.array_equal(ones.m_used, ok.astype(np.int32)), case
    first = set_bits(got)                                                                                    # (f)
    for sr in (128, 256, n):
        assert set_bits(run(x, A, w, Z, sets, omega, slice_rows=sr)) == first, (case, sr)
    assert set_bits(run(x, A, w, Z, sets, omega)) == first, case
    rev = run(x, A, w, Z, sets[::-1], omega[::-1])
    ns = len(sets)
    for s in range(ns):
        assert set_bits(rev, ns - 1 - s) == set_bits(got, s), (case, s, "reversed list")
    for s in (0, 4, 8, 9, ns - 1):
        assert set_bits(run(x, A, w, Z, [sets[s]], [omega[s]]), 0) == set_bits(got, s), (case, s, "alone")
    assert set_bits(got, ns - 1) == set_bits(got, 4), case          # the same set twice in one list
    assert bits(x.xtv(v)) == bits(before), case                                                               # (g)


# ---- 2. dosage and dense handles ----------------------------------------------------------------------------------------------------------
def _aux(n, c, seed, weighted):
    rng = np.random.default_rng(seed)
    Z = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1)
    w = rng.uniform(0.05, 0.25, n) if weighted else None
    A = rng.standard_normal(n)
    wz = Z if w is None else w[:, None] * Z
    return A - wz @ np.linalg.solve(Z.T @ wz, Z.T @ A), w, Z


def _sets_among(keep, seed, sizes):
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(keep, min(k, keep.size), replace=False)) for k in sizes]
    return sets, [rng.uniform(0.5, 2.0, s.size) for s in sets]


def _hold_dense(x, X, A, w, Z, sizes, what, allowed=None, dead=()):
    """The assertions on a dense / dosage handle: sets of the given sizes among the well-conditioned columns (of `allowed`), and --
    with `dead`, columns the scan finds degenerate -- one set that holds two of those beside two members."""
    sp = S.score_dense(X, A, w, Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        fine = sp["V"] / sp["Q"] >= 10 * S.MIN_V_OVER_Q
    keep = np.flatnonzero(fine if allowed is None else fine & np.isin(np.arange(X.shape[1]), allowed))
    assert keep.size >= 20
    bounds = T.scan_bounds(sp, None, None, A, w, Z)
    sets, omega = _sets_among(keep, 5, sizes)
    if len(dead):
        assert np.isnan(sp["V"][list(dead)]).all()
        sets.append(np.sort(np.concatenate([keep[:2], np.asarray(dead)])))
        omega.append(np.ones(sets[-1].size))
    res = T.set_test(sp, w, sets, omega)
    assert all(T.clear(d) for d in res["detail"]), what
    plain = x.score_test(A, w, Z)
    got = run(x, A, w, Z, sets, omega)
    assert bits(got.assoc.z, got.assoc.beta, got.assoc.se, got.assoc.neglog10p) == bits(plain.z, plain.beta, plain.se, plain.neglog10p), what
    ones = x.set_test(A, w, Z, [np.array([j]) for j in range(X.shape[1])], cov=True)
    got.cov_diag_want = np.array([c[0, 0] for c in ones.cov])
    hold(got, sp, w, res, bounds, what)
    assert set_bits(run(x, A, w, Z, sets, omega, slice_rows=128)) == set_bits(got), what


@pytest.mark.parametrize("shape", [(17, 1, False), (129, 3, True), (1025, 5, True)])
def test_dosage_handles(mih, shape):
    n, c, weighted = shape
    den = 255
    num = np.concatenate([H.edge_matrix(n, den, 40 + n + 1000 * k) for k in range(4)], axis=1)      # 36 ordinary columns among 80
    mun, sc, _, _ = H.dosage_host_stats(num, den)
    X = np.where(num == 0xFFFF, 0.0, (num.astype(np.float64) - mun[None, :]) * sc[None, :])
    good = np.flatnonzero((np.abs(X) > 0).sum(axis=0) > max(3, n // 20))             # the near-constant columns of edge_matrix have V / Q ~ 0
    A, w, Z = _aux(n, c, 50 + n, weighted)
    _hold_dense(mih.DosageMatrix(num, den), X, A, w, Z, (1, 2, 7, 16, 17), ("dosage",) + shape, allowed=good, dead=(6, 9))


@pytest.mark.parametrize("shape", [(17, 1, False), (257, 3, True)])
def test_dense_handles(mih, shape):
    n, c, weighted = shape
    X = np.random.default_rng(60 + n).standard_normal((n, 140))
    A, w, Z = _aux(n, c, 70 + n, weighted)
    for dt in (np.float64, np.float32):
        Xd = np.asfortranarray(X.astype(dt))
        _hold_dense(mih.DenseMatrix(Xd), Xd.astype(np.float64), A, w, Z, (1, 2, 16, 17, 65, 128), ("dense", dt.__name__) + shape)


# ---- 3. refusals, nsets = 0 ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(mih):
    n, p = 129, 33
    codes, A, w, Z = S.edge_inputs((n, p, 1, 2, 0.03, (1, 1, 1), "logistic", 4242))
    x = handle(mih, codes, (1, 1, 1))
    L = mih.lib()
    A, Z = np.ascontiguousarray(A[:, 0]), np.asfortranarray(Z)
    ptr0, col0, om0 = np.array([0, 2, 5], dtype=np.int64), np.array([1, 2, 4, 8, 9], dtype=np.int32), np.ones(5)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(h=None, A_=A, w_=w, Z_=Z, c=2, sr=0, ns=2, sp_=ptr0, sc_=col0, om_=om0, null_out=None):
        out = [np.full(p, 7.0) for _ in range(4)] + [np.full(2, 7, dtype=np.int32)] + [np.full(2, 7.0) for _ in range(4)] + \
              [np.full(2, 7, dtype=np.uint8), np.full(5, 7.0), np.full(13, 7.0)]
        ps = [ptr(o) for o in out]
        if null_out is not None:
            ps[null_out] = None
        rc = L.mih_assoc_sets(x._h if h is None else h, ptr(A_), ptr(w_), ptr(Z_), c, sr, ns, ptr(sp_), ptr(sc_), ptr(om_), *ps)
        assert all((o == 7).all() for o in out), "outputs written"
        return rc

    def bad(v, i, val):
        b = np.array(v, order="F", copy=True)
        b.reshape(-1, order="F")[i] = val
        return b
    assert call(h=C.c_void_p(None)) == BAD_ARG
    for k in range(10):                                      # z .. skat_state are required; lambda and cov may be NULL
        assert call(null_out=k) == BAD_ARG, k
    for c in (0, -1, 65):
        assert call(c=c) == BAD_ARG, c
    assert call(w_=bad(w, 5, np.nan)) == BAD_ARG and call(w_=bad(w, 5, -1e-300)) == BAD_ARG and call(w_=bad(w, 128, np.inf)) == BAD_ARG
    assert call(A_=bad(A, 3, np.inf)) == BAD_ARG and call(Z_=bad(Z, n + 1, np.nan)) == BAD_ARG
    assert call(w_=np.zeros(n)) == BAD_ARG and call(sr=-1) == BAD_ARG
    assert call(ns=-1) == BAD_ARG
    assert call(sp_=None) == BAD_ARG and call(sc_=None) == BAD_ARG and call(om_=None) == BAD_ARG
    assert call(sp_=np.array([1, 2, 5], dtype=np.int64)) == BAD_ARG                       # does not start at 0
    assert call(sp_=np.array([0, 3, 2], dtype=np.int64)) == BAD_ARG                       # decreases
    big = np.arange(129, dtype=np.int32) % p
    assert call(ns=1, sp_=np.array([0, 129], dtype=np.int64), sc_=big, om_=np.ones(129)) == BAD_ARG       # more than 128 entries
    assert call(sc_=bad(col0, 4, p)) == BAD_ARG and call(sc_=bad(col0, 0, -1)) == BAD_ARG                # outside [0, p)
    assert call(sc_=bad(col0, 3, 4)) == BAD_ARG and call(sc_=bad(col0, 1, 0)) == BAD_ARG                 # equal, descending
    for v in (-1e-300, np.nan, np.inf):
        assert call(om_=bad(om0, 2, v)) == BAD_ARG, v
    buf = C.create_string_buffer(512)
    L.mih_last_error(buf, 512)
    assert b"weight 1 of set 2" in buf.value, buf.value
    # through the Python mirror: ArgumentError
    for sets, om in (([[2, 1]], None), ([[0, p]], None), ([[-1, 3]], None), ([list(range(33)) * 4], None), ([[1, 2]], [[1.0, -1.0]]), ([[1, 2]], [[np.nan, 1.0]]),
                     ((np.array([0, 3, 2]), np.array([1, 2])), None), ((np.array([1, 2]), np.array([1, 2])), None)):
        with pytest.raises(ArgumentError):
            x.set_test(A, w, Z, sets, om)
    with pytest.raises(ArgumentError):
        x.set_test(A, bad(w, 0, -1.0), Z, [[1, 2]])
    # lambda and cov may be NULL
    out = [np.full(p, 7.0) for _ in range(4)] + [np.full(2, 7, dtype=np.int32)] + [np.full(2, 7.0) for _ in range(4)] + [np.full(2, 7, dtype=np.uint8)]
    assert L.mih_assoc_sets(x._h, ptr(A), ptr(w), ptr(Z), 2, 0, 2, ptr(ptr0), ptr(col0), ptr(om0), *[ptr(o) for o in out], None, None) == 0
    assert out[4].tolist() == [2, 3] and not (out[5] == 7.0).any()


def test_no_sets_is_the_plain_scan(mih):
    n, p = 129, 33
    codes, A, w, Z = S.edge_inputs((n, p, 1, 2, 0.03, (1, 1, 1), "logistic", 4242))
    x = handle(mih, codes, (1, 1, 1))
    plain = x.score_test(A[:, 0], w, Z)
    for sets in ([], (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))):
        got = x.set_test(A[:, 0], w, Z, sets, cov=True)
        assert bits(got.assoc.z, got.assoc.beta, got.assoc.se, got.assoc.neglog10p) == bits(plain.z, plain.beta, plain.se, plain.neglog10p)
        assert got.m_used.size == 0 and got.lambdas.size == 0 and got.cov == [] and got.top(3).size == 0
    empty = x.set_test(A[:, 0], w, Z, [[], [1, 2]])          # an empty set among others: no members
    assert empty.m_used.tolist() == [0, 2] and empty.skat_state[0] == 0 and np.isnan(empty.neglog10p_burden[0]) and empty.skat_q[0] == 0.0


# ---- 4. the host mirror ---------------------------------------------------------------------------------------------------------------------
def test_assoc_sets_beta_weights_do_not_depend_on_the_scaling_of_the_handle(mih):
    """(j): omega = Beta(maf; 1, 25) / sinv on the scaled handle is SKAT's weighting of the raw genotypes, so a scaled and an
    unscaled handle of the same genotypes give the same p-values.  Each is held to its own spec by the tolerance of (e); the two
    specs agree only as far as the null fit solves its score equations (fit_null stops at a relative deviance change of 1e-8, which
    leaves sum A ~ 1e-10 and the centring not quite projected out), so the device values may differ by the two tolerances plus
    the difference of the two specs, which is held below 1e-9 of the value."""
    case = T.EDGE_CASES[7]
    codes, _, _, Z, sets, _, _, _, _ = prepared(case)
    n = codes.shape[0]
    rng = np.random.default_rng(3)
    y = (rng.random(n) < 0.3).astype(np.float64)
    sets = [np.asarray(s) for s in sets if len(s) > 1][:8]
    got, want, tols = {}, {}, {}
    for flags in ((1, 1, 1), (0, 0, 1)):
        r = handle(mih, codes, flags).assoc_sets(y, Z, sets, d=mih.Bernoulli())
        null = r.assoc.null
        sp = S.score(codes, flags, null.A, null.w, Z)
        bounds = T.scan_bounds(sp, codes, flags, null.A, null.w, Z)
        res = T.set_test(sp, null.w, sets, [r.omega[r.set_ptr[k]:r.set_ptr[k + 1]] for k in range(len(sets))])
        assert np.array_equal(r.m_used, res["m_used"]) and np.array_equal(r.skat_state, res["skat_state"]), flags
        got[flags], want[flags] = r, res
        tols[flags] = [T.device_tolerance(sp, d, bounds, T.cov_bound(sp, null.w, d, bounds)) for d in res["detail"]]
        for k in range(len(sets)):
            assert abs(r.neglog10p_burden[k] - res["neglog10p_burden"][k]) <= tols[flags][k][1], (flags, k, "burden")
            assert abs(r.neglog10p_skat[k] - res["neglog10p_skat"][k]) <= tols[flags][k][2], (flags, k, "skat")
    rs, ru = got[(1, 1, 1)], got[(0, 0, 1)]
    assert np.array_equal(rs.skat_state, ru.skat_state) and (ru.skat_state == 1).all()
    mu, sinv = handle(mih, codes, (1, 1, 1)).mu_sigma()
    assert np.array_equal(rs.omega * sinv[rs.set_col], ru.omega) or np.allclose(rs.omega * sinv[rs.set_col], ru.omega, rtol=4e-16, atol=0)
    for k in range(len(sets)):
        for name, i in (("neglog10p_burden", 1), ("neglog10p_skat", 2)):
            spec_gap = abs(want[(1, 1, 1)][name][k] - want[(0, 0, 1)][name][k])
            assert spec_gap <= 1e-9 * want[(0, 0, 1)][name][k], (k, name, spec_gap)
            assert abs(getattr(rs, name)[k] - getattr(ru, name)[k]) <= tols[(1, 1, 1)][k][i] + tols[(0, 0, 1)][k][i] + spec_gap, (k, name)
    assert ru.top(3).size == 3 and ru.top(2, by="burden").size == 2
    with pytest.raises(ArgumentError):
        mih.DenseMatrix(np.asfortranarray(rng.standard_normal((n, 5)))).assoc_sets(y, Z, [[0, 1]], d=mih.Bernoulli())


def test_gwas_sets_writes_one_row_per_set(mih, normal_data, tmp_path):
    """The file-level entry beside gwas(): the shipped .bed as a PLINK trio, a set file of three sets -- one around the strongest
    planted SNP -- and the refusal of an id the .bim does not have."""
    n = normal_data["n"]
    y = normal_data["y"]
    prefix = str(tmp_path / "normal")
    shutil.copy(normal_data["bed"], prefix + ".bed")
    p = mih.SnpLinAlg(mih.read_bed(normal_data["bed"], n), n).p
    with open(prefix + ".fam", "w") as f:
        f.writelines(f"{i + 1} 1 0 0 1 {float(y[i])!r}\n" for i in range(n))
    with open(prefix + ".bim", "w") as f:
        f.writelines(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n" for j in range(p))
    setfile = str(tmp_path / "sets.txt")
    groups = {"geneA": range(9410, 9420), "geneB": range(100, 140), "geneC": [5]}
    with open(setfile, "w") as f:
        f.write("# set_id snp_id\n")
        for name, cols in groups.items():
            f.writelines(f"{name} snp{j + 1}\n" for j in reversed(list(cols)))
    out = str(tmp_path / "sets_out.txt")
    cov = os.path.join(FIX, "covariates.txt")
    ids, res = mih.gwas_sets(prefix, mih.Normal, setfile, covariates=cov, outfile=out)
    assert ids == ["geneA", "geneB", "geneC"] and res.set_col[:10].tolist() == list(range(9410, 9420))
    assert res.top(1).tolist() == [0] and res.neglog10p_skat[0] > 20 and res.skat_state.tolist()[2] == 2
    single = mih.gwas(prefix, mih.Normal, covariates=cov, outfile="")
    assert bits(res.assoc.z) == bits(single.z) and bits(res.neglog10p_skat[2]) == bits(single.neglog10p[5])
    lines = open(out).read().splitlines()
    assert len(lines) == 4 and lines[0].split("\t") == ["set_id", "n_snps", "m_used", "burden_z", "neglog10p_burden", "skat_q", "neglog10p_skat", "skat_state"]
    row = lines[1].split("\t")
    assert row[0] == "geneA" and int(row[1]) == 10 and float(row[6]) == res.neglog10p_skat[0]
    with open(setfile, "a") as f:
        f.write("geneD rs_nowhere\n")
    with pytest.raises(ArgumentError, match="rs_nowhere"):
        mih.gwas_sets(prefix, mih.Normal, setfile, covariates=cov, outfile="")
