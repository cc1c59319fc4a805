"""The marginal association scan on the device (csrc/assoc.hip: mih_assoc_score; score_test and assoc of the matrix classes)
against the numpy statement tests/assoc_spec.py.

z, beta and se are held to assoc_spec.bound, a derived bound (its docstring has the derivation): U and b by the bound the
residual-edge tests hold X'r to, Q by the class-sum bound, the rest propagated through V and the square root with the 1 / V and
kappa(G) factors explicit, doubled for numpy's own rounding.  tests/test_assoc_spec_cpu.py asserts the conditions this relies on
for every case: V_j / Q_j >= 1e-3 on the non-degenerate columns and kappa(G) <= 100.  wsum is held to the EXACT class sums of the
quantised weights (Fractions) within one rounding to float64, and to the true weights within (q / 2) count.  Every output is
compared bit for bit between slice_rows 0, 128, 256 and n and with a second call.

The shapes are those where the kernels change path: fewer rows than the 16 of a dword, the 64 of one matrix-core step, the 128
of a tile, several tiles and -- with slice_rows 128 and 256 -- several row slices; one column, the 32 of a column group and its
neighbours, an odd and an even number of groups (the class kernel takes them in pairs); 19 and 20 residuals, the width of one
fused pass."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import assoc_spec as S
import gpu_helpers as H
from conftest import FIX
from test_gpu_hardcall_pack import bed_of

pytestmark = pytest.mark.gpu

BAD_ARG = 2
U = 2.0 ** -53


def bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def handle(mih, codes, flags):
    return mih.SnpLinAlg(bed_of(codes), codes.shape[0], center=bool(flags[0]), scale=bool(flags[1]), impute=bool(flags[2]))


def outputs(r):
    return bits(r.z, r.beta, r.se, r.neglog10p) + (bits(r.wsum) if r.wsum is not None else b"")


def hold(got, sp, tol, what):
    """z, beta, se against the spec within the bound, NaN exactly at the spec's NaN; neglog10p against scipy on the device's own z."""
    t = sp["z"].shape[1]
    rz = S.check(got.z.reshape(-1, t), sp["z"], tol[0], what + ("z",))
    rb = S.check(got.beta.reshape(-1, t), sp["beta"], tol[1], what + ("beta",))
    rs = S.check(got.se, sp["se"], tol[2], what + ("se",))
    want = S.neglog10p(got.z)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got.neglog10p), nan), what
    assert (np.abs(got.neglog10p - want)[~nan] <= 1e-14 * want[~nan] + 1e-15).all(), what
    return max(rz, rb, rs)


# ---- 1. edge shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", S.EDGE_P)
def test_edge_shapes(mih, p):
    cases = [c for c in S.edge_cases() if c[1] == p]
    assert len(cases) == len(S.EDGE_N)
    worst = 0.0
    for case in cases:
        n, p, t, c, missing, flags, wk, seed = case
        codes, A, w, Z = S.edge_inputs(case)
        x = handle(mih, codes, flags)
        v = np.random.default_rng(seed).standard_normal(n)
        before = x.xtv(v)
        sp = S.score(codes, flags, A, w, Z)
        tol = S.bound(sp, codes, flags, A, w, Z)
        got = x.score_test(A, w, Z, wsum=True)
        assert np.array_equal(np.isnan(got.z.reshape(p, -1)[:, 0]), sp["deg"]), case          # NaN exactly at the degenerate columns
        worst = max(worst, hold(got, sp, tol, case))
        # the class sums
        cnt = np.stack([(codes == g).sum(axis=0) for g in (1, 2, -1)], axis=1)
        if w is None:
            assert np.array_equal(got.wsum, cnt.astype(np.float64)), case
        else:
            exact = S.class_sums_quantised(codes, w)
            true = S.class_sums(codes, w)
            q = S.quantum(w)
            for k in range(3):
                for j in range(p):
                    e = exact[k + 1][j]
                    assert abs(Fraction(float(got.wsum[j, k])) - e) <= e * Fraction(1, 2 ** 53), (case, j, k)      # one rounding
                    assert abs(got.wsum[j, k] - true[k + 1, j]) <= q / 2 * cnt[j, k] + 2 * U * true[k + 1, j], (case, j, k)
        if wk == "ones":                                              # unit weights given as numbers: the counts again, within the bound
            none = x.score_test(A, None, Z, wsum=True)
            assert np.array_equal(none.wsum, got.wsum), case
            hold(none, sp, tol, case + ("None",))
        # bits: the row slices, a second call, and the handle is only read
        first = outputs(got)
        for sr in (0, 128, 256, n):
            assert outputs(x.score_test(A, w, Z, slice_rows=sr, wsum=True)) == first, (case, sr)
        assert bits(x.xtv(v)) == bits(before), case
    print(f"assoc p={p}: max err / bound = {worst:.3g}")


# ---- 2. the slice rule ----------------------------------------------------------------------------------------------------------------
def test_more_rows_than_one_f32_accumulator_may_cover(mih):
    """n = 5 592 406, p = 32, the smallest n at which a column exists that an unsliced f32 accumulator provably gets wrong.  An
    accumulator of the class kernel holds a digit sum in quarters: a row adds the digit u in {0..3} for dosage 1 (u quarters) and
    2 u for dosage 2.  f32 holds every integer up to 2^24 and only even ones up to 2^25, so a dosage-1 accumulator fails as soon as
    an ODD total above 2^24 is possible: n rows reach at most 3 n (3 n - 1 if that is even), and 3 n - 1 >= 2^24 + 1 first at
    n = 5 592 406 (3 x 5 592 405 = 16 777 215 < 2^24); a dosage-2 accumulator adds even numbers up to 6, fails at a total = 2 mod 4
    above 2^25, and 6 n - 2 = 33 554 434 is the first such at the same n.
    Weights: R_i = 2^54 - 2 (w = 1 - 2^-53: every base-4 digit above the lowest is 3) except one row with R = 2^54 - 6 (digit 1 is
    2).  Column 0 is all dosage 1: its digit-1 sum is 3 n - 1 = 16 777 217.  Column 1 is all dosage 2: 6 n - 2.  The other columns
    repeat four 1024-row patterns.  The class sums must be the exact integers rounded once, for slice_rows at the limit, above it
    (taken as the limit), and 0 (the library's rule), with the same bits of every output."""
    n, p, odd = 5592406, 32, 4097
    assert float(np.float32(3 * (n - 1))) == 3 * (n - 1) and float(np.float32(3 * n - 1)) != 3 * n - 1
    assert float(np.float32(6 * n - 2)) != 6 * n - 2 and 3 * n - 1 > 2 ** 24 and 6 * n - 2 > 2 ** 25
    rng = np.random.default_rng(77)
    stride = (n + 3) // 4
    pats = rng.integers(0, 256, size=(4, 256), dtype=np.uint8)
    pats[(pats & 3) == 1] ^= 1; pats[((pats >> 2) & 3) == 1] ^= 4; pats[((pats >> 4) & 3) == 1] ^= 16; pats[((pats >> 6) & 3) == 1] ^= 64   # no missing code
    bed = np.empty((p, stride), dtype=np.uint8)
    bed[0], bed[1] = 0xAA, 0xFF                                    # .bed code 10: one copy, 11: two copies
    for j in range(2, p):
        bed[j] = np.resize(pats[j % 4], stride)
    bed[:, -1] &= (1 << (2 * (n - 4 * (stride - 1)))) - 1          # the pad rows of the last byte
    x = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    w = np.full(n, 1.0 - 2.0 ** -53)
    w[odd] = 1.0 - 3 * 2.0 ** -53
    R, Rodd = 2 ** 54 - 2, 2 ** 54 - 6
    assert S.quantum(w) == 2.0 ** -54 and int(w[0] * 2.0 ** 54) == R and int(w[odd] * 2.0 ** 54) == Rodd
    want = np.empty((p, 3))
    seen = {}
    for j in range(p):
        key = j if j < 2 else 2 + j % 4
        if key not in seen:
            col = np.array([0, -1, 1, 2], dtype=np.int8)[np.stack([(bed[j] >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)[:n]]
            seen[key] = [float(Fraction(R * int((col == g).sum()) - (R - Rodd if col[odd] == g else 0), 2 ** 54)) for g in (1, 2, -1)]
        want[j] = seen[key]
    assert want[0, 0] > 0 and want[1, 1] > 0 and (want[:, 2] == 0).all()
    A = np.random.default_rng(78).standard_normal(n)
    first = None
    for sr in (S.SLICE_ROWS_LIMIT, S.SLICE_ROWS_LIMIT + 128, 1 << 23, 0):
        got = x.score_test(A, w, None, slice_rows=sr, wsum=True)
        assert np.array_equal(got.wsum, want), (sr, np.argwhere(got.wsum != want)[:4].tolist())
        assert np.isnan(got.z[:2]).all() and np.isfinite(got.z[2:]).all(), sr           # two monomorphic columns
        first = outputs(got) if first is None else first
        assert outputs(got) == first, sr


# ---- 3. dosage and dense handles ----------------------------------------------------------------------------------------------------------
def _aux(n, t, c, seed, weighted):
    rng = np.random.default_rng(seed)
    Z = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1)
    w = rng.uniform(0.05, 0.25, n) if weighted else None
    A = rng.standard_normal((n, t))
    wz = Z if w is None else w[:, None] * Z
    return A - wz @ np.linalg.solve(Z.T @ wz, Z.T @ A), w, Z


@pytest.mark.parametrize("shape", [(17, 20, 1, 1, False), (129, 20, 2, 3, True), (1025, 20, 1, 19, True)])
def test_dosage_handles(mih, shape):
    n, p, t, c, weighted = shape
    den = 255
    num = H.edge_matrix(n, den, 40 + n)
    mun, sc, _, _ = H.dosage_host_stats(num, den)
    X = np.where(num == 0xFFFF, 0.0, (num.astype(np.float64) - mun[None, :]) * sc[None, :])
    keep = np.flatnonzero((np.abs(X) > 0).sum(axis=0) > max(3, n // 20))             # the near-constant columns of edge_matrix have V / Q ~ 0
    A, w, Z = _aux(n, t, c, 50 + n, weighted)
    sp = S.score_dense(X, A, w, Z)
    ok = keep[sp["V"][keep] / sp["Q"][keep] >= S.MIN_V_OVER_Q]
    assert ok.size >= 8
    tol = S.bound(sp, None, None, A, w, Z)
    got = mih.DosageMatrix(num, den).score_test(A, w, Z, wsum=True)
    assert np.isnan(got.wsum).all()
    for g, s_, b in ((got.z.reshape(p, -1), sp["z"], tol[0]), (got.beta.reshape(p, -1), sp["beta"], tol[1]), (got.se, sp["se"], tol[2])):
        r = S.check(g[ok], s_[ok], b[ok], shape)
        print(f"dosage {shape}: max err / bound = {r:.3g}")
    again = mih.DosageMatrix(num, den).score_test(A, w, Z, slice_rows=128)
    assert bits(again.z, again.beta, again.se) == bits(got.z, got.beta, got.se)


@pytest.mark.parametrize("shape", [(15, 7, 1, 1, False), (257, 33, 3, 5, True), (1000, 40, 1, 18, True)])
def test_dense_handles(mih, shape):
    n, p, t, c, weighted = shape
    X = np.random.default_rng(60 + n).standard_normal((n, p))
    A, w, Z = _aux(n, t, c, 70 + n, weighted)
    sp = S.score_dense(X, A, w, Z)
    assert (sp["V"] / sp["Q"]).min() >= S.MIN_V_OVER_Q
    tol = S.bound(sp, None, None, A, w, Z)
    for dt in (np.float64, np.float32):
        Xd = X.astype(dt)
        spd = sp if dt is np.float64 else S.score_dense(Xd.astype(np.float64), A, w, Z)
        told = tol if dt is np.float64 else S.bound(spd, None, None, A, w, Z)
        got = mih.DenseMatrix(Xd).score_test(A, w, Z)
        r = hold(got, spd, told, shape + (dt.__name__,))
        print(f"dense {shape} {dt.__name__}: max err / bound = {r:.3g}")


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped(mih, normal_data):
    n = normal_data["n"]
    bed = mih.read_bed(normal_data["bed"], n)
    two = np.stack([(np.asarray(bed) >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n]
    codes = np.array([0, -1, 1, 2], dtype=np.int64)[two].T.copy()
    z = np.loadtxt(os.path.join(FIX, "covariates.txt"), delimiter=",")
    return mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True), codes, normal_data["y"], z


def test_assoc_normal_finds_the_planted_snps_of_the_shipped_example(mih, shipped):
    x, codes, y, z = shipped
    res = x.assoc(y, z)
    assert res.top(7).tolist() == [9414, 4716, 8374, 6289, 7754, 4245, 3136]
    null = res.null
    A = (y - null.mu) / math.sqrt(null.phi)
    sp = S.score(codes, (1, 1, 1), A, None, z)
    tol = S.bound(sp, codes, (1, 1, 1), A, None, z)
    r = S.check(res.z[:, None], sp["z"], tol[0], "z")
    print(f"assoc Normal: max err / bound = {r:.3g}")
    rt = math.sqrt(null.phi)                       # the mirror's dispersion scaling: beta and se of the unit-weight call times sqrt(phi)
    S.check(res.beta[:, None], sp["beta"] * rt, tol[1] * rt * (1 + 4 * U) + 2 * U * np.abs(sp["beta"] * rt), "beta")
    S.check(res.se, sp["se"] * rt, tol[2] * rt * (1 + 4 * U) + 2 * U * sp["se"] * rt, "se")
    assert abs(res.z[9414] ** 2 - 554.82227036049) < 1e-6
    two = x.assoc(np.stack([y, -2.0 * y + 1.0], axis=1), z)          # two traits share the pass and the weights
    assert bits(two.z[:, 0]) == bits(res.z) and np.allclose(two.z[:, 1], -res.z, rtol=1e-9, atol=1e-9)
    assert np.allclose(two.beta[:, 1], -2.0 * res.beta, rtol=1e-9, atol=1e-12) and np.allclose(two.se[:, 1], 2.0 * res.se, rtol=1e-9)


def test_assoc_bernoulli_on_the_shipped_example(mih, shipped):
    x, codes, y, z = shipped
    yb = (y > np.median(y)).astype(np.float64)
    res = x.assoc(yb, z, d=mih.Bernoulli())
    null = res.null
    assert null.converged and null.phi == 1.0
    sp = S.score(codes, (1, 1, 1), null.A, null.w, z)
    tol = S.bound(sp, codes, (1, 1, 1), null.A, null.w, z)
    t = sp["z"].shape[1]
    r = max(S.check(res.z.reshape(-1, t), sp["z"], tol[0], "z"), S.check(res.beta.reshape(-1, t), sp["beta"], tol[1], "beta"),
            S.check(res.se, sp["se"], tol[2], "se"))
    print(f"assoc Bernoulli: max err / bound = {r:.3g}")
    assert set(res.top(3).tolist()) <= {9414, 4716, 8374, 6289, 7754, 4245, 3136}


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(mih):
    n, p = 129, 33
    codes, A, w, Z = S.edge_inputs((n, p, 1, 2, 0.03, (1, 1, 1), "logistic", 4242))
    x = handle(mih, codes, (1, 1, 1))
    L = mih.lib()
    A, Z = np.asfortranarray(A), np.asfortranarray(Z)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(h=None, A_=A, t=1, w_=w, Z_=Z, c=2, sr=0, null_out=None):
        out = [np.full(p, 7.0) for _ in range(4)] + [np.full(3 * p, 7.0)]
        ps = [ptr(o) for o in out]
        if null_out is not None:
            ps[null_out] = None
        rc = L.mih_assoc_score(x._h if h is None else h, ptr(A_), t, ptr(w_), ptr(Z_), c, sr, *ps)
        assert all((o == 7.0).all() for o in out), "outputs written"
        return rc

    def bad(v, i, val):
        b = np.array(v, order="F", copy=True)
        b.reshape(-1, order="F")[i] = val
        return b
    assert call(h=C.c_void_p(None)) == BAD_ARG
    for k in range(4):
        assert call(null_out=k) == BAD_ARG, k
    for t in (0, -1, 33):
        assert call(t=t) == BAD_ARG, t
    for c in (0, -1, 65):
        assert call(c=c) == BAD_ARG, c
    assert call(w_=bad(w, 5, np.nan)) == BAD_ARG and call(w_=bad(w, 5, -1e-300)) == BAD_ARG and call(w_=bad(w, 128, np.inf)) == BAD_ARG
    assert call(A_=bad(A, 3, np.inf)) == BAD_ARG and call(A_=bad(A, 128, np.nan)) == BAD_ARG
    assert call(Z_=bad(Z, n + 1, np.nan)) == BAD_ARG and call(Z_=bad(Z, 0, -np.inf)) == BAD_ARG
    Zdep = np.asfortranarray(np.stack([Z[:, 0], 0.0 * Z[:, 0]], axis=1))          # a zero pivot: Z'WZ is not positive definite
    assert call(Z_=Zdep) == BAD_ARG
    assert call(w_=np.zeros(n)) == BAD_ARG                                         # G = 0
    assert call(sr=-1) == BAD_ARG
    buf = C.create_string_buffer(512)
    L.mih_last_error(buf, 512)
    assert b"slice_rows" in buf.value
    out = [np.full(p, 7.0) for _ in range(4)]
    assert L.mih_assoc_score(x._h, ptr(A), 1, ptr(w), ptr(Z), 2, 0, *[ptr(o) for o in out], None) == 0             # wsum may be NULL
    assert not any((o == 7.0).any() for o in out[:3])


def test_gwas_writes_one_row_per_snp(mih, shipped, normal_data, tmp_path):
    """The file-level entry beside iht(): a PLINK trio made of the shipped .bed, the phenotype in .fam column 6, the covariate file."""
    import shutil
    x, codes, y, z = shipped
    n, p = normal_data["n"], x.p
    prefix = str(tmp_path / "normal")
    shutil.copy(normal_data["bed"], prefix + ".bed")
    with open(prefix + ".fam", "w") as f:
        f.writelines(f"{i + 1} 1 0 0 1 {float(y[i])!r}\n" for i in range(n))
    with open(prefix + ".bim", "w") as f:
        f.writelines(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n" for j in range(p))
    out = str(tmp_path / "gwas.txt")
    res = mih.gwas(prefix, mih.Normal, covariates=os.path.join(FIX, "covariates.txt"), outfile=out)
    assert res.top(7).tolist() == [9414, 4716, 8374, 6289, 7754, 4245, 3136]
    ref = x.assoc(y, normal_data["z"])                           # (the standardized covariates: what parse_covariates makes of the file)
    assert np.allclose(res.z, ref.z, rtol=1e-9, atol=1e-9, equal_nan=True)
    lines = open(out).read().splitlines()
    assert len(lines) == p + 1 and lines[0].split("\t") == ["chr", "pos", "SNPid", "ref", "alt", "z", "beta", "se", "neglog10p"]
    row = lines[9415].split("\t")
    assert row[2] == "snp9415" and float(row[5]) == res.z[9414] and float(row[8]) == res.neglog10p[9414] and float(row[8]) > 100
