"""Linear solves with V = tau_e I + tau_g Phi on the device (csrc/lmm.hip: mih_grm_solve; kinship_solve() of SnpLinAlg and
DosageMatrix) against the numpy statement tests/lmm_spec.py.

Inputs: the planted generator of pca_spec (Phi has spread eigenvalues) with p = 400 columns at the sample counts where the
kernels change path -- 1, 17 around a matrix-core block, 127 / 129 around a tile, 257 = three tiles, 513 past the 512-row slab --
and the column counts where k_lmm_vmul<IB, NB> switches (16 / 17, 33, 65) and the most (128).  Every check runs on all columns,
on a column mask and with method="Robust".

Bounds, derived and not measured (lmm_spec states them): V_s = tau_e I + tau_g Phi_s from grm_spec.grm on the handle's own
mu_sigma(), E = grm_spec.bound, u = 2^-53.
    residual   |b - V_s x|_2 <= reported + (tau_g |E|_F + 8 (n + m) u |V_s|_F) |x|_2
    converged  reported <= tol |b|_2 + iters u ((2 n + 6) |V_s|_F Theta + |b|_2) + (n + 4) u (|V_s|_F |x|_2 + |b|_2)
Bit for bit: a column does not depend on the other columns of the block, on panel_cols or on the call."""
import ctypes as C

import numpy as np
import pytest

import grm_spec as K
import lmm_spec as L
import pca_spec as P
from conftest import free_device_bytes
from test_gpu_hardcall_pack import from_bed, numerators

from mendeliht_amd import api

pytestmark = pytest.mark.gpu

BAD_ARG = 2
TE, TG = L.TAU


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_bits(a, b):
    return bits(a.x) == bits(b.x) and bits(a.residuals) == bits(b.residuals) and np.array_equal(a.iters, b.iters) and np.array_equal(a.converged, b.converged)


def column(res, j):
    """Column j of a result, as a solve of that column alone returns it."""
    return api.SolveResult(res.x[:, j], res.iters[j:j + 1], res.converged[j:j + 1], res.residuals[j:j + 1])


class Spec:
    """Everything the bounds need of one (handle, genotypes, column selection, method), computed once."""

    def __init__(self, h, g, method, cols=None):
        mu, sinv = h.mu_sigma()
        self.n = g.shape[0]
        self.phi = K.grm(g, mu, sinv, cols, method)
        self.e_fro = float(np.linalg.norm(K.bound(g, mu, sinv, cols, method)))
        self.v = L.vmat(self.phi, TE, TG)
        self.v_fro = float(np.linalg.norm(self.v))

    def check(self, res, B, what, tol=L.TOL, max_iter=500):
        n, m = B.shape
        assert res.x.shape == (n, m) and res.iters.shape == res.converged.shape == res.residuals.shape == (m,), what
        assert np.all(np.isfinite(res.x)) and np.all(np.isfinite(res.residuals)), what
        xs, its, convs, _, theta = L.pcg(self.phi, B, TE, TG, tol, max_iter)
        rho = np.linalg.norm(B - self.v @ res.x, axis=0)
        xn, bn = np.linalg.norm(res.x, axis=0), np.linalg.norm(B, axis=0)
        rb = L.residual_bound(res.residuals, TG, self.e_fro, self.v_fro, n, m, xn)
        assert np.all(rho <= rb), (what, rho, rb)
        cb = tol * bn + L.gap_bound(res.iters, n, self.v_fro, np.maximum(theta, xn), bn) + L.eval_bound(n, self.v_fro, xn, bn)
        conv = res.converged
        print(what, "iters", int(res.iters.max()), "spec", int(its.max()), "residual / (tol |b|)",
              float((res.residuals[bn > 0] / (tol * bn[bn > 0])).max()) if tol > 0 and np.any(bn > 0) else 0.0)
        assert np.all(res.residuals[conv] <= cb[conv]), (what, res.residuals, cb)
        assert np.all(res.iters[~conv] == max_iter) and np.all(res.iters <= max_iter), what
        return rho


def variants(p):
    every = np.ones(p, dtype=bool)
    return (("GRM", every), ("GRM", np.arange(p) % 3 != 1), ("Robust", every))


# ---- 1. the edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", L.SOLVE_N)
def test_solve_at_the_edge_shapes(mih, n):
    p = L.SOLVE_P
    codes = P.planted(n, p, 3)
    x = from_bed(mih, codes)
    g = K.genotypes(codes)
    r = np.random.default_rng(n).standard_normal(n)
    before = x.xtv(r)
    for method, cols in variants(p):
        spec = Spec(x, g, method, cols)
        got = {}
        for m in L.SOLVE_M:
            B = L.rhs(n, m)
            got[m] = x.kinship_solve(B, TE, TG, method=method, cols=cols)
            assert got[m].converged.all(), (n, m, method)
            spec.check(got[m], B, (n, m, method, int(cols.sum())))
        # bit for bit: a column of m = 128 (33) is the solve of that column alone -- the first, a middle and the last block
        # of 16 -- whatever the panels, and on a second call
        for m, js in ((128, (5, 70, 127)), (33, (0, 20, 32))):
            B = L.rhs(n, m)
            for j in js:
                assert same_bits(column(got[m], j), x.kinship_solve(B[:, j:j + 1], TE, TG, method=method, cols=cols)), (n, m, j, method)
        for pc in (0, 4, 64):
            assert same_bits(got[17], x.kinship_solve(L.rhs(n, 17), TE, TG, method=method, cols=cols, panel_cols=pc)), (n, pc, method)
        # ... and whatever the width of the block: the first 16 columns of the 65, solved through another <IB, NB>
        B = L.rhs(n, 65)
        narrow = x.kinship_solve(B[:, :16], TE, TG, method=method, cols=cols)
        for j in (0, 15):
            assert same_bits(column(narrow, j), column(got[65], j)), (n, j, method)
    assert bits(x.xtv(r)) == bits(before), n                         # the source is only read


@pytest.fixture(scope="module")
def wide(mih):
    n, p = 257, L.SOLVE_P
    codes = P.planted(n, p, 3)
    x = from_bed(mih, codes)
    every = np.ones(p, dtype=bool)
    spec = Spec(x, K.genotypes(codes), "GRM", every)
    spec.v.setflags(write=False)
    return codes, x, spec, every


def test_zero_and_proportional_columns(mih, wide):
    codes, x, spec, every = wide
    n = 257
    B = L.rhs(n, 20)
    B[:, 3] = 0.0                                                    # a zero column among live ones
    B[:, 18] = 0.0                                                   # ... and one in the second block of 16
    B[:, 7] = -2.5 * B[:, 2]                                         # a multiple of another
    res = x.kinship_solve(B, TE, TG, cols=every)
    spec.check(res, B, "zero, multiple")
    for j in (3, 18):
        assert np.all(res.x[:, j] == 0.0) and res.iters[j] == 0 and res.converged[j] and res.residuals[j] == 0.0
    assert res.converged.all() and np.all(res.iters[[0, 2, 7]] > 0)
    # the multiple: its solution is the multiple to rounding only (nothing bit for bit).  V (x_7 + 2.5 x_2) is the sum of the
    # two residuals and of the rounding of -2.5 b_2, all with the device's V, whose least eigenvalue is within tau_g |E|_F of
    # the spec's
    diff = np.linalg.norm(res.x[:, 7] + 2.5 * res.x[:, 2])
    xn, bn = np.linalg.norm(res.x[:, 7]), np.linalg.norm(B[:, 7])
    lam_min = np.linalg.eigvalsh(spec.v)[0] - TG * spec.e_fro
    assert diff <= (res.residuals[7] + 2.5 * res.residuals[2] + 2 * L.eval_bound(n, spec.v_fro, xn, bn) + 2 * L.U * bn) / lam_min
    # every column zero: no iteration at all
    none = x.kinship_solve(np.zeros((n, 5)), TE, TG, cols=every)
    assert np.all(none.x == 0.0) and np.all(none.iters == 0) and none.converged.all() and np.all(none.residuals == 0.0)
    # the live columns are those of a block without the zero ones
    alone = x.kinship_solve(B[:, [0, 2]], TE, TG, cols=every)
    assert same_bits(column(alone, 0), column(res, 0)) and same_bits(column(alone, 1), column(res, 2))


def test_max_iter_tol_and_vector_arguments(mih, wide):
    codes, x, spec, every = wide
    n = 257
    B = L.rhs(n, 17)
    one = x.kinship_solve(B, TE, TG, cols=every, max_iter=1)
    assert not one.converged.any() and np.all(one.iters == 1) and np.all(np.isfinite(one.x)) and np.all(np.isfinite(one.residuals))
    spec.check(one, B, "max_iter=1", max_iter=1)
    assert np.all(one.residuals > L.TOL * np.linalg.norm(B, axis=0))
    full = x.kinship_solve(B, TE, TG, cols=every)
    loose = x.kinship_solve(B, TE, TG, cols=every, tol=1e-3)
    assert loose.converged.all() and loose.iters.max() < full.iters.max()
    spec.check(loose, B, "tol=1e-3", tol=1e-3)
    # tol = 0 cannot be met short of an exact zero residual: max_iter iterations, finite, as good as a converged run
    zero = x.kinship_solve(B, TE, TG, cols=every, tol=0.0, max_iter=60)
    assert np.all(zero.iters[~zero.converged] == 60) and np.all(np.isfinite(zero.x))
    assert np.all(np.linalg.norm(B - spec.v @ zero.x, axis=0) <= L.residual_bound(zero.residuals, TG, spec.e_fro, spec.v_fro, n, 17, np.linalg.norm(zero.x, axis=0)))
    # tau_g = 0: V = tau_e I, the preconditioner is the inverse -- one iteration, alpha = r'z / p'Vp the quotient of two sums of
    # the same n positive terms in two orders, so within 2 (n + 1) u of 1
    flat = x.kinship_solve(B, 2.0, 0.0, cols=every)
    assert flat.converged.all() and np.all(flat.iters == 1) and np.all(np.abs(flat.x - B / 2.0) <= 4 * (n + 2) * L.U * np.abs(B / 2.0))
    # a vector gives a vector; the default minmaf rule is grm()'s; method by number
    v = x.kinship_solve(B[:, 4], TE, TG, cols=every)
    assert v.x.shape == (n,) and bits(v.x) == bits(full.x[:, 4]) and v.iters.shape == (1,)
    with np.errstate(invalid="ignore"):
        keep = x._allele_maf() >= 0.01
    assert same_bits(x.kinship_solve(B, TE, TG), x.kinship_solve(B, TE, TG, cols=keep))
    assert same_bits(x.kinship_solve(B, TE, TG, method=1, cols=every), x.kinship_solve(B, TE, TG, method="Robust", cols=every))
    # against the reference solve: |x - V_s^-1 b| <= |b - V_s x| / lambda_min(V_s)
    err = np.linalg.norm(full.x - L.dense(spec.phi, B, TE, TG), axis=0)
    rho = np.linalg.norm(B - spec.v @ full.x, axis=0)
    assert np.all(err <= (rho + 8 * n * L.U * spec.v_fro * np.linalg.norm(full.x, axis=0)) / np.linalg.eigvalsh(spec.v)[0])


def test_dosage_matrix_of_the_same_hard_calls(mih):
    n, p = 129, 150
    codes = P.planted(n, p, 3)
    d = mih.DosageMatrix(numerators(codes, unit=1), 2)
    g = K.genotypes(codes) / 2.0
    every = np.ones(p, dtype=bool)
    B = L.rhs(n, 33)
    for method in K.METHODS:
        spec = Spec(d, g, method, every)
        res = d.kinship_solve(B, TE, TG, method=method, cols=every)
        assert res.converged.all()
        spec.check(res, B, (method, "dosage"))
        assert same_bits(res, d.kinship_solve(B, TE, TG, method=method, cols=every, panel_cols=4))
        assert same_bits(column(res, 32), d.kinship_solve(B[:, 32:], TE, TG, method=method, cols=every))


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------
def last_error(mih):
    buf = C.create_string_buffer(512)
    mih.lib().mih_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def test_refusals_leave_the_outputs_untouched(mih):
    lib = mih.lib()
    n, p = 17, 33
    codes = P.planted(n, p, 2)
    x = from_bed(mih, codes)
    dense = mih.DenseMatrix(np.random.default_rng(0).standard_normal((n, 5)))
    B = np.ascontiguousarray(L.rhs(n, 3).T)
    X, res = np.full(n * 130, -7.0), np.full(130, -7.0)
    it, conv = np.full(130, -7, dtype=np.int32), np.full(130, -7, dtype=np.int32)
    none = np.zeros(p, dtype=np.uint8)
    before = free_device_bytes()

    def call(h=None, ck=None, method=0, te=TE, tg=TG, m=3, tol=L.TOL, max_iter=500, out=None):
        o = [a.ctypes.data_as(C.c_void_p) for a in (B, X, it, conv, res)]
        if out is not None:
            o[out] = None
        return lib.mih_grm_solve(x._h if h is None else h, None if ck is None else ck.ctypes.data_as(C.c_void_p), method, 0, te, tg, o[0], m,
                                 tol, max_iter, o[1], o[2], o[3], o[4])

    nan, inf = float("nan"), float("inf")
    cases = [("dense", dict(h=dense._h)), ("empty", dict(ck=none)), ("method", dict(method=7)), ("m0", dict(m=0)), ("m<0", dict(m=-1)),
             ("m>128", dict(m=129)), ("tau_e 0", dict(te=0.0)), ("tau_e<0", dict(te=-1.0)), ("tau_e nan", dict(te=nan)),
             ("tau_e inf", dict(te=inf)), ("tau_g<0", dict(tg=-1e-9)), ("tau_g nan", dict(tg=nan)), ("tau_g inf", dict(tg=inf)),
             ("tol nan", dict(tol=nan)), ("tol inf", dict(tol=inf)), ("tol<0", dict(tol=-1.0)), ("max_iter", dict(max_iter=0))]
    cases += [(f"null {i}", dict(out=i)) for i in range(5)]
    for what, kw in cases:
        assert call(**kw) == BAD_ARG and last_error(mih), what
        assert np.all(X == -7.0) and np.all(res == -7.0) and np.all(it == -7) and np.all(conv == -7), what
    assert abs(free_device_bytes() - before) <= 64 << 20
    for kw in (dict(tau_e=0.0), dict(tau_g=-1.0), dict(tol=nan), dict(max_iter=0), dict(method="MoM"), dict(cols=np.zeros(p, dtype=bool)),
               dict(B=np.zeros((n, 129))), dict(B=np.zeros((n, 0))), dict(B=np.zeros(n + 1)), dict(B=np.zeros((n, 2, 2)))):
        with pytest.raises(api.ArgumentError):
            x.kinship_solve(**{"B": B.T, "tau_e": TE, "tau_g": TG, **kw})
    assert not hasattr(mih.DenseMatrix, "kinship_solve")
    assert call() == 0 and np.all(conv[:3] == 1) and np.all(it[:3] >= 1)                 # and the handle still serves, m = 3 of room for 130
    assert np.all(X[3 * n:] == -7.0) and np.all(res[3:] == -7.0) and np.all(it[3:] == -7) and np.all(conv[3:] == -7)
    assert bits(X[:3 * n].reshape(3, n).T) == bits(x.kinship_solve(B.T, TE, TG, cols=np.ones(p, dtype=bool)).x)      # n x m, column-major


def test_a_matrix_the_device_cannot_hold_is_refused_before_anything_is_allocated(mih):
    import re
    x = mih.SnpLinAlg.synthetic(300_000, 32)
    before = free_device_bytes()
    with pytest.raises(MemoryError) as e:
        x.kinship_solve(np.ones((300_000, 20)), 1.0, 1.0)
    need, free = (int(v) for v in re.findall(r"(\d{9,}) bytes", str(e.value)))
    assert need >= 8 * 300_032 ** 2 + 6 * 8 * 300_032 * 32 and need > free and abs(free - before) <= 64 << 20
    assert abs(free_device_bytes() - before) <= 64 << 20


# ---- 3. the REML null model (mih_lmm_null; lmm_null() and assoc(kinship=...)) ----------------------------------------------------------
"""Inputs: the planted generator at p = 2000, n in {129, 300, 513}, c in {1, 3} covariates, sigma_g^2 = sigma_e^2 = 1, the
phenotype of lmm_spec.phenotype so that Cov(y) = sigma_g^2 Phi + sigma_e^2 I exactly.  tests/test_lmm_spec_cpu.py asserts, from
the spec alone, that every one of them converges inside max_iter in the interior with kappa(V) <= 1e3 and that its last two
changes of tau are clear of tol.

Tolerance, measured from the spec alone and not from the device: for every compared quantity q (the iterates of tau, alpha, Py,
the traces, gamma, the ratios) rel(q) = max |q_pcg - q_dense| / max |q_dense| between the spec's PCG form at cg_tol and its
dense-solve form; D = the largest rel(q) of the case.  The device must be within 3 D of the PCG form in every quantity, in the
same relative measure: it differs from the PCG form by the order of its sums and by at most one CG iteration at the stopping
threshold per solve."""
NULL_P = 2000
NULL_CASES = [(129, 1), (129, 3), (300, 1), (300, 3), (513, 1), (513, 3)]
QUANTITIES = ("path", "alpha", "py", "trace", "gamma", "ratios")
_cases = {}


def mean_imputed(codes, cols):
    g = K.genotypes(codes[:, cols])
    return np.where(np.isnan(g), np.nanmean(g, axis=0)[None, :], g)


def null_case(mih, n, c, noise=False, seed=None):
    """(handle, codes, phi_s, y, Z, marker columns, G) of one case, made once."""
    key = (n, c, noise, seed)
    if key not in _cases:
        codes = P.planted(n, NULL_P, 3)
        x = from_bed(mih, codes)
        mu, sinv = x.mu_sigma()
        a, div = K.operand(K.genotypes(codes), mu, sinv, None, "GRM")
        phi = (a @ a.T) / div
        phi.setflags(write=False)
        Z = L.covariates(n, c, n + c if seed is None else seed)
        y = L.phenotype(a * np.sqrt(a.shape[1] / div), Z, np.arange(1, c + 1, dtype=float), 0.0 if noise else 1.0, 1.0, n + c if seed is None else seed)
        mk = x.lmm_markers()
        _cases[key] = (x, codes, phi, y, Z, mk, mean_imputed(codes, mk))
    return _cases[key]


def quantities(f):
    return {"path": np.asarray(f.path if hasattr(f, "path") else f.tau_path), "alpha": np.asarray(f.alpha), "py": np.asarray(f.py if hasattr(f, "py") else f.Py),
            "trace": np.asarray(f.trace), "gamma": np.asarray([f.gamma]), "ratios": np.asarray(f.ratios)}


@pytest.mark.parametrize("case", NULL_CASES, ids=lambda s: "-".join(map(str, s)))
def test_null_model_against_the_spec(mih, case):
    n, c = case
    x, codes, phi, y, Z, mk, G = null_case(mih, n, c)
    every = np.ones(NULL_P, dtype=bool)
    null = x.lmm_null(y, Z, cols=every)
    assert np.array_equal(x._marker_genotypes(mk), G) and np.array_equal(null.marker_cols, mk) and len(mk) == 30
    fp = L.reml(phi, y, Z, G=G, solver="pcg")
    fd = L.reml(phi, y, Z, G=G, solver="dense")
    assert fd.state == 1 and fp.state == 1 and fp.iters == fd.iters
    assert null.iters == fp.iters and null.state == fp.state, (null.iters, null.state, fp.iters, fp.state)
    qp, qd, qg = quantities(fp), quantities(fd), quantities(null)
    scale = {k: float(np.max(np.abs(qd[k]))) for k in QUANTITIES}
    rel = {k: float(np.max(np.abs(qp[k] - qd[k]))) / scale[k] for k in QUANTITIES}
    D = max(rel.values())
    dev = {k: float(np.max(np.abs(qg[k] - qp[k]))) / scale[k] for k in QUANTITIES}
    print(case, "iters", null.iters, "cg", null.cg_iters, "spec cg", fp.cg_iters, "tau", null.tau, "h2", null.h2, "gamma", null.gamma, "cv", null.ratio_cv)
    print("   spec pcg - dense (relative):", {k: f"{v:.2e}" for k, v in rel.items()}, "D", f"{D:.2e}")
    print("   device - spec pcg (relative):", {k: f"{v:.2e}" for k, v in dev.items()}, "share of 3 D", f"{max(dev.values()) / (3 * D):.3f}")
    for k in QUANTITIES:
        assert qg[k].shape == qp[k].shape and dev[k] <= 3.0 * D, (case, k, dev[k], D)
    # every solve converged: cg_tol = 1e-10 plus the recurrence gap, which lmm_spec.gap_bound puts below 6e-10 |b| at these sizes
    assert null.worst_residual <= 1e-10 + 6e-10 and abs(null.h2 - fp.h2) <= 3.0 * D and null.dbar == pytest.approx(fp.dbar, rel=1e-12)
    # bit for bit: a second call, and the panels
    for pc in (0, 64):
        again = x.lmm_null(y, Z, cols=every, panel_cols=pc)
        assert all(bits(a) == bits(b) for a, b in zip(quantities(null).values(), quantities(again).values())), (case, pc)
        assert (again.iters, again.state, again.cg_iters, again.worst_residual) == (null.iters, null.state, null.cg_iters, null.worst_residual)


def test_null_model_on_the_boundary(mih):
    """y is pure noise (seed 0 reaches the boundary rule in the dense-solve spec: test_lmm_spec_cpu.py): state 2, tau_g = 0, tau_e
    the OLS value, and the scan is the plain one up to the host's operations -- Py = e0 / s2 and gamma = 1 / s2 make z / sqrt(gamma)
    the z of A = e0 / sqrt(s2), which is what assoc() without kinship hands to the score test.  The solves at tau_g = 0 take
    one iteration and leave rounding only; the comparison allows cg_tol = 1e-10, what the solves are asked for."""
    n, c = 300, 1
    x, codes, phi, y, Z, mk, G = null_case(mih, n, c, noise=True, seed=0)
    every = np.ones(NULL_P, dtype=bool)
    fd = L.reml(phi, y, Z, G=G, solver="dense")
    assert fd.state == 2
    null = x.lmm_null(y, Z, cols=every)
    e0, s2, _ = L.ols(y, Z)
    assert null.state == 2 and null.tau[1] == 0.0 and null.iters == fd.iters and null.h2 == 0.0
    assert abs(null.tau[0] - s2) <= 4 * n * L.U * s2
    assert np.allclose(null.Py, e0 / s2, rtol=0, atol=1e-10 * np.abs(e0 / s2).max()) and np.allclose(null.ratios, 1.0 / s2, rtol=1e-10, atol=0)
    kin, plain = x.assoc(y, Z, kinship=null), x.assoc(y, Z)
    ok = ~np.isnan(plain.z)
    assert np.array_equal(np.isnan(kin.z), ~ok) and ok.sum() > NULL_P // 2
    for a, b in ((kin.z, plain.z), (kin.beta, plain.beta), (kin.se, plain.se), (kin.neglog10p, plain.neglog10p)):
        assert np.allclose(a[ok], b[ok], rtol=1e-9, atol=1e-10 * np.abs(b[ok]).max())


def test_null_model_refusals(mih):
    n, c = 129, 3
    x, codes, phi, y, Z, mk, G = null_case(mih, n, c)
    bad = Z.copy()
    bad[:, 2] = 2.0 * bad[:, 0] - bad[:, 1]
    with pytest.raises(api.ArgumentError, match="rank-deficient.*rank 2"):
        x.lmm_null(y, bad)
    with pytest.raises(api.ArgumentError, match="probes"):
        x.lmm_null(y, np.column_stack([Z] + [np.random.default_rng(k).standard_normal(n) for k in range(61)]), probes=64)      # 1 + 64 + 64
    with pytest.raises(api.ArgumentError, match="probes"):
        x.lmm_null(y, Z, probes=65)
    with pytest.raises(api.ArgumentError, match="R must"):
        x.lmm_null(y, Z, G=np.random.default_rng(0).standard_normal((n, 129)))
    ynan = y.copy()
    ynan[7] = np.nan
    with pytest.raises(api.ArgumentError, match="not finite"):
        x.lmm_null(ynan, Z)
    for kw in (dict(tol=-1.0), dict(max_iter=0), dict(cg_tol=float("nan")), dict(cg_max_iter=0), dict(method="MoM"), dict(markers=0), dict(min_mac=10 ** 9)):
        with pytest.raises(api.ArgumentError):
            x.lmm_null(y, Z, **kw)
    with pytest.raises(api.ArgumentError, match="one trait"):
        x.lmm_null(np.column_stack([y, y]), Z)
    # max_iter reached is not an error: state 0, the iterates so far
    short = x.lmm_null(y, Z, max_iter=2)
    assert short.state == 0 and short.iters == 2 and short.tau_path.shape == (3, 2) and not short.converged and np.all(np.isfinite(short.Py))
    assert bits(short.tau_path) == bits(x.lmm_null(y, Z).tau_path[:3])


def test_assoc_with_kinship(mih):
    n, c = 300, 3
    x, codes, phi, y, Z, mk, G = null_case(mih, n, c)
    null = x.lmm_null(y, Z)
    res = x.assoc(y, Z, kinship=null)
    raw = x.score_test(null.Py, None, Z)
    zs, bs, ss = L.rescale(raw.z, raw.beta, raw.se, null.gamma)
    assert bits(res.z) == bits(zs) and bits(res.beta) == bits(bs) and bits(res.se) == bits(ss) and bits(res.neglog10p) == bits(mih.neglog10p(zs))
    assert res.null is null and np.isfinite(res.z).sum() > NULL_P // 2
    auto = x.assoc(y, Z, kinship=True)
    assert all(bits(a) == bits(b) for a, b in ((auto.z, res.z), (auto.beta, res.beta), (auto.se, res.se), (auto.neglog10p, res.neglog10p)))
    assert bits(auto.null.Py) == bits(null.Py) and auto.null.gamma == null.gamma
    # without kinship: today's path, the bits of a direct score_test call on the null model of the covariates
    plain = x.assoc(y, Z)
    nm = mih.fit_null(y, Z, mih.Normal())
    rt = np.sqrt(nm.phi)
    direct = x.score_test((y - nm.mu) / rt, None, Z)
    assert bits(plain.z) == bits(direct.z) and bits(plain.beta) == bits(direct.beta * rt) and bits(plain.se) == bits(direct.se * rt)
    assert bits(plain.neglog10p) == bits(direct.neglog10p) and bits(x.assoc(y, Z, kinship=None).z) == bits(plain.z)
    ok = np.isfinite(plain.z)
    assert np.allclose(mih.neglog10p(plain.z[ok]), plain.neglog10p[ok], rtol=1e-12, atol=1e-300)       # the same tail function
    # refusals
    yb = (y > np.median(y)).astype(float)
    dense = mih.DenseMatrix(np.random.default_rng(0).standard_normal((n, 5)))
    for call in (lambda: x.assoc(yb, Z, d=mih.Bernoulli(), kinship=True), lambda: x.assoc(y, Z, d=mih.Normal(), l=mih.LogLink(), kinship=null),
                 lambda: x.assoc(np.column_stack([y, y]), Z, kinship=null), lambda: x.assoc(y, Z, spa=True, kinship=null),
                 lambda: x.assoc(y, Z, firth=True, kinship=null), lambda: dense.assoc(y, Z, kinship=True), lambda: x.assoc(y, Z, kinship="yes")):
        with pytest.raises(api.ArgumentError):
            call()
    # one statistical reading, recorded and not asserted beyond finiteness: the exact per-SNP statistic (x'Py)^2 / (x'Px) with
    # the dense P at the fitted tau against the device's z^2, whose denominator is gamma x~'x~ -- the variance-ratio approximation
    vinv = np.linalg.inv(L.vmat(phi, null.tau[0], null.tau[1]))
    pm = vinv - vinv @ Z @ np.linalg.inv(Z.T @ vinv @ Z) @ Z.T @ vinv
    cols = np.flatnonzero(np.isfinite(res.z))
    X = mean_imputed(codes, cols)
    exact = (X.T @ (pm @ y)) ** 2 / np.einsum("ij,ij->j", X, pm @ X)
    reld = np.abs(res.z[cols] ** 2 - exact) / np.maximum(exact, 1e-12)
    big = exact > 1.0
    print(f"variance-ratio approximation at n = 300, p = 2000: z^2 against the exact statistic, relative difference median "
          f"{np.median(reld[big]):.3e}, max {reld[big].max():.3e} over the {int(big.sum())} SNPs with exact statistic > 1; gamma {null.gamma:.4f}, "
          f"cv of the ratios {null.ratio_cv:.3f}")
    assert np.all(np.isfinite(reld))


def test_gwas_with_lmm_writes_the_rescaled_scan(mih, tmp_path):
    """The file-level entry: a PLINK trio of the planted genotypes, the phenotype in the .fam -- gwas(lmm=True) is
    x.assoc(y, kinship=True) of the same matrix, one row per SNP in the usual columns."""
    from test_gpu_hardcall_pack import bed_of
    n, c = 300, 1
    x, codes, phi, y, Z, mk, G = null_case(mih, n, c)
    prefix = str(tmp_path / "planted")
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]) + bed_of(codes).tobytes())
    with open(prefix + ".fam", "w") as f:
        f.writelines(f"{i + 1} 1 0 0 1 {float(y[i])!r}\n" for i in range(n))
    with open(prefix + ".bim", "w") as f:
        f.writelines(f"1\tsnp{j + 1}\t0\t{j + 1}\t1\t2\n" for j in range(NULL_P))
    out = str(tmp_path / "lmm.txt")
    res = mih.gwas(prefix, mih.Normal, outfile=out, lmm=True)
    ref = x.assoc(y, kinship=True)
    assert isinstance(res.null, mih.LmmNull) and res.null.state == ref.null.state == 1 and res.null.iters == ref.null.iters
    for a, b in ((res.z, ref.z), (res.beta, ref.beta), (res.se, ref.se), (res.neglog10p, ref.neglog10p)):
        assert np.allclose(a, b, rtol=1e-9, atol=1e-12, equal_nan=True)
    rows = open(out).read().splitlines()
    assert rows[0] == "chr\tpos\tSNPid\tref\talt\tz\tbeta\tse\tneglog10p" and len(rows) == NULL_P + 1
    j = int(np.nanargmax(np.abs(res.z)))
    assert rows[j + 1].split("\t")[5] == repr(float(res.z[j]))
