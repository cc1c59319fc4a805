"""The leading principal components of the kinship matrix on the device (csrc/pca.hip: mih_grm_eig; pca() of SnpLinAlg and
DosageMatrix) against the numpy statement tests/pca_spec.py.

Inputs: the planted generator of pca_spec at the shapes where the kernels change path -- 16 / 17 around a matrix-core block,
63 / 65 around a wave's share of the tile, 128 / 129 around a tile, 257 = three tiles, column counts below and above the block
size (Phi has rank < b at p = 4 and 5) -- plus one sample.  tests/test_pca_spec_cpu.py asserts, from the spec alone, that every
one of them has relative gaps of at least 0.05 among its leading k + 1 eigenvalues.

Bounds, derived and not measured (pca_spec states them): Phi_s, lambda^s, v^s from grm_spec.grm and eigh on the handle's own
mu_sigma(); E = grm_spec.bound, u = 2^-53, rho_i = |Phi_s u_i - lambda_i u_i|_2 evaluated in numpy, gap_i the distance from
lambda^s_i to the nearest other eigenvalue of Phi_s.
    residual       rho_i <= tol lambda_1 + |E|_F + 8 (n + b) u |Phi_s|_F
    values         |lambda_i - lambda^s_i| <= rho_i + 8 n u lambda^s_1
    vectors        |u_i - v^s_i|_2 <= (2 rho_i + 16 n u lambda^s_1) / gap_i      (after the sign rule)
    orthonormal    |U'U - I| <= 8 (n + b) u elementwise"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grm_spec as K
import pca_spec as P
import qc_spec as Q
from conftest import FIX, free_device_bytes
from test_gpu_hardcall_pack import codes_of, from_bed, numerators

from mendeliht_amd import api

pytestmark = pytest.mark.gpu

TOL = 1e-10
BAD_ARG = 2


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_bits(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a[:3], b[:3])) and a.iters == b.iters and a.converged == b.converged


class Spec:
    """Everything the bounds need of one (handle, genotypes, column selection, method), computed once."""

    def __init__(self, h, g, method, cols=None):
        mu, sinv = h.mu_sigma()
        self.n = g.shape[0]
        self.phi = K.grm(g, mu, sinv, cols, method)
        self.e_fro = float(np.linalg.norm(K.bound(g, mu, sinv, cols, method)))
        self.lam = np.linalg.eigvalsh(self.phi)[::-1]
        self.fro = float(np.linalg.norm(self.phi))

    def round_off(self, b):
        """The last two terms of the residual bound."""
        return self.e_fro + 8.0 * (self.n + b) * P.U * self.fro

    def check(self, res, k, b, what, tol=TOL, vectors=True):
        n = self.n
        w, v = P.top(self.phi, k)
        assert res.values.shape == (k,) and res.vectors.shape == (n, k) and res.residuals.shape == (k,), what
        rho = P.residuals(self.phi, res.values, res.vectors)
        rb = tol * w[0] + self.round_off(b)
        print(what, "iters", res.iters, "rho/bound", float((rho / rb).max()) if rb > 0 else float(rho.max()))
        assert np.all(rho <= rb), (what, rho, rb)
        assert np.all(np.abs(res.values - w) <= P.value_bound(rho, w[0], n)), (what, res.values, w)
        assert np.all(np.diff(res.values) <= 0.0), what
        if vectors:
            err = np.linalg.norm(res.vectors - v, axis=0)
            assert np.all(err <= P.vector_bound(rho, w[0], n, P.gaps(self.lam, k))), (what, err)
        assert np.abs(res.vectors.T @ res.vectors - np.eye(k)).max() <= P.orth_bound(n, b), what
        for c in range(k):                                           # the sign rule
            col = res.vectors[:, c]
            assert col[np.argmax(np.abs(col))] > 0.0, (what, c)
        # the device's own residuals: those of the returned pairs, up to the rounding of the two evaluations
        assert np.all(np.abs(res.residuals - rho) <= self.round_off(b)), (what, res.residuals, rho)
        if res.converged:
            assert res.residuals.max() <= tol * res.values[0], what
        return rho


# ---- 1. the planted inputs at the edge shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_planted_structure_at_the_edge_shapes(mih, shape):
    n, p, k = shape
    codes = P.planted(n, p, k)
    x = from_bed(mih, codes)
    g = K.genotypes(codes)
    b, _ = P.block_size(k, n)
    r = np.random.default_rng(n + p).standard_normal(n)
    before = x.xtv(r)
    for method in K.METHODS:
        spec = Spec(x, g, method)
        res = x.pca(k, method=method, cols=np.ones(p, dtype=bool))
        assert res.converged and 1 <= res.iters <= 60, (shape, method, res.iters)
        spec.check(res, k, b, (shape, method))
        for pc in (0, 4, 64):                                        # a second call, and Phi's bits do not depend on the panels
            again = x.pca(k, method=method, cols=np.ones(p, dtype=bool), panel_cols=pc)
            assert same_bits(res, again), (shape, method, pc)
    assert bits(x.xtv(r)) == bits(before), shape                     # the source is only read


def test_one_sample(mih):
    """n = 1: the centred genotype of the only sample is 0, so Phi is the single value Phi_11 = 0 >= 0, which is its own
    eigenvalue, with the vector (1).  Robust divides by 2 sum mu (1 - mu / 2), which is 0 for the planted (all-homozygous)
    sample: Phi has no finite number and the numerical rank is 0."""
    codes = P.planted(1, 4, 1)
    x = from_bed(mih, codes)
    phi = x.grm(cols=np.ones(4, dtype=bool))
    assert phi.shape == (1, 1) and phi[0, 0] >= 0.0
    res = x.pca(1, cols=np.ones(4, dtype=bool))
    assert res.converged and res.iters == 1
    assert res.values[0] == phi[0, 0] and np.array_equal(res.vectors, [[1.0]]) and res.residuals[0] == 0.0
    assert np.isnan(x.grm(method="Robust", cols=np.ones(4, dtype=bool))[0, 0])
    with pytest.raises(api.ArgumentError, match="rank 0"):
        x.pca(1, method="Robust", cols=np.ones(4, dtype=bool))


# ---- 2. options -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(mih):
    n, p, k = 257, 600, 4
    codes = P.planted(n, p, k)
    x = from_bed(mih, codes)
    spec = Spec(x, K.genotypes(codes), "GRM")
    spec.phi.setflags(write=False)
    return codes, x, spec, np.ones(p, dtype=bool)


def test_seed_and_block_agree_within_the_bounds(mih, wide):
    codes, x, spec, every = wide
    k = 4
    got = {}
    for seed, block in ((0, 0), (1, 0), (0, 16), (0, 32), (0, 4), (0, 64), (0, 128)):
        res = x.pca(k, cols=every, seed=seed, block=block)
        assert res.converged, (seed, block)
        spec.check(res, k, P.block_size(k, 257, block)[0], (seed, block))
        got[seed, block] = res
    assert same_bits(got[0, 0], got[0, 16])                          # the rule gives 16 for k = 4
    assert not same_bits(got[0, 0], got[1, 0]) and not same_bits(got[0, 16], got[0, 32])
    assert same_bits(got[1, 0], x.pca(k, cols=every, seed=1))
    # a selection of columns and the default minmaf rule
    half = np.arange(600) % 2 == 0
    sub = Spec(x, K.genotypes(codes), "GRM", half)
    sub.check(x.pca(k, cols=half), k, 16, "half", vectors=P.relative_gap(sub.lam, k) >= 0.05)
    with np.errstate(invalid="ignore"):
        keep = Q.maf(Q.counts(codes)[0]) >= 0.01
    assert same_bits(x.pca(k), x.pca(k, cols=keep)) and same_bits(x.pca(k, method=0), x.pca(k, method="GRM"))


def test_max_iter_returns_the_last_ritz_pairs_with_honest_residuals(mih, wide):
    codes, x, spec, every = wide
    k, b = 4, 16
    res = x.pca(k, cols=every, max_iter=1)
    assert res.converged is False and res.iters == 1
    assert res.residuals.max() > TOL * res.values[0]
    rho = P.residuals(spec.phi, res.values, res.vectors)
    assert np.all(np.abs(res.residuals - rho) <= spec.round_off(b)), (res.residuals, rho)
    assert np.abs(res.vectors.T @ res.vectors - np.eye(k)).max() <= P.orth_bound(257, b)
    # a loose tolerance stops early, and says so
    loose = x.pca(k, cols=every, tol=1e-3)
    assert loose.converged and loose.iters < x.pca(k, cols=every).iters and loose.residuals.max() <= 1e-3 * loose.values[0]
    # tol = 0 cannot be met: max_iter products, the pairs still within the bounds of a converged run
    zero = x.pca(k, cols=every, tol=0.0, max_iter=40)
    assert not zero.converged and zero.iters == 40
    spec.check(zero, k, b, "tol=0")


def test_rank_below_k_is_refused_with_the_rank_found(mih):
    codes = P.planted(40, 1, 1, seed=1)                              # one polymorphic column: Phi = x x' / 2 has rank 1
    x = from_bed(mih, codes)
    res = x.pca(1, cols=np.ones(1, dtype=bool))
    spec = Spec(x, K.genotypes(codes), "GRM")
    spec.check(res, 1, 16, "rank 1")
    assert abs(res.values[0] - np.trace(spec.phi)) <= 1e-12 * res.values[0]
    with pytest.raises(api.ArgumentError, match="rank 1"):
        x.pca(2, cols=np.ones(1, dtype=bool))
    assert same_bits(res, x.pca(1, cols=np.ones(1, dtype=bool)))     # and the handle still serves


# ---- 3. dosage handles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 150, 3), (129, 150, 3)], ids=lambda s: "-".join(map(str, s)))
def test_dosage_matrix_of_the_same_hard_calls(mih, shape):
    n, p, k = shape
    codes = P.planted(n, p, k)
    d = mih.DosageMatrix(numerators(codes, unit=1), 2)
    g = K.genotypes(codes) / 2.0
    r = np.random.default_rng(n).standard_normal(n)
    before = d.xtv(r)
    for method in K.METHODS:
        spec = Spec(d, g, method)
        assert P.relative_gap(spec.lam, k) >= 0.05
        res = d.pca(k, method=method, cols=np.ones(p, dtype=bool))
        assert res.converged
        spec.check(res, k, 16, (shape, method, "dosage"))
        assert same_bits(res, d.pca(k, method=method, cols=np.ones(p, dtype=bool), panel_cols=4))
    assert bits(d.xtv(r)) == bits(before)


# ---- 4. the shipped fixture -------------------------------------------------------------------------------------------------------
def test_shipped_fixture_with_the_default_minmaf(mih):
    """n = 1000 unrelated samples without planted structure: the gaps are small, so the vectors are compared as a subspace,
    |(I - V_s V_s') U|_F <= 2 max rho / (lambda^s_5 - lambda^s_6) (Davis-Kahan for the invariant subspace).  The spectrum is
    nearly flat -- lambda_17 / lambda_5 = 0.97 is the rate of a block of 16 -- so tol = 1e-10 takes about 700 products, more
    than the default max_iter: the call asks for 2000."""
    n, k = 1000, 5
    bed = mih.read_bed(os.path.join(FIX, "normal.bed"), n)
    x = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    codes = codes_of(bed, n)
    with np.errstate(invalid="ignore"):
        keep = Q.maf(Q.counts(codes)[0]) >= 0.01
    spec = Spec(x, K.genotypes(codes), "GRM", keep)
    if spec.lam[4] - spec.lam[5] < 1e-3 * spec.lam[0]:
        pytest.skip("the spec's own lambda_5 - lambda_6 is below 1e-3 lambda_1: no subspace to compare")
    res = x.pca(k, max_iter=2000)
    assert res.converged and res.iters > 500
    assert not x.pca(k, max_iter=50).converged                      # and the default way of running out of iterations
    w, v = P.top(spec.phi, k)
    rho = P.residuals(spec.phi, res.values, res.vectors)
    print("fixture: iters", res.iters, "rho", rho, "gap56", spec.lam[4] - spec.lam[5])
    assert np.all(rho <= TOL * w[0] + spec.round_off(16))
    assert np.all(np.abs(res.values - w) <= P.value_bound(rho, w[0], n))
    out = res.vectors - v @ (v.T @ res.vectors)
    assert np.linalg.norm(out) <= 2.0 * rho.max() / (spec.lam[4] - spec.lam[5])
    # the recipe of the docstring
    z = np.column_stack([np.ones(x.n), res.vectors])
    assert z.shape == (1000, 6)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def last_error(mih):
    buf = C.create_string_buffer(512)
    mih.lib().mih_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def test_refusals_leave_the_outputs_untouched(mih):
    L = mih.lib()
    codes = P.planted(17, 33, 2)
    x = from_bed(mih, codes)
    dense = mih.DenseMatrix(np.random.default_rng(0).standard_normal((17, 5)))
    val, vec, res = np.full(20, -7.0), np.full(17 * 20, -7.0), np.full(20, -7.0)
    it, conv = C.c_int32(-7), C.c_int32(-7)
    none = np.zeros(33, dtype=np.uint8)
    before = free_device_bytes()

    def call(h=None, ck=None, method=0, k=2, block=0, tol=TOL, max_iter=500, out=None):
        o = [a.ctypes.data_as(C.c_void_p) for a in (val, vec, res)] + [C.byref(it), C.byref(conv)]
        if out is not None:
            o[out] = None
        return L.mih_grm_eig(x._h if h is None else h, None if ck is None else ck.ctypes.data_as(C.c_void_p), method, 0, k, block, tol,
                             max_iter, 0, *o)

    cases = [("dense", dict(h=dense._h)), ("empty", dict(ck=none)), ("method", dict(method=7)), ("k0", dict(k=0)), ("k>n", dict(k=18)),
             ("k>64", dict(k=65)), ("block<k", dict(k=5, block=4)), ("block>128", dict(block=129)), ("tol nan", dict(tol=float("nan"))),
             ("tol inf", dict(tol=float("inf"))), ("tol<0", dict(tol=-1.0)), ("max_iter", dict(max_iter=0))]
    cases += [(f"null {i}", dict(out=i)) for i in range(5)]
    for what, kw in cases:
        assert call(**kw) == BAD_ARG and last_error(mih), what
        assert np.all(val == -7.0) and np.all(vec == -7.0) and np.all(res == -7.0) and it.value == -7 and conv.value == -7, what
    assert abs(free_device_bytes() - before) <= 64 << 20
    for kw in (dict(k=0), dict(k=18), dict(block=200), dict(tol=float("nan")), dict(max_iter=0), dict(method="MoM"),
               dict(cols=np.zeros(33, dtype=bool))):
        with pytest.raises(api.ArgumentError):
            x.pca(**{"k": 2, **kw})
    assert call() == 0 and it.value >= 1 and conv.value == 1        # and the handle still serves, k = 2 of room for 20
    assert np.all(val[2:] == -7.0) and np.all(vec[2 * 17:] == -7.0) and np.all(res[2:] == -7.0)
    assert bits(vec[:2 * 17].reshape(2, 17).T) == bits(x.pca(2, cols=np.ones(33, dtype=bool)).vectors)      # n x k, column-major


def test_a_matrix_the_device_cannot_hold_is_refused_before_anything_is_allocated(mih):
    x = mih.SnpLinAlg.synthetic(300_000, 32)
    before = free_device_bytes()
    with pytest.raises(MemoryError) as e:
        x.pca(10)
    need, free = (int(v) for v in re.findall(r"(\d{9,}) bytes", str(e.value)))
    assert need >= 8 * 300_032 ** 2 + 3 * 8 * 300_032 * 32 and need > free and abs(free - before) <= 64 << 20
    assert abs(free_device_bytes() - before) <= 64 << 20
