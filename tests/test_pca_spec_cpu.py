"""The numpy statement of pca() (tests/pca_spec.py) against itself and eigh, the conditions the GPU tests of
tests/test_gpu_pca.py rely on -- asserted from the spec alone, on every input they use -- and the interface of the entry point:
declared, exported, mirrored, and refusing bad arguments on the host (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grm_spec as K
import pca_spec as P
from conftest import ROOT

BAD_ARG = 2


def spec_phi(n, p, k, method):
    g = K.genotypes(P.planted(n, p, k))
    mu, sinv = K.mu_sigma(g)
    return K.grm(g, mu, sinv, None, method)


def test_top_on_a_matrix_with_known_eigenpairs():
    """Phi = V diag(9, 4, 1) V' with V = [(3, 4, 0) / 5, (-4, 3, 0) / 5, (0, 0, 1)]: the second vector's largest entry is negative,
    so the sign rule returns its negative, whatever sign eigh gave it."""
    v = np.array([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
    phi = (v * np.array([9.0, 4.0, 1.0])[None, :]) @ v.T
    w, u = P.top(phi, 2)
    assert np.allclose(w, [9.0, 4.0], rtol=0, atol=1e-14)
    assert np.allclose(u, [[0.6, 0.8], [0.8, -0.6], [0.0, 0.0]], rtol=0, atol=1e-14)
    w, u = P.top(-phi + 10.0 * np.eye(3), 3)                              # the order reverses: 9, 6, 1
    assert np.allclose(w, [9.0, 6.0, 1.0], rtol=0, atol=1e-14)
    assert np.allclose(u, [[0.0, 0.8, 0.6], [0.0, -0.6, 0.8], [1.0, 0.0, 0.0]], rtol=0, atol=1e-14)
    # a tie in magnitude goes to the lowest index; a clear maximum decides otherwise
    assert np.array_equal(P.sign_rule(np.array([-2.0, 2.0, 1.0])), [2.0, -2.0, -1.0])
    assert np.array_equal(P.sign_rule(np.array([1.0, -3.0, 2.0])), [-1.0, 3.0, -2.0])
    assert np.array_equal(P.sign_rule(np.array([[1.0, -1.0], [-3.0, 0.5]])), [[-1.0, 1.0], [3.0, -0.5]])


def test_block_size_rule_and_start_block():
    assert [P.block_size(k, 10 ** 6)[0] for k in (1, 4, 8, 9, 10, 24, 25, 64)] == [16, 16, 16, 32, 32, 48, 64, 128]
    assert P.block_size(3, 7) == (16, 7) and P.block_size(3, 300, 32) == (32, 32)
    q = P.start(0, 300, 16)
    assert q.shape == (300, 16) and np.all(np.abs(q) < 1.0) and np.all(q != 0.0)
    assert abs(q.mean()) < 0.05 and abs(q.std() - 1 / np.sqrt(3)) < 0.02            # uniform on (-1, 1)
    assert np.array_equal(q, P.start(0, 300, 16)) and not np.array_equal(q, P.start(1, 300, 16))
    assert np.array_equal(P.start(5, 300, 16)[:17, :3], P.start(5, 17, 3))          # an entry depends on (seed, row, column) alone
    # the first entry by hand: splitmix64's output function of 0 + golden * 1
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & P.MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & P.MASK
    z ^= z >> 31
    assert q[0, 0] == ((z >> 12) + 0.5) * 2.0 ** -51 - 1.0


def test_orth_twice_is_enough():
    """A block with condition number 1e6: one pass through the Gram matrix leaves u cond^2 = 1e-4 of orthogonality error, the
    second pass brings it to rounding."""
    rng = np.random.default_rng(3)
    y = np.linalg.qr(rng.standard_normal((200, 8)))[0] @ np.diag(10.0 ** -np.arange(8) * 10) @ np.linalg.qr(rng.standard_normal((8, 8)))[0]
    once = P.orth(y)
    twice = P.orth(once)
    err1 = np.abs(once.T @ once - np.eye(8)).max()
    err2 = np.abs(twice.T @ twice - np.eye(8)).max()
    assert once.shape == twice.shape == (200, 8)
    assert err2 <= P.orth_bound(200, 8) < err1


@pytest.mark.parametrize("method", K.METHODS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_conditions_the_gpu_tests_rely_on(shape, method):
    """Every planted input of test_gpu_pca.py: the leading k + 1 eigenvalues are separated by at least 0.05 lambda_1, so that
    matching by rank is unambiguous and the vector bound is finite; and the numpy iteration reaches tol = 1e-10 within 60
    iterations with the default block, within all four bounds against eigh."""
    n, p, k = shape
    phi = spec_phi(n, p, k, method)
    assert np.all(np.isfinite(phi))
    lam = np.linalg.eigvalsh(phi)[::-1]
    assert P.relative_gap(lam, k) >= 0.05, P.relative_gap(lam, k)
    b, bl = P.block_size(k, n)
    val, vec, res, it, done = P.iterate(phi, k, tol=1e-10)
    assert done and it <= 60, it
    assert res.max() <= 1e-10 * val[0]
    w, v = P.top(phi, k)
    rho = P.residuals(phi, val, vec)
    assert np.all(rho <= P.residual_bound(phi, w[0], 1e-10, n, b))
    assert np.all(np.abs(val - w) <= P.value_bound(rho, w[0], n))
    assert np.all(np.linalg.norm(vec - v, axis=0) <= P.vector_bound(rho, w[0], n, P.gaps(lam, k)))
    assert np.abs(vec.T @ vec - np.eye(k)).max() <= P.orth_bound(n, b)


def test_iteration_options_agree_within_the_bounds():
    n, p, k = 257, 600, 4
    phi = spec_phi(n, p, k, "GRM")
    lam = np.linalg.eigvalsh(phi)[::-1]
    w, v = P.top(phi, k)
    for block, seed in ((0, 1), (32, 0), (4, 0)):
        b, _ = P.block_size(k, n, block)
        val, vec, res, it, done = P.iterate(phi, k, block=block, seed=seed, max_iter=500)
        assert done
        rho = P.residuals(phi, val, vec)
        assert np.all(rho <= P.residual_bound(phi, w[0], 1e-10, n, b))
        assert np.all(np.linalg.norm(vec - v, axis=0) <= P.vector_bound(rho, w[0], n, P.gaps(lam, k)))
    # max_iter = 1: not converged, one product taken, and the residuals are the honest ones of the returned pairs
    val, vec, res, it, done = P.iterate(phi, k, max_iter=1)
    assert not done and it == 1 and res.max() > 1e-10 * val[0]
    assert np.allclose(res, P.residuals(phi, val, vec), rtol=1e-9, atol=8 * (n + 16) * P.U * np.linalg.norm(phi))


def test_rank_below_k_and_one_sample():
    g = K.genotypes(P.planted(40, 1, 1, seed=1))                  # a polymorphic column with two missing genotypes
    mu, sinv = K.mu_sigma(g)
    phi = K.grm(g, mu, sinv, None, "GRM")
    assert np.linalg.matrix_rank(phi) == 1
    val, vec, res, it, done = P.iterate(phi, 1)
    assert done and abs(val[0] - np.trace(phi)) <= 1e-12 * val[0]
    with pytest.raises(P.RankError, match="rank 1"):
        P.iterate(phi, 2)
    # one sample: the centred genotype is 0, Phi_11 = 0 is its own eigenvalue and the vector is (1)
    phi1 = spec_phi(1, 4, 1, "GRM")
    assert phi1.shape == (1, 1) and phi1[0, 0] >= 0.0
    val, vec, res, it, done = P.iterate(phi1, 1)
    assert done and it == 1 and val[0] == phi1[0, 0] and np.array_equal(vec, [[1.0]]) and res[0] == 0.0
    # ... and where the Robust divisor is 0 there is no finite number in Phi: numerical rank 0
    phi1 = spec_phi(1, 4, 1, "Robust")
    assert np.isnan(phi1[0, 0])
    with pytest.raises(P.RankError, match="rank 0"):
        P.iterate(phi1, 1)


def test_planted_generator():
    codes = P.planted(300, 1000, 5)
    assert codes.shape == (300, 1000) and set(np.unique(codes)) == {-1, 0, 1, 2}
    assert np.all(codes[:, 3] == 0) and np.all(codes[:, 17] == 2) and np.all(codes[:, 998] == -1)
    assert abs(np.mean(codes == -1) - 0.05) < 0.01
    assert np.array_equal(codes, P.planted(300, 1000, 5))
    assert P.planted(16, 4, 1).shape == (16, 4)


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_mirrored(mih):
    from mendeliht_amd import api
    header = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"^int\s+(mih_\w+)\s*\(", header, flags=re.M))
    assert "mih_grm_eig" in declared and "mih_grm_eig" in api.exported_symbols()
    getattr(C.CDLL(mih.library_path()), "mih_grm_eig")
    for cls in (mih.SnpLinAlg, mih.DosageMatrix):
        assert callable(cls.pca) and "np.column_stack([np.ones(x.n), x.pca(10).vectors])" in cls.pca.__doc__
    assert not hasattr(mih.DenseMatrix, "pca")
    assert mih.PcaResult._fields == ("values", "vectors", "residuals", "iters", "converged")


def test_argument_refusals_come_before_any_device_call(mih):
    """k, block, tol, max_iter and a null handle are refused on the host, before the first device call -- so they are refused
    on a machine without a device too -- with a message, and nothing is written."""
    L = mih.lib()
    out = [np.full(4, -7.0), np.full(40, -7.0), np.full(4, -7.0)]
    it, conv = C.c_int32(-7), C.c_int32(-7)

    def call(k=2, block=0, tol=1e-10, max_iter=500):
        rc = L.mih_grm_eig(None, None, 0, 0, k, block, tol, max_iter, 0, *(a.ctypes.data_as(C.c_void_p) for a in out), C.byref(it), C.byref(conv))
        buf = C.create_string_buffer(512)
        L.mih_last_error(buf, 512)
        return rc, buf.value.decode(errors="replace")

    for kw, word in ((dict(k=0), "k must"), (dict(k=-1), "k must"), (dict(k=65), "k must"), (dict(block=1), "block"), (dict(block=129), "block"),
                     (dict(k=20, block=16), "block"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"),
                     (dict(tol=-1e-3), "tol"), (dict(max_iter=0), "max_iter"), (dict(), "null matrix handle")):
        rc, msg = call(**kw)
        assert rc == BAD_ARG and word in msg, (kw, rc, msg)
        assert all(np.all(a == -7.0) for a in out) and it.value == -7 and conv.value == -7, kw
