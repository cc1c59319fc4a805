"""The numpy statement of kinship_solve() (tests/lmm_spec.py) against itself and a Cholesky solve, the conditions the GPU tests
of tests/test_gpu_lmm.py rely on -- asserted from the spec alone, on every input they use -- and the interface of the entry
point: declared, exported, mirrored, and refusing bad arguments on the host (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grm_spec as K
import lmm_spec as L
import pca_spec as P
from conftest import ROOT

BAD_ARG = 2
TE, TG = L.TAU


def spec_phi(n, method, cols=None, p=L.SOLVE_P):
    g = K.genotypes(P.planted(n, p, 3))
    mu, sinv = K.mu_sigma(g)
    return K.grm(g, mu, sinv, cols, method)


def variants(p=L.SOLVE_P):
    return (("GRM", None), ("GRM", np.arange(p) % 3 != 1), ("Robust", None))


def test_pcg_on_a_system_with_a_known_solution():
    """Phi = diag(1, 2, 3): the Jacobi preconditioner is the inverse, one iteration; and a full 3 x 3 matrix, at most 3."""
    phi = np.diag([1.0, 2.0, 3.0])
    b = np.array([1.0, -2.0, 0.5])
    x, it, conv, res, theta = L.pcg(phi, b, 0.5, 2.0)
    assert it[0] == 1 and conv[0] and np.allclose(x, b / (0.5 + 2.0 * np.array([1.0, 2.0, 3.0])), rtol=1e-15, atol=0)
    phi = np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 4.0]])
    x, it, conv, res, theta = L.pcg(phi, np.column_stack([b, np.zeros(3), 2.0 * b]), 0.5, 2.0)
    assert list(conv) == [True, True, True] and it[0] <= 3 and it[1] == 0 and it[2] == it[0]
    assert np.allclose(x[:, 0], L.dense(phi, b, 0.5, 2.0), rtol=1e-12, atol=0) and np.all(x[:, 1] == 0.0) and res[1] == 0.0
    assert np.array_equal(x[:, 2], 2.0 * x[:, 0])                     # (a power of two: the same roundings)
    assert theta[1] == 0.0 and theta[0] >= np.linalg.norm(x[:, 0]) * (1 - 1e-12)
    # max_iter = 1: one iteration, not converged, finite, and the residual is the honest one
    x1, it, conv, res, _ = L.pcg(phi, b, 0.5, 2.0, max_iter=1)
    assert it[0] == 1 and not conv[0] and np.all(np.isfinite(x1)) and res[0] == np.linalg.norm(b - L.vmat(phi, 0.5, 2.0) @ x1)
    # tol >= 1 is met by x = 0
    x0, it, conv, res, _ = L.pcg(phi, b, 0.5, 2.0, tol=1.0)
    assert it[0] == 0 and conv[0] and np.all(x0 == 0.0) and res[0] == np.linalg.norm(b)


@pytest.mark.parametrize("n", L.SOLVE_N)
def test_conditions_the_gpu_tests_rely_on(n):
    """Every input of test_gpu_lmm.py: V is well conditioned (kappa <= 1e3), the numpy iteration reaches tol = 1e-10 well
    inside max_iter = 500 for every column, its solution is the Cholesky solve's within the residual, and the gap between
    its recurrence residual and its true residual is inside gap_bound -- printed beside the bound."""
    worst = 0.0
    for method, cols in variants():
        phi = spec_phi(n, method, cols)
        assert np.all(np.isfinite(phi))
        v = L.vmat(phi, TE, TG)
        lam = np.linalg.eigvalsh(v)
        assert lam[0] > 0 and lam[-1] / lam[0] <= 1e3, (n, method, lam[-1] / lam[0])
        v_fro = np.linalg.norm(v)
        for m in L.SOLVE_M:
            B = L.rhs(n, m)
            x, it, conv, res, theta = L.pcg(phi, B, TE, TG)
            assert conv.all() and it.max() <= 100, (n, m, method, it.max())
            bn, xn = np.linalg.norm(B, axis=0), np.linalg.norm(x, axis=0)
            gap = np.maximum(res - L.TOL * bn, 0.0)                  # what the true residual has beyond the stopping rule
            bound = L.gap_bound(it, n, v_fro, theta, bn) + L.eval_bound(n, v_fro, xn, bn)
            assert np.all(gap <= bound), (n, m, method)
            worst = max(worst, float((res / bn).max()))
            err = np.linalg.norm(x - L.dense(phi, B, TE, TG), axis=0)
            assert np.all(err <= (res + 8 * n * L.U * v_fro * xn) / lam[0]), (n, m, method)
    print(f"n = {n}: largest true residual of a converged column {worst:.3e} |b| (tol 1e-10)")


def test_recurrence_gap_measured_beside_the_bound():
    """The gap |(b - V x_k) - r_k| of the numpy iteration itself at the largest shape, run to tol = 0 for 60 iterations so that
    the recurrence residual is far below the gap: what remains of the true residual is the gap."""
    n, m = 513, 128
    phi = spec_phi(n, "GRM")
    v_fro = np.linalg.norm(L.vmat(phi, TE, TG))
    B = L.rhs(n, m)
    x, it, conv, res, theta = L.pcg(phi, B, TE, TG, tol=0.0, max_iter=60)
    bn = np.linalg.norm(B, axis=0)
    bound = L.gap_bound(it, n, v_fro, theta, bn) + L.eval_bound(n, v_fro, np.linalg.norm(x, axis=0), bn)
    print(f"gap after 60 iterations: at most {float((res / bn).max()):.3e} |b|, the bound allows {float((bound / bn).max()):.3e} |b|")
    assert np.all(res <= bound)


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_mirrored(mih):
    from mendeliht_amd import api
    header = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"^int\s+(mih_\w+)\s*\(", header, flags=re.M))
    assert "mih_grm_solve" in declared and "mih_grm_solve" in api.exported_symbols()
    getattr(C.CDLL(mih.library_path()), "mih_grm_solve")
    for cls in (mih.SnpLinAlg, mih.DosageMatrix):
        assert callable(cls.kinship_solve) and "V = tau_e I + tau_g Phi" in cls.kinship_solve.__doc__
    assert not hasattr(mih.DenseMatrix, "kinship_solve")
    assert mih.SolveResult._fields == ("x", "iters", "converged", "residuals")


def test_argument_refusals_come_before_any_device_call(mih):
    """m, tau_e, tau_g, tol, max_iter and a null handle are refused on the host, before the first device call -- so they are
    refused on a machine without a device too -- with a message, and nothing is written."""
    lib = mih.lib()
    B = np.ones(8)
    out = [np.full(8, -7.0), np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32), np.full(4, -7.0)]

    def call(te=1.0, tg=1.0, m=2, tol=1e-10, max_iter=500):
        rc = lib.mih_grm_solve(None, None, 0, 0, te, tg, B.ctypes.data_as(C.c_void_p), m, tol, max_iter, *(a.ctypes.data_as(C.c_void_p) for a in out))
        buf = C.create_string_buffer(512)
        lib.mih_last_error(buf, 512)
        return rc, buf.value.decode(errors="replace")

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(m=0), "m must"), (dict(m=-3), "m must"), (dict(m=129), "m must"), (dict(te=0.0), "tau_e"), (dict(te=-1.0), "tau_e"),
                     (dict(te=nan), "tau_e"), (dict(te=inf), "tau_e"), (dict(tg=-1.0), "tau_g"), (dict(tg=nan), "tau_g"), (dict(tg=inf), "tau_g"),
                     (dict(tol=nan), "tol"), (dict(tol=inf), "tol"), (dict(tol=-1e-3), "tol"), (dict(max_iter=0), "max_iter"),
                     (dict(), "null matrix handle")):
        rc, msg = call(**kw)
        assert rc == BAD_ARG and word in msg, (kw, rc, msg)
        assert all(np.all(a == -7) for a in out), kw


# ---- the REML null model ------------------------------------------------------------------------------------------------------------
NULL_P = 2000
NULL_CASES = [(129, 1), (129, 3), (300, 1), (300, 3), (513, 1), (513, 3)]
TOL_REML = 1e-5


def null_inputs(n, c, noise=False, seed=None):
    """The inputs of test_gpu_lmm.null_case, with the spec's own mu and sigma."""
    codes = P.planted(n, NULL_P, 3)
    g = K.genotypes(codes)
    mu, sinv = K.mu_sigma(g)
    a, div = K.operand(g, mu, sinv, None, "GRM")
    seed = n + c if seed is None else seed
    Z = L.covariates(n, c, seed)
    y = L.phenotype(a * np.sqrt(a.shape[1] / div), Z, np.arange(1, c + 1, dtype=float), 0.0 if noise else 1.0, 1.0, seed)
    gm = g[:, 40:70]
    return (a @ a.T) / div, y, Z, np.where(np.isnan(gm), np.nanmean(gm, axis=0)[None, :], gm)


def test_probes_and_the_small_algebra():
    u = L.probes(0, 300, 30)
    assert u.shape == (300, 30) and set(np.unique(u)) == {-1.0, 1.0} and abs(u.mean()) < 0.03
    assert np.array_equal(u, L.probes(0, 300, 30)) and not np.array_equal(u, L.probes(1, 300, 30))
    assert np.array_equal(L.probes(5, 300, 30)[:17, :3], L.probes(5, 17, 3))          # an entry depends on (seed, row, probe) alone
    q = P.start(0, 300, 30)                                                            # the same hash as pca's start: its top bit is the sign
    assert np.array_equal(u, np.where(q < 0.0, 1.0, -1.0))                             # (z >> 12) 2^-51 - 1 < 0 <=> the top bit is 0
    nxt, h = L.ai_step(np.array([1.0, 1.0]), np.array([1.0, 2.0]), np.array([[2.0, 1.5], [0.5, 3.0]]))
    assert h == 0 and np.allclose(nxt, [1.2, 1.6], rtol=1e-15, atol=0)
    nxt, h = L.ai_step(np.array([1.0, 1.0]), np.array([-4.0, 0.5]), np.eye(2))
    assert h == 3 and np.array_equal(nxt, [0.5, 1.0625])
    assert L.rel_change(np.array([1.0, 2.0]), np.array([3.0, 2.0])) == 1.0


@pytest.mark.parametrize("case", NULL_CASES, ids=lambda s: "-".join(map(str, s)))
def test_conditions_the_null_model_tests_rely_on(case):
    """Every input of test_gpu_lmm.py's null-model tests: the dense-solve fit converges inside max_iter, in the interior (both
    components above 0.05 s2), with kappa(V) <= 1e3 along the trajectory; the PCG form takes the same number of iterations; and
    the last change of tau and the one before are clear of tol_reml by a thousand times the distance of the two forms, so that
    an implementation within that distance stops at the same iteration."""
    n, c = case
    phi, y, Z, G = null_inputs(n, c)
    fd = L.reml(phi, y, Z, G=G, solver="dense", tol_reml=TOL_REML, kappa=True)
    fp = L.reml(phi, y, Z, G=G, solver="pcg", tol_reml=TOL_REML)
    assert fd.state == 1 and fd.iters < 50 and fp.state == 1 and fp.iters == fd.iters
    assert np.all(fd.tau > 0.05 * fd.s2) and fd.kappa <= 1e3, (fd.tau, fd.s2, fd.kappa)
    dist = float(np.max(np.abs(fd.path - fp.path) / np.abs(fd.path)))
    changes = [L.rel_change(fd.path[k + 1], fd.path[k]) for k in range(fd.iters)]
    assert changes[-1] <= TOL_REML - 1e3 * dist and all(ch >= TOL_REML + 1e3 * dist for ch in changes[:-1]), (changes, dist)
    assert fp.worst <= 1e-10 + 6e-10 and 0.0 < fd.h2 < 1.0 and np.all(fd.ratios > 0.0)
    print(case, "iters", fd.iters, "tau", fd.tau, "h2", round(fd.h2, 4), "kappa", round(fd.kappa, 1), "gamma", round(fd.gamma, 4), "pcg - dense", f"{dist:.2e}")


def test_boundary_input_reaches_the_boundary_rule():
    phi, y, Z, G = null_inputs(300, 1, noise=True, seed=0)
    fd = L.reml(phi, y, Z, G=G, solver="dense")
    e0, s2, _ = L.ols(y, Z)
    assert fd.state == 2 and fd.tau[1] == 0.0 and fd.tau[0] == s2 and fd.iters < 50
    assert np.allclose(fd.py, e0 / s2, rtol=0, atol=1e-12) and np.allclose(fd.ratios, 1.0 / s2, rtol=1e-12, atol=0)
    fp = L.reml(phi, y, Z, G=G, solver="pcg")
    assert fp.state == 2 and fp.iters == fd.iters
    # the iterate before the last is clear of the threshold, and a step can shrink it tenfold: far below
    assert 1.5e-8 * s2 < fd.path[-2, 1] < 5e-8 * s2


def test_hutchinson_against_exact_traces():
    """The Monte-Carlo error of 30 probes, a property of the method: printed and recorded, no bound asserted
    beyond both fits converging."""
    phi, y, Z, G = null_inputs(300, 3)
    fh = L.reml(phi, y, Z, G=G, solver="dense")
    fe = L.reml(phi, y, Z, G=G, solver="dense", exact=True)
    assert fh.state == 1 and fe.state == 1
    print(f"n = 300, c = 3, 30 probes: tau {fh.tau} against exact traces {fe.tau}: relative difference {np.abs(fh.tau - fe.tau) / fe.tau}, "
          f"h2 {fh.h2:.4f} against {fe.h2:.4f}, gamma {fh.gamma:.4f} against {fe.gamma:.4f}")


def test_null_entry_points_are_declared_and_exported(mih):
    from mendeliht_amd import api
    header = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"^int\s+(mih_\w+)\s*\(", header, flags=re.M))
    for sym in ("mih_lmm_null", "mih_neglog10p"):
        assert sym in declared and sym in api.exported_symbols()
        getattr(C.CDLL(mih.library_path()), sym)
    for cls in (mih.SnpLinAlg, mih.DosageMatrix):
        assert callable(cls.lmm_null) and "x.assoc(y, z, kinship=null)" in cls.lmm_null.__doc__
    assert not hasattr(mih.DenseMatrix, "lmm_null") and "kinship" in mih.DenseMatrix.assoc.__doc__
    # the tail function is host code: it answers without a device
    z = np.array([0.0, 1.959963984540054, -40.0, np.nan])
    got = mih.neglog10p(z)
    assert got[0] == 0.0 and abs(got[1] - np.log10(20.0)) < 1e-12 and 340 < got[2] < 360 and np.isnan(got[3])
    # the argument refusals of mih_lmm_null come before any device call
    lib = mih.lib()
    buf = np.full(64, -7.0)
    i32, i64 = C.c_int32(-7), C.c_int64(-7)
    vp = buf.ctypes.data_as(C.c_void_p)

    def call(c=1, probes=30, R=0, tol=1e-5, max_iter=50, cg_tol=1e-10, cg_max_iter=500):
        d = [C.c_double(-7.0) for _ in range(3)]
        rc = lib.mih_lmm_null(None, None, 0, 0, vp, vp, c, probes, 0, vp, R, tol, max_iter, cg_tol, cg_max_iter, vp, vp, vp, C.byref(d[0]), vp, vp,
                              C.byref(d[1]), vp, C.byref(i32), C.byref(i32), C.byref(i64), C.byref(d[2]))
        msg = C.create_string_buffer(512)
        lib.mih_last_error(msg, 512)
        return rc, msg.value.decode(errors="replace")

    for kw, word in ((dict(c=0), "covariates"), (dict(probes=0), "probes"), (dict(probes=65), "probes"), (dict(c=100, probes=30), "probes"),
                     (dict(R=129), "R must"), (dict(R=-1), "R must"), (dict(tol=float("nan")), "tol_reml"), (dict(cg_tol=-1.0), "cg_tol"),
                     (dict(max_iter=0), "max_iter"), (dict(cg_max_iter=0), "cg_max_iter"), (dict(), "null matrix handle")):
        rc, msg = call(**kw)
        assert rc == BAD_ARG and word in msg, (kw, rc, msg)
        assert np.all(buf == -7.0) and i32.value == -7 and i64.value == -7, kw


def test_host_algebra_harness(tmp_path):
    """tests/lmm_host_harness.cpp: csrc/lmm_host.h (no HIP in it) built with plain g++ and run on inputs with known answers."""
    import subprocess
    exe = tmp_path / "lmm_host_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mendeliht.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lmm_host_harness.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
