"""The host algebra of pca() (csrc/sym_eig.h: the cyclic Jacobi eigen-solver, the rank rule, the sign rule) against numpy, through
the stand-alone program tests/sym_eig_harness.cpp built with plain g++ (no HIP, no GPU, nothing loaded into python).

Tolerances, derived: u = 2^-53.  Jacobi is backward stable: the computed eigenvalues of an order-b matrix are those of A + dA
with |dA|_F <= c b u |A|_F, so by Weyl every one is within 8 b u |A|_F of an exact one (the constant 8 covers the sweeps and
eigh's own error of the same form).  V is orthogonal to the same order, and |A V - V diag(w)|_F is within that bound times
sqrt(b) at most (one column each).  An invariant subspace is compared through its projector: by Davis-Kahan the two
projectors differ by at most twice the backward errors over the gap that separates the cluster from the rest."""
import os
import subprocess

import numpy as np
import pytest

import pca_spec as P
from conftest import ROOT

U = 2.0 ** -53
CSRC = os.path.join(ROOT, "mendeliht.jl_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("sym_eig")
    exe = d / "sym_eig_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "sym_eig_harness.cpp"), "-o", str(exe)])

    def run(cmd, vec, n):
        fin, fout = d / "in.bin", d / "out.bin"
        with open(fin, "wb") as f:
            f.write(np.int64(n).tobytes())
            f.write(np.ascontiguousarray(vec, dtype=np.float64).tobytes())
        r = subprocess.run([str(exe), cmd, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return np.fromfile(fout, dtype=np.float64)
    return run


def eig(run, a):
    n = a.shape[0]
    out = run("eig", a, n)
    assert out.size == n + n * n + 1
    return out[:n], out[n:n + n * n].reshape(n, n), int(out[-1])


def check_decomposition(a, w, v):
    b = a.shape[0]
    fro = np.linalg.norm(a)
    tol = 8.0 * b * U * fro
    want = np.linalg.eigvalsh(a)[::-1]
    assert np.all(np.diff(w) <= 0.0)                                       # descending
    assert np.max(np.abs(w - want)) <= tol + 1e-300, (b, float(np.max(np.abs(w - want))), tol)
    assert np.max(np.abs(v.T @ v - np.eye(b))) <= 8.0 * b * U, b
    assert np.linalg.norm(a @ v - v * w[None, :]) <= np.sqrt(b) * tol + 1e-300, b


@pytest.mark.parametrize("b", [1, 2, 15, 16, 17, 64, 128])
def test_random_symmetric_matrices(harness, b):
    rng = np.random.default_rng(100 + b)
    m = rng.standard_normal((b, b))
    a = (m + m.T) / 2.0
    w, v, sweeps = eig(harness, a)
    assert 0 <= sweeps <= 20
    check_decomposition(a, w, v)


def test_only_the_lower_triangle_is_read(harness):
    rng = np.random.default_rng(7)
    m = rng.standard_normal((9, 9))
    a = (m + m.T) / 2.0
    dirty = np.tril(a) + np.triu(np.full((9, 9), 1e30), 1)
    w0, v0, _ = eig(harness, a)
    w1, v1, _ = eig(harness, dirty)
    assert np.array_equal(w0, w1) and np.array_equal(v0, v1)


def test_rank_deficient_gram_matrix(harness):
    """Y is 200 x 16 of rank 5: G = Y'Y has 5 eigenvalues of the order of |G| and 11 within the backward error of 0, which the
    rank rule drops when they are at or below 2^-52 d_1 -- and whatever it keeps, the leading 5 are right."""
    rng = np.random.default_rng(8)
    y = rng.standard_normal((200, 5)) @ rng.standard_normal((5, 16))
    g = y.T @ y
    w, v, _ = eig(harness, g)
    check_decomposition(g, w, v)
    tol = 8.0 * 16 * U * np.linalg.norm(g)
    assert np.all(np.abs(w[5:]) <= tol) and w[4] > 1e-3 * w[0]
    r = int(harness("rank", w, 16)[0])
    assert r == P.rank_rule(w) and 5 <= r <= 16
    lead = v[:, :5]
    exact = np.linalg.svd(y, full_matrices=False)[2][:5].T              # the row space of Y
    assert np.linalg.norm(lead @ lead.T - exact @ exact.T) <= 4.0 * tol / (w[4] - tol)


def test_repeated_eigenvalue_gives_the_invariant_subspace(harness):
    """diag(5, 5, 5, 2, 1, 1, -3) in a random orthogonal basis: the eigenvectors of a repeated eigenvalue are any basis of its
    eigenspace, so the projectors are compared."""
    rng = np.random.default_rng(9)
    lam = np.array([5.0, 5.0, 5.0, 2.0, 1.0, 1.0, -3.0])
    q = np.linalg.qr(rng.standard_normal((7, 7)))[0]
    a = (q * lam[None, :]) @ q.T
    a = (a + a.T) / 2.0
    w, v, _ = eig(harness, a)
    check_decomposition(a, w, v)
    tol = 8.0 * 7 * U * np.linalg.norm(a)
    for lo, hi, gap in ((0, 3, 3.0), (3, 4, 1.0), (4, 6, 1.0), (6, 7, 4.0)):
        mine, exact = v[:, lo:hi], q[:, lo:hi]
        assert np.linalg.norm(mine @ mine.T - exact @ exact.T) <= 4.0 * tol / gap, (lo, hi)


def test_zero_and_diagonal_matrices_need_no_sweep(harness):
    w, v, sweeps = eig(harness, np.zeros((6, 6)))
    assert sweeps == 0 and np.all(w == 0.0) and np.array_equal(v, np.eye(6))
    w, v, sweeps = eig(harness, np.diag([1.0, 3.0, 2.0]))
    assert sweeps == 0 and np.array_equal(w, [3.0, 2.0, 1.0])
    assert np.array_equal(v, np.eye(3)[:, [1, 2, 0]])


def test_a_nan_is_answered_with_nans(harness):
    a = np.eye(4)
    a[2, 1] = a[1, 2] = np.nan
    w, v, sweeps = eig(harness, a)
    assert sweeps == 61 and np.isnan(w).all() and np.isnan(v).all()


def test_rank_rule(harness):
    eps = 2.0 ** -52
    cases = [([4.0, 1.0, 4.0 * eps, 0.0], 2),                           # d_i == 2^-52 d_1 is dropped: strictly above survives
             ([4.0, 1.0, 4.0 * eps * (1 + 2 * eps), 0.0], 3),
             ([1.0], 1), ([0.0, 0.0], 0), ([-1.0], 0), ([float("nan"), 1.0], 0), ([3.0, 2.0, -1e-20], 2),
             ([1e-300, 1e-300], 2)]
    for d, want in cases:
        assert int(harness("rank", np.array(d), len(d))[0]) == want == P.rank_rule(d), d


def test_sign_rule(harness):
    cases = [[1.0, -3.0, 2.0], [1.0, 3.0, -2.0], [-2.0, 2.0, 1.0], [2.0, -2.0], [0.0, 0.0], [-0.0, -1e-300], [-7.0]]
    for x in cases:
        got = harness("sign", np.array(x), len(x))
        want = P.sign_rule(np.array(x))
        assert np.array_equal(got, want), x
        piv = int(np.argmax(np.abs(got)))
        assert got[piv] >= 0.0 and np.array_equal(np.abs(got), np.abs(x))
    assert np.array_equal(harness("sign", np.array([-2.0, 2.0, 1.0]), 3), [2.0, -2.0, -1.0])       # the lowest index on a tie
