"""tests/xb_spec.py (the statement SnpLinAlg.transpose / xb / score are held to) against exact rational arithmetic, and the
register transposition of k_transpose_tiles (csrc/transpose_bits.h) against its definition.  No GPU: the transposition is checked
by tests/transpose_bits_harness.cpp, a stand-alone program built with plain g++ under AddressSanitizer and UBSan (nothing is loaded
into python)."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import xb_spec as S
from conftest import ROOT

CSRC = os.path.join(ROOT, "mendeliht.jl_amd", "csrc")
FLAGS = [(c, s, i) for c in (0, 1) for s in (0, 1) for i in (0, 1)]


def random_codes(rng, n, p, missing):
    codes = rng.binomial(2, rng.uniform(0.05, 0.5, size=p)[None, :], size=(n, p)).astype(np.int64)
    if missing:
        codes[rng.random((n, p)) < missing] = -1
    return codes


CASES = {
    "no missing": lambda rng: random_codes(rng, 40, 70, 0.0),
    "missing": lambda rng: random_codes(rng, 40, 70, 0.08),
    "small": lambda rng: random_codes(rng, 7, 33, 0.1),
    "one snp": lambda rng: random_codes(rng, 17, 1, 0.2),
}


def _with(codes, snp=None, sample=None):
    codes = codes.copy()
    if snp is not None:
        codes[:, snp] = -1
    if sample is not None:
        codes[sample, :] = -1
    return codes


CASES["all-missing sample"] = lambda rng: _with(random_codes(rng, 23, 37, 0.05), sample=5)
CASES["all-missing snp"] = lambda rng: _with(random_codes(rng, 23, 37, 0.05), snp=11)
CASES["both"] = lambda rng: _with(random_codes(rng, 23, 37, 0.05), snp=0, sample=22)


def _worst(got, exact, bound):
    """max |got - exact| / bound over the finite entries; the NaN patterns must agree."""
    worst = 0.0
    for i in range(exact.shape[0]):
        for t in range(exact.shape[1]):
            if exact[i, t] is None:
                assert np.isnan(got[i, t]), (i, t)
                continue
            assert np.isfinite(got[i, t]), (i, t)
            err = abs(Fraction(float(got[i, t])) - exact[i, t])
            if err:
                assert bound[i, t] > 0, (i, t)
                worst = max(worst, float(err / Fraction(float(bound[i, t]))))
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_spec_against_rationals(name):
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    codes = CASES[name](rng)
    n, p = codes.shape
    B = rng.standard_normal((p, 3))
    B[:, 2] *= 10.0 ** rng.integers(-6, 7, size=p)                   # a wide dynamic range in one column
    assert np.array_equal(S.transpose_codes(S.transpose_codes(codes)), codes)
    assert S.transpose_codes(codes).shape == (p, n)
    for flags in FLAGS:
        ex = S.exact_fraction(codes, B, *flags)
        fast = S.exact(codes, B, *flags)
        for a, b in zip(ex.ravel(), fast.ravel()):                   # the integer-limb route is the same rational number
            assert (a is None) == (b is None)
            assert a is None or a == b, flags
        for digits in (None, 428, 1316):
            bound = S.bound(codes, B, flags, digits)
            assert bound.shape == (n, 3) and np.all(bound >= 0)
            # numpy's own f64 product of the standardised matrix lies inside the bound of the exact value
            worst = _worst(S.xb(codes, B, *flags), ex, bound)
            assert worst <= 1.0, (name, flags, digits, worst)
    # ... and the bound is no blank cheque: a relative error of 2^-36 in the largest weight is outside it
    flags = (0, 1, 0)
    ex = S.exact_fraction(codes, B, *flags)
    j = int(np.argmax(np.abs(B[:, 0]) * (np.where(codes < 0, 0, codes).sum(axis=0) > 0)))
    Bp = B.copy()
    Bp[j, 0] *= 1.0 + 2.0 ** -36
    rows = np.flatnonzero(codes[:, j] > 0)
    if rows.size and not any(v is None for v in ex.ravel()):
        got = S.exact_fraction(codes, Bp, *flags)
        bound = S.bound(codes, B, flags)
        err = [abs(got[i, 0] - ex[i, 0]) for i in rows]
        assert any(e > Fraction(float(bound[i, 0])) for e, i in zip(err, rows))


def test_one_dimensional_b_and_flags_off():
    rng = np.random.default_rng(5)
    codes = random_codes(rng, 19, 21, 0.1)
    b = rng.standard_normal(21)
    assert S.xb(codes, b, 0, 0, 0).shape == (19,)
    assert np.array_equal(S.xb(codes, b, 0, 0, 0), np.where(codes < 0, 0, codes).astype(np.float64) @ b)


def test_score_hand_computed():
    #            snp0 snp1 snp2 snp3
    codes = np.array([[0, 1, 2, -1],
                      [1, -1, 0, 2],
                      [2, 1, -1, 0]])
    w = np.array([0.5, -1.0, 2.0, 4.0])
    # mean dosages over the observed genotypes: 1, 1, 1, 1
    assert np.array_equal(S.mu_sigma(codes)[0], [1.0, 1.0, 1.0, 1.0])
    want = np.array([0 * 0.5 - 1.0 + 4.0 + 4.0 * 1.0, 0.5 - 1.0 * 1.0 + 0.0 + 8.0, 1.0 - 1.0 + 2.0 * 1.0 + 0.0])
    assert np.array_equal(S.score(codes, w), want)
    assert np.array_equal(S.score(codes, w, average=True), want / 8.0)
    # weights for SNPs 1 and 3 only
    want13 = np.array([-1.0 + 4.0, -1.0 + 8.0, -1.0 + 0.0])
    assert np.array_equal(S.score(codes, [-1.0, 4.0], cols=[1, 3]), want13)
    assert np.array_equal(S.score(codes, [-1.0, 4.0], cols=np.array([False, True, False, True]), average=True), want13 / 4.0)


def test_transposition_of_2bit_fields_under_sanitizers(tmp_path):
    exe = tmp_path / "transpose_bits_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "transpose_bits_harness.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("ok random fields", "ok single fields at 256 positions", "ok all ones", "ok twice is the identity"):
        assert line in r.stdout, r.stdout + r.stderr
