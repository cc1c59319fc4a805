"""csrc/normal_tail.h -- -log10 of the two-sided normal tail of a z statistic, the one function mih_assoc_score evaluates on the
host -- compiled into tests/normal_tail_harness.cpp with g++ (plainly, and once more under -fsanitize=address,undefined as a
stand-alone program) and compared with scipy.special.log_ndtr: -log10 p = -(log 2 + log_ndtr(-|z|)) / log 10.

Grid: |z| from 0 to 200 -- 0, powers of ten from 1e-300 up, 2001 even steps of 0.1, and the switch between libm's erfc and the
continued fraction (|z| = 25 sqrt 2 = 35.3553...) with its neighbours on both sides, and the switch to log1p at |z| = sqrt(2) / 2.

Tolerance: relative 4 x the worst error MEASURED on the machine this was written on, the margin covering libm differences between
machines.  Measured worst relative error against scipy over |z| >= 0.5: 6.96e-16 (against 50-digit mpmath the function is within
6.3e-16 over the whole grid): RTOL = 4 x 7.0e-16.  Below |z| = 0.5 the REFERENCE cancels -- log 2 + log_ndtr(-|z|) -> 0 as the
difference of two numbers near 0.69, each a few ulp of 2^-53 off: scipy itself is 4.9e-13 away from mpmath at |z| = 1e-3 -- so
there the reference is granted its own absolute error, 8 x 2^-53 / log 10, on top; and at |z| <= 1e-9, where that allowance
would be all there is, the function is held to RTOL against the series -log10 p = (|z| sqrt(2 / pi) + z^2 / pi) / log 10 + O(z^3)."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MEASURED = 7.0e-16
RTOL = 4 * MEASURED
SWITCH = 25.0 * math.sqrt(2.0)


def grid():
    z = [0.0] + [10.0 ** e for e in range(-300, -2, 7)] + [1e-3, 1e-2] + [0.1 * k for k in range(1, 2001)]
    for c in (SWITCH, math.sqrt(2.0) / 2.0):
        z += [np.nextafter(c, 0.0), c, np.nextafter(c, 1e9), c - 1e-9, c + 1e-9, c - 1e-3, c + 1e-3]
    z += [40.0, 37.5, 38.0, 39.0, 199.999]
    return np.array(sorted(set(float(v) for v in z)))


def build(tmp_path, sanitize):
    exe = tmp_path / ("tail_san" if sanitize else "tail")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mendeliht.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "normal_tail_harness.cpp"), "-o", str(exe)]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.check_call(cmd)
    return exe


def run(exe, z):
    r = subprocess.run([str(exe)], input="\n".join(repr(float(v)) for v in z) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return np.array([float(t) for t in r.stdout.split()])


def reference(z):
    from scipy.special import log_ndtr
    return -(math.log(2.0) + log_ndtr(-z)) / math.log(10.0)


@pytest.mark.parametrize("sanitize", [False, True])
def test_neglog10p_against_scipy(tmp_path, sanitize):
    z = grid()
    exe = build(tmp_path, sanitize)
    got = run(exe, z)
    ref = reference(z)
    assert got.shape == ref.shape and got[0] == 0.0 and np.isfinite(got).all()
    big = z >= 0.5
    err = np.abs(got - ref)[big] / ref[big]
    print(f"worst relative error against scipy over |z| >= 0.5: {err.max():.3g} at |z| = {z[big][err.argmax()]!r}")
    assert err.max() <= RTOL
    assert (np.abs(got - ref)[~big] <= RTOL * ref[~big] + 8 * 2.0 ** -53 / math.log(10.0)).all()
    tiny = (z > 0) & (z <= 1e-9)                # (the next term of the series is relatively z^2)
    series = (z[tiny] * math.sqrt(2.0 / math.pi) + z[tiny] ** 2 / math.pi) / math.log(10.0)
    assert (np.abs(got[tiny] - series) <= RTOL * series).all()
    assert (np.diff(got) >= 0).all()               # never falling over the whole grid, across both switches and between neighbouring doubles
    at40 = run(exe, [40.0])[0]                     # p = 7.3e-350 is no double; its logarithm is (the one-sided tail would be 349.4)
    assert abs(at40 - 349.136) < 1e-3 and abs(at40 - reference(np.array([40.0]))[0]) <= RTOL * at40


def test_sign_nan_and_infinity(tmp_path):
    got = run(build(tmp_path, False), [-3.0, 3.0, float("nan"), float("inf"), -float("inf"), -40.0])
    assert got[0] == got[1] and np.isnan(got[2]) and got[3] == np.inf and got[4] == np.inf and abs(got[5] - 349.136) < 1e-3
