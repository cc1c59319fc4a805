"""csrc/scalar_log.h -- the one logarithm the loglikelihood's closed forms take, written so that the host and the device round it
alike -- against an exact reference, through the stand-alone program tests/scalar_log_harness.cpp built with plain g++ (no HIP, no
GPU, nothing loaded into python).  The bound: the algorithm's published error is below 1 ulp; the reference is numpy's log
evaluated in extended precision (np.longdouble, 64-bit mantissa: its own error is 2^-11 ulp of a double), so |got - ref| <= 1 ulp
of the result is asserted, not measured."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "mendeliht.jl_amd", "csrc")


@pytest.fixture(scope="module")
def scalar_log(tmp_path_factory):
    d = tmp_path_factory.mktemp("scalar_log")
    exe = d / "scalar_log_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "scalar_log_harness.cpp"), "-o", str(exe)])

    def run(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        fin, fout = d / "in.bin", d / "out.bin"
        with open(fin, "wb") as f:
            f.write(np.int64(x.size).tobytes())
            f.write(x.tobytes())
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return np.fromfile(fout, dtype=np.float64)
    return run


def _within_one_ulp(got, x):
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended-precision long double"
    ref = np.log(x.astype(np.longdouble))
    err = np.abs(got.astype(np.longdouble) - ref)
    ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble)
    bad = np.flatnonzero(err > ulp)
    assert bad.size == 0, (x[bad][:5], got[bad][:5], (err[bad] / ulp[bad])[:5])


def test_random_arguments_over_the_whole_range(scalar_log):
    rng = np.random.default_rng(41)
    x = np.concatenate([np.exp(rng.uniform(-700.0, 700.0, 200_000)), rng.uniform(0.5, 2.0, 200_000),
                        1.0 + rng.uniform(-1e-6, 1e-6, 50_000), rng.integers(1, 2 ** 52, 20_000).astype(np.float64) * 2.0 ** -1074])
    _within_one_ulp(scalar_log(x), x)


def test_edges_of_the_reduction_and_special_values(scalar_log):
    r2 = np.sqrt(2.0)
    near = lambda v: [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]
    x = np.array(near(1.0) + near(r2) + near(r2 / 2) + near(2.0) + near(0.5) + near(np.finfo(np.float64).tiny)
                 + [np.finfo(np.float64).max, 2.0 ** -1074, 2.0 ** -1073, 2.0 ** 600, 2.0 ** -600, np.e, 10.0])
    got = scalar_log(x)
    _within_one_ulp(got, x)
    assert got[1] == 0.0 and got[list(x).index(2.0 ** 600)] == pytest.approx(600 * np.log(2.0), rel=1e-15)
    with np.errstate(all="ignore"):
        sp = scalar_log(np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan]))
    assert sp[0] == -np.inf and sp[1] == -np.inf and np.isnan(sp[2]) and sp[3] == np.inf and np.isnan(sp[4]) and np.isnan(sp[5])
    # monotone across the seam of the reduction at sqrt(2)
    seam = r2 + np.arange(-2000, 2001) * np.spacing(r2)
    assert np.all(np.diff(scalar_log(seam)) >= 0.0)
