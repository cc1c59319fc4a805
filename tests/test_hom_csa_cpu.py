"""The carry-save positional counter k_xtv_hom adds its lists with (HomCsa, csrc/score_image.h) against the division-loop
definition of the balanced digits and against HomSum, term by term, chunk by chunk and in the kernel's own cadence.
tests/hom_csa_harness.cpp is a stand-alone program built with plain g++ under AddressSanitizer and UBSan (no HIP, no GPU,
nothing loaded into python)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "mendeliht.jl_amd", "csrc")


def test_positional_counts_under_sanitizers(tmp_path):
    exe = tmp_path / "hom_csa_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "hom_csa_harness.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("ok lengths 0..400", "ok flush cadence", "ok field bound", "ok padding", "ok sub-slices", "ok 2^22 terms"):
        assert line in r.stdout, r.stdout + r.stderr
