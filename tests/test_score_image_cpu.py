"""The two host-callable identities of the score image (csrc/score_image.h) against their plain definitions: the row-to-bit map
of the one-bit tile and the SWAR sum of base-4 digits.  tests/score_image_harness.cpp is a stand-alone program built with plain
g++ under AddressSanitizer and UBSan (no HIP, no GPU, nothing loaded into python)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "mendeliht.jl_amd", "csrc")


def test_row_map_and_digit_sums_under_sanitizers(tmp_path):
    exe = tmp_path / "score_image_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "score_image_harness.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok row map" in r.stdout and "ok digit sums" in r.stdout
