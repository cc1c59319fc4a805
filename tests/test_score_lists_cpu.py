"""Where the 16-byte chunks of a slot group's exception lists live (hom_chunk_base, hom_chunk_rank, hom_chunk_slot of
csrc/score_image.h): a bijection onto the group's block, the chunks of one index in one contiguous run in lane order, run after
run.  tests/score_lists_harness.cpp is a stand-alone program built with plain g++ under AddressSanitizer and UBSan (no HIP, no GPU,
nothing loaded into python)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "mendeliht.jl_amd", "csrc")


def test_chunk_placement_under_sanitizers(tmp_path):
    exe = tmp_path / "score_lists_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "score_lists_harness.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("ok empty and single lanes", "ok equal and monotone", "ok one long lane", "ok random"):
        assert line in r.stdout, r.stdout
