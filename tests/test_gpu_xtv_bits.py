"""The raw f64 output of X'r, bit for bit, against digests recorded from the commit BEFORE csrc/xtv.hip was split by matrix kind
(tests/golden/xtv_bits.json).  The other X'r tests compare kernel families with each other or with exact arithmetic within a bound;
a slip made alike in every family -- in a shared slice helper, ring feed or digit-column sum -- would pass them.  The pass is
bit-reproducible for a given row slicing, so the sha256 of `SnpLinAlg.xtv`'s bytes is a legitimate expectation (two fresh
processes of the recording commit gave the same digests for every case here).

Cases: every residual count that changes the pass plan on the shipped 1000 x 10000 example (one row slice) in the default format
and in each explicit one; a 16400 x 70 synthetic matrix with missing entries, where nbp = 129 gives 16 row slices of 9 blocks
with slice 14 short, slice 15 EMPTY, a ragged third column group and idle waves; the dense f64 and the 16-bit dosage pass.

Record again (only from a commit whose bits are the reference):  python tests/test_gpu_xtv_bits.py > tests/golden/xtv_bits.json
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "xtv_bits.json")
M = 19

# (matrix, xtv_digits or None for the default format, residual counts)
CASES = (
    ("normal", None, (1, 2, 3, 4, 7, 10, 13, 16, 19)),      # k_xtv_dma16 with 1..6 operands, half and full, flat packing
    ("normal", 4908, (1, 3, 5, 8)),
    ("normal", 1316, (1, 3, 5, 8)),                         # k_xtv_dma (one operand), k_xtv_mfma_lds with 2, 3 and 4
    ("normal", 428, (1, 2, 3, 4)),                          # the single-fit format; one residual per operand
    ("normal", 1308, (4,)),
    ("sliced", None, (1, 19)),
    ("sliced", 1316, (4,)),
    ("dense", None, (1, 3)),
    ("dosage", None, (1, 3)),
)
IDS = [f"{mat}-{dg or 'default'}-m{m}" for mat, dg, ms in CASES for m in ms]


def residuals(n):
    return np.random.default_rng(1).standard_normal((n, M)) * np.exp(np.random.default_rng(2).uniform(-3, 3, M))


def matrices(mih):
    """name -> (matrix, its residuals); built once and left unchanged"""
    bed = mih.read_bed(os.path.join(ROOT, "tests", "fixtures", "normal.bed"), 1000)
    mats = {
        "normal": mih.SnpLinAlg(bed, 1000, center=True, scale=True, impute=True),
        "sliced": mih.SnpLinAlg.synthetic(16400, 70, seed=3, missing_rate=0.02),
        "dense": mih.DenseMatrix(np.random.default_rng(5).standard_normal((1002, 37))),
        "dosage": mih.DosageMatrix.synthetic(1002, 37, seed=4, missing_rate=0.02),
    }
    return {k: (x, residuals(x.n)) for k, x in mats.items()}


def digest(mats, mat, dg, m):
    x, r = mats[mat]
    out = x.xtv(r[:, :m], xtv_digits=dg)
    assert out.shape == (x.p, m) and out.dtype == np.float64
    return hashlib.sha256(np.asfortranarray(out).tobytes(order="F")).hexdigest()


@pytest.fixture(scope="module")
def mats(mih):
    return matrices(mih)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest(golden):
    assert sorted(golden) == sorted(IDS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(mat, dg, m) for mat, dg, ms in CASES for m in ms], ids=IDS)
def test_xtv_bits_equal_the_recorded_ones(mats, golden, case):
    mat, dg, m = case
    assert digest(mats, mat, dg, m) == golden[f"{mat}-{dg or 'default'}-m{m}"]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import mendeliht_amd
    ms_ = matrices(mendeliht_amd)
    json.dump({f"{mat}-{dg or 'default'}-m{m}": digest(ms_, mat, dg, m) for mat, dg, ms in CASES for m in ms}, sys.stdout, indent=1)
    print()
