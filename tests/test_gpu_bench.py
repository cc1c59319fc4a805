"""bench.py's plain run on a small matrix: the result line's fields, exactly --steps timed steps, and --dump-outputs writing the
last step's model and figures, the same bits on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
           "--n", "20000", "--p", "60000", "--k", "20", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_bench_line_and_dumped_outputs_repeat_bit_for_bit(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        line = _bench(d)
        assert line["steps"] == 5 and line["warmup"] == 2
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["unit"] == "iterations/s" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0 and line["ms_per_step"] == pytest.approx(1e3 / line["value"], rel=1e-9)
        for key in ("cv_iht", "mv", "dense", "cpu_baseline", "cpu_baseline_cv"):     # the secondary objects run with --full only
            assert key not in line, key
        assert "host_driven_steps_same_box" not in line["config"] and "without_the_measurement_hook" not in line["config"]
        files = sorted(os.listdir(d))
        assert files == ["backtracks.npy", "beta.npy", "c.npy", "logl.npy", "tol.npy"], files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(v.dtype == np.float64 for v in arrays.values())
        assert arrays["beta"].shape == (60000,) and 0 < np.count_nonzero(arrays["beta"]) <= 20
        assert arrays["logl"][0] == line["config"]["final_logl"]
        assert arrays["backtracks"][0] == line["config"]["backtracks_in_timed_steps"]
        runs.append(arrays)
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name
