"""Column shards of a BGEN file streamed rank by rank (dist.read_bgen_shard): W processes, each with its block of variants,
end on the single-process denominator with the single read's numerators, and the column-sharded fit on them reproduces the
single-process fit on parse_genotypes.  The GPU box has one device, so the ranks share it and talk over gloo."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from bgen_files import write_probs
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture(scope="module")
def shard_files(tmp_path_factory):
    """8-bit BGEN, 96 variants: 0..31 fractional (own denominator 255), 32..63 multiples of 85 (3), 64..95 hard calls (1) --
    at world 2 and 3 the last rank's block holds only hard calls; and a trait with 5 planted effects."""
    d = tmp_path_factory.mktemp("bgen_shards")
    rng = np.random.default_rng(21)
    n, p = 900, 96
    kaa = rng.integers(0, 256, (n, p))
    kab = (rng.random((n, p)) * (256 - kaa)).astype(np.int64)
    kaa[:, 32:64], kab[:, 32:64] = kaa[:, 32:64] // 85 * 85, kab[:, 32:64] // 85 * 85
    g = rng.binomial(2, 0.3, (n, 32))
    kaa[:, 64:], kab[:, 64:] = np.where(g == 0, 255, 0), np.where(g == 1, 255, 0)
    miss = rng.random((n, p)) < 0.02
    write_probs(str(d / "s.bgen"), kaa, kab, miss, 8)
    d_ = np.where(miss, np.nan, (2 * (255 - kaa - kab) + kab) / 255)
    m = np.nanmean(d_, axis=0)
    xs = np.where(miss, 0.0, (d_ - m) / np.sqrt(m * (1 - m / 2)))
    beta = np.zeros(p)
    beta[[3, 40, 66, 70, 90]] = [0.6, -0.5, 0.4, 0.7, -0.45]
    np.savetxt(d / "y.txt", xs @ beta + rng.standard_normal(n))
    return d


@pytest.mark.parametrize("world", [2, 3])
def test_bgen_shards_match_the_single_read_and_fit(mih, shard_files, tmp_path, world):
    d = shard_files
    out = str(tmp_path / "res")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "bgen_sharded_worker.py"), out, str(d / "s.bgen"), str(d / "y.txt"), "5"]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="4"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    x, samples, chrom, pos, ids, ref, alt = mih.parse_genotypes(str(d / "s.bgen"))
    assert x.denom == 255
    whole = x.export()
    y = np.loadtxt(d / "y.txt")
    one = mih.fit_iht(y, x, None, k=5, verbose=False)
    res = [json.load(open(f"{out}.r{k}.json")) for k in range(world)]
    assert [q["off"] for q in res] == sorted(q["off"] for q in res) and res[0]["off"] == 0
    assert sum(q["p"] for q in res) == 96 and all(q["p_global"] == 96 for q in res)
    from mendeliht_amd.genotypes import read_bgen_device
    last = res[-1]
    assert read_bgen_device(str(d / "s.bgen"), variants=range(last["off"], 96))[0].denom == 1     # its own grid: hard calls
    for q in res:
        assert q["denom"] == 255 and q["world"] == world and q["n_samples"] == 900
        assert q["ids"] == ids[q["off"]:q["off"] + q["p"]]
        assert np.array_equal(np.load(f"{out}.r{q['rank']}.npy"), whole[:, q["off"]:q["off"] + q["p"]])
        assert q["support"] == np.flatnonzero(one.beta).tolist() and q["iter"] == one.iter
        np.testing.assert_allclose(q["beta"], one.beta[one.beta != 0], rtol=0, atol=1e-9)
        np.testing.assert_allclose(q["logl_trace"], one.trace["logl"], rtol=1e-11)
        assert q["beta"] == res[0]["beta"] and q["logl"] == res[0]["logl"]
