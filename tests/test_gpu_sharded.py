"""Column-sharded single fit (one fit over several GPUs): W processes, each with its block of
SNP columns, must reproduce the single-process fit -- same support, same iteration log, beta to 1e-9.
The GPU box has one device, so the ranks share it and talk over gloo; on a multi-GPU node the same
code runs with backend nccl (RCCL) and one device per rank."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, SweepTally

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_fit_matches_single_process(tmp_path, world):
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "sharded_worker.py"), str(out)]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["world"] == world
    others = [json.load(open(str(out) + f".r{k}"))["cases"] for k in range(1, world)]
    cv = res["cases"].pop("cv_grid")
    assert cv["distributed"] == cv["single"]                               # (fold,k) grid over the ranks == one process
    for oc in others:
        assert oc.pop("cv_grid")["distributed"] == cv["single"]
    # multivariate traits over the column shards (round 5): same support, iterations and backtracks as the single-process fit,
    # B / C / Sigma to rounding, the same model on every rank; the tied columns fire _choose! over the WHOLE model
    for name in ("mv_shipped", "mv_r3_cov", "mv_tiny", "mv_ties_choose"):
        case = res["cases"].pop(name)
        sh, one = case["sharded"], case["single"]
        assert sh["support"] == one["support"] and len(sh["support"]) > 0, name
        assert sh["iter"] == one["iter"] and sh["bt"] == one["bt"], name
        np.testing.assert_allclose(sh["beta"], one["beta"], rtol=0, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(sh["c"], one["c"], rtol=0, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(sh["Sigma"], one["Sigma"], rtol=1e-9, err_msg=name)
        np.testing.assert_allclose(sh["sigma_g"], one["sigma_g"], rtol=1e-9, atol=1e-12, err_msg=name)      # (a pve of 1e-36 in the tied case is zero)
        np.testing.assert_allclose(sh["logl_trace"], one["logl_trace"], rtol=1e-11, err_msg=name)
        assert sh["choose_fired"] == one["choose_fired"], name
        for oc in others:
            o2 = oc.pop(name)["sharded"]
            assert o2["support"] == sh["support"] and o2["beta"] == sh["beta"] and o2["logl"] == sh["logl"] and o2["Sigma"] == sh["Sigma"], name
    assert one["choose_fired"]                                             # (mv_ties_choose, the last of the four)
    tally = SweepTally(f"column-sharded fits, world {world}", ceiling=1, floor=10)
    for name, case in res["cases"].items():
        sh, one = case["sharded"], case["single"]
        # the Newton update of the NegBin r stops at |dr| <= 1e-6 (utilities.jl:242): rounding-level
        # differences in xb move r by up to that much, so that case is held to 1e-5 instead of 1e-9
        tb, tl = (1e-5, 1e-6) if name == "negbin_newton" else (1e-9, 1e-11)
        try:
            assert sh["support"] == one["support"], name                       # bit-exact support at fixed k
            assert sh["iter"] == one["iter"] and sh["bt"] == one["bt"], name
            np.testing.assert_allclose(sh["beta"], one["beta"], rtol=0, atol=tb, err_msg=name)
            np.testing.assert_allclose(sh["c"], one["c"], rtol=0, atol=tb, err_msg=name)
            np.testing.assert_allclose(sh["logl_trace"], one["logl_trace"], rtol=tl, err_msg=name)
            np.testing.assert_allclose(sh["tol"], one["tol"], rtol=1e4 * tb, atol=1e-12, err_msg=name)
            assert abs(sh["sigma_g"] - one["sigma_g"]) < tb, name
            assert sh["choose_fired"] == one["choose_fired"], name
        except AssertionError:
            #  a random trajectory is compared first and set aside (counted, with a ceiling) only when it differs -- and (round 6)
            # only when the single-process fit does not reproduce ITSELF on covariates scaled by a few ulps (the worker's single_nudged:
            # iterations, backtracks, support, estimates to the same tolerance); "it used up max_step backtracks" is no longer a reason
            def moved(v):
                return v["iter"] != one["iter"] or v["bt"] != one["bt"] or v["support"] != one["support"] or \
                       np.max(np.abs(np.asarray(v["beta"]) - np.asarray(one["beta"])), initial=0.0) > tb or \
                       np.max(np.abs(np.asarray(v["c"]) / v["g"] - np.asarray(one["c"])), initial=0.0) > tb
            if name.startswith("random") and any(moved(v) for v in case.get("single_nudged", [])):
                tally.set_aside("the single-process fit does not reproduce itself under ulp nudges", (name,))
                continue
            raise
        tally.ok()
        if name.startswith("group_"):        # (round 6) the doubly sparse projection over the shards did something: a model of at most J groups' worth of effects
            assert 0 < len(sh["support"]) <= {"group_random_labels": 6, "group_sorted_labels": 12, "group_vector_k": 9, "group_debias": 6}[name], (name, sh["support"])
        if name == "debias_k20_one_rank":    # what the case is about: 20 columns, every one of them rank 0's, and the refit ran
            lo, cnt = case["block"]
            assert len(sh["support"]) == 20 and all(lo <= j < lo + cnt for j in sh["support"]) and sh["iter"] >= 6, (name, sh["support"], sh["iter"])
        for oc in others:                                                   # every rank returns the same model
            assert oc[name]["sharded"]["support"] == sh["support"], name
            assert oc[name]["sharded"]["beta"] == sh["beta"], name
            assert oc[name]["sharded"]["logl"] == sh["logl"], name
    tally.finish()
    # the reference's recorded run (docs/src/man/examples.md:230-267) reproduced by the column-SHARDED fit
    g = json.load(open(os.path.join(GOLD, "golden_normal_k7.json")))
    sh = res["cases"]["normal_k7"]["sharded"]
    assert sh["iter"] == g["iterations"] and sh["bt"] == g["backtracks"]
    assert [j + 1 for j in sh["support"]] == g["positions_1based"]
    np.testing.assert_allclose(sh["logl_trace"], g["logl"], rtol=1e-11)
    np.testing.assert_allclose(sh["tol"], g["tol"], rtol=1e-7)
    np.testing.assert_allclose(sh["beta"], g["beta_printed"], rtol=5e-6)
    np.testing.assert_allclose(sh["c"], g["c_printed"], rtol=5e-6)
    assert sh["sigma_g"] == pytest.approx(g["pve"], rel=1e-9)
    assert res["cases"]["ties_choose"]["single"]["choose_fired"]


def _check_growth_and_gather(res, world):
    """a large model, a small one, a larger one, a small one over ONE communicator (its staging buffer grows and is re-used):
    every rank reports the same fit, the local supports add up to k; and the library's gather of the CV losses
    (mih_cv_allgather) equals the torch.distributed one and the single-process matrix exactly"""
    for k in range(world):
        for a, b in zip(res[k]["cases"]["staging_growth"], res[0]["cases"]["staging_growth"]):
            assert (a["k"], a["logl"], a["iter"]) == (b["k"], b["logl"], b["iter"]), k
        cv = res[k]["cases"]["cv_gather"]
        assert cv["native"] == cv["torch"] == res[0]["cases"]["cv_gather"]["single"], k
    for t, kk in enumerate((40, 3, 90, 5)):
        assert sum(res[k]["cases"]["staging_growth"][t]["nnz"] for k in range(world)) == kk


def _same_summary(a, b, what):
    """two fits' summaries, bit for bit -- except the loglikelihood trace's last bit: the device-resident step (native exchange)
    assembles the closed form with the device's `log`, the host-driven step (callbacks) with glibc's (<= 1 ulp apart)"""
    assert set(a) == set(b), what
    for key in a:
        if key in ("logl_trace", "logl"):
            np.testing.assert_allclose(a[key], b[key], rtol=4e-16, atol=0, err_msg=str(what))
        else:
            assert a[key] == b[key], (what, key)


def _build_fake_rccl():
    """tests/libfake_rccl.so from tests/fake_rccl.c (gcc against the real <rccl/rccl.h>: the stand-in's definitions must match
    the real prototypes to compile) and, beside it, the code object of its one kernel (the device-side all-reduce of round 5)."""
    src, lib = os.path.join(ROOT, "tests", "fake_rccl.c"), os.path.join(ROOT, "tests", "libfake_rccl.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src, "-o", lib,
                               "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread", "-ldl"])
    ksrc, kobj = os.path.join(ROOT, "tests", "fake_rccl_kernels.hip"), os.path.join(ROOT, "tests", "fake_rccl_kernels.hsaco")
    if not os.path.exists(kobj) or os.path.getmtime(kobj) < os.path.getmtime(ksrc):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O2", ksrc, "-o", kobj])
    return lib


@pytest.mark.parametrize("world", [2, 3])
def test_native_exchange_with_more_than_one_rank_on_one_gpu(tmp_path, world):
    """csrc/comm.hip with world > 1 on the one-GPU box: the ranks share device 0 and the library loads the
    test-only stand-in librccl (tests/fake_rccl.c: shared memory + hipMemcpy, the real header's prototypes and enum names)
    through MENDELIHT_RCCL_LIB.  The native exchange -- hand-declared data type / reduction codes, the all-gather layout, the
    growth and re-use of the staging buffer, the private stream against the fit's stream, collective teardown -- must give
    the callbacks' results bit for bit on every rank, the single-process fit to rounding, and mih_cv_allgather the torch
    all-gather's losses exactly."""
    lib = _build_fake_rccl()
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "sharded_worker.py"), str(out)]
    env = dict(os.environ, OMP_NUM_THREADS="4", MIH_NATIVE="1", MIH_NATIVE_ONE_DEVICE="1", MENDELIHT_RCCL_LIB=lib)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [json.load(open(str(out) + f".native.r{k}")) for k in range(world)]
    for name in ("normal_k7", "logistic", "init_beta", "poisson_outlier"):
        for k in range(world):
            a, b = res[k]["cases"][name]["native"], res[k]["cases"][name]["callbacks"]
            _same_summary(a, b, (name, k))                               # every field, bit for bit (json round-trips doubles)
            assert a == res[0]["cases"][name]["native"], (name, k)       # ... and the same on every rank
            # the native fit's steps ran resident on the device (round 5), the callbacks' were host-driven
            assert res[k]["cases"][name]["resident_steps_native"] >= a["iter"] - 1 > 0, (name, k)
            assert res[k]["cases"][name]["resident_steps_callbacks"] == 0, (name, k)
        one, sh = res[0]["cases"][name]["single"], res[0]["cases"][name]["native"]
        assert sh["support"] == one["support"] and sh["iter"] == one["iter"] and sh["bt"] == one["bt"], name
        np.testing.assert_allclose(sh["beta"], one["beta"], rtol=0, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(sh["logl_trace"], one["logl_trace"], rtol=1e-11, err_msg=name)
    # (round 6) debias over the shards: host-driven steps either way, the panel's sum on the library's communicator or through the callbacks
    for k in range(world):
        a, b = res[k]["cases"]["debias"]["native"], res[k]["cases"]["debias"]["callbacks"]
        _same_summary(a, b, ("debias", k))
        assert a == res[0]["cases"]["debias"]["native"], ("debias", k)
    one, sh = res[0]["cases"]["debias"]["single"], res[0]["cases"]["debias"]["native"]
    assert sh["support"] == one["support"] and sh["iter"] == one["iter"] >= 6 and sh["bt"] == one["bt"], "debias"
    np.testing.assert_allclose(sh["beta"], one["beta"], rtol=0, atol=1e-9, err_msg="debias")
    plain = res[0]["cases"]["debias"]["single_plain"]               # the refit ran and moved the estimates (or the trajectory)
    assert plain["support"] != one["support"] or plain["iter"] != one["iter"] or np.max(np.abs(np.asarray(plain["beta"]) - np.asarray(one["beta"]))) > 1e-6
    # the multivariate fit through the native exchange: the callbacks' result on every rank, the single-process fit to rounding
    for k in range(world):
        a, b = res[k]["cases"]["mv_r3"]["native"], res[k]["cases"]["mv_r3"]["callbacks"]
        _same_summary(a, b, ("mv_r3", k))
        assert a == res[0]["cases"]["mv_r3"]["native"], k
    one, sh = res[0]["cases"]["mv_r3"]["single"], res[0]["cases"]["mv_r3"]["native"]
    assert sh["support"] == one["support"] and sh["iter"] == one["iter"] and sh["bt"] == one["bt"] and sh["iter"] >= 5
    np.testing.assert_allclose(sh["beta"], one["beta"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(sh["Sigma"], one["Sigma"], rtol=1e-9)
    g = json.load(open(os.path.join(GOLD, "golden_normal_k7.json")))     # the reference's recorded run through the native exchange
    sh = res[0]["cases"]["normal_k7"]["native"]
    assert sh["iter"] == g["iterations"] and [j + 1 for j in sh["support"]] == g["positions_1based"]
    np.testing.assert_allclose(sh["logl_trace"], g["logl"], rtol=1e-11)
    _check_growth_and_gather(res, world)


def test_native_rccl_exchange_matches_the_callbacks_on_two_gpus(tmp_path):
    """The library's own RCCL communicator (mih_comm_create_rccl) with MORE than one rank -- ncclAllReduce / ncclAllGather over
    xGMI, the hand-declared enum values, the all-gather layout, the ordering against the fit's stream -- against the
    torch.distributed callbacks: identical results on every rank.  Needs two GPUs (one per rank): skipped on the one-GPU test
    box, where the native path is covered with a one-rank communicator (test_native_rccl_communicator_world1)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs one GPU per rank (two GPUs)")
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "sharded_worker.py"), str(out)]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="4", MIH_NATIVE="1", HSA_ENABLE_IPC_MODE_LEGACY="0"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [json.load(open(str(out) + f".native.r{k}")) for k in range(2)]
    for name in ("normal_k7", "logistic"):
        for k in range(2):
            a, b = res[k]["cases"][name]["native"], res[k]["cases"][name]["callbacks"]
            _same_summary(a, b, (name, k))                               # every field, bit for bit (json round-trips doubles)
            assert res[k]["cases"][name]["resident_steps_native"] >= a["iter"] - 1 > 0, (name, k)
        assert res[0]["cases"][name]["native"] == res[1]["cases"][name]["native"], name
    _check_growth_and_gather(res, 2)
