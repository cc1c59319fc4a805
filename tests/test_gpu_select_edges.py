"""project_k! on the device at its buffer edges: the stand-alone select of csrc/topk.hip (the device finish, the host finish, the
radix fallback, the landing buffer's second copy) against the oracle bit for bit, and the resident select of csrc/resident.inc
inside fits whose supports fill or overflow its lists -- step_mode 0 against step_mode 1 bit for bit, both against the oracle,
with the counters saying which way every step ran.  tests/test_select_edges_cpu.py shows without a device that every input has
the property its name promises; DESIGN.md ("The select at its buffer edges") has the table of edges and the counters observed."""
import numpy as np
import pytest

from conftest import hash_folds, seeded_draw, tied_case
from gpu_helpers import (_NUDGES, clear_cut_backtracks, tied_copy_counts, tied_fit_route, SELECT_C_N, SELECT_C_WEIGHT, SELECT_FIT_N, TINY_COMBOS, TINY_DROPPED, TINY_MAX_ITER, TINY_N, _run_probe_snippet, _same_fit,
                         model_size_cases, planted_response, project_cases, select_constants, select_fit_problem, select_layout_c,
                         select_tied_copies, tiny_problem)

pytestmark = pytest.mark.gpu

_CASES = project_cases()


@pytest.fixture(scope="module")
def projected(oracle):
    """oracle.project_k of every case, computed once."""
    return [oracle.project_k(c.v, c.k) for c in _CASES]


@pytest.mark.parametrize("t", range(len(_CASES)), ids=[c.name for c in _CASES])
def test_project_k_at_its_buffer_edges(mih, projected, t):
    """mih.project_k = oracle.project_k, entry for entry, on a vector that sits on one side of kFinishBin, kFinishCap, the landing
    buffer k + 64 or the gather buffer k + 1024 (gpu_helpers.project_cases; the side is proved in the CPU companion), on the
    degenerate inputs and on lengths around the sweeps' grids with the threshold at the ends of the vector and at the hand-over of
    the unrolled loop to its tail."""
    c = _CASES[t]
    got = mih.project_k(c.v, c.k)
    assert np.array_equal(got, projected[t]), (c.name, np.flatnonzero(got != projected[t])[:8], np.count_nonzero(got), np.count_nonzero(projected[t]))


_RADIX_SNIPPET = r"""
import os, sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import mendeliht_amd as m
from gpu_helpers import project_cases
assert os.environ.get("MENDELIHT_HIP_PROBES") == "1" and os.environ.get("MENDELIHT_TOPK_RADIX8") == "1"
np.savez(sys.argv[2], **{f"r{t}": m.project_k(c.v, c.k) for t, c in enumerate(project_cases())})
"""


def test_project_k_radix_select_on_every_case(mih, projected, tmp_path):
    """The 8 x 8-bit radix select + compact_device (the fallback behind the gather buffer) on the WHOLE list: one child process on
    the measurement build with MENDELIHT_TOPK_RADIX8=1; the results come back as arrays and are compared with the oracle here.
    Survivors beyond k + 64 take compact_device's second copy, survivors beyond k + 1024 grow its buffer."""
    got = _run_probe_snippet(_RADIX_SNIPPET, tmp_path / "radix.npz", extra_env={"MENDELIHT_TOPK_RADIX8": "1"}, timeout=300)
    assert len(got.files) == len(_CASES)
    bad = [c.name for t, c in enumerate(_CASES) if not np.array_equal(got[f"r{t}"], projected[t])]
    assert not bad, bad


# ---- the resident select inside fits ------------------------------------------------------------------------------------------
_COUNTS = {}


def _both_modes(mih, what, x, y, z, resident=True, **kw):
    """The fit with its steps resident (step_mode 0) and host-driven (step_mode 1), the profile counters on around each: the same
    fit bit for bit (_same_fit), every step of the first accounted for, none of the second resident."""
    out = []
    for mode in (0, 1):
        mih.profile_enable(x, True)
        mih.profile_counters(x, reset=True)
        try:
            res = mih.fit_iht(y, x, z, verbose=False, step_mode=mode, **kw)
        finally:
            cnt = mih.profile_counters(x, reset=True)
            mih.profile_enable(x, False)
        out.append((res, cnt))
    (a, cnt), (b, host) = out
    _COUNTS[what] = {key: cnt[key] for key in ("resident_steps", "resident_handbacks", "resident_direct", "resident_redos", "resident_attempts")}
    print(what, "steps", len(a.trace["logl"]), _COUNTS[what])
    _same_fit(a, b, what)
    # every fit of this file is Normal: its one scalar logarithm is csrc/scalar_log.h's on the host and on the device, so the
    # loglikelihood traces are equal bit for bit, without the last-bit allowance of _same_fit
    assert np.array_equal(a.trace["logl"].view(np.uint64), b.trace["logl"].view(np.uint64)), what
    assert host["resident_steps"] == 0 and host["resident_handbacks"] == 0, (what, host)
    if resident:
        assert cnt["resident_steps"] + cnt["resident_handbacks"] == len(a.trace["logl"]), (what, cnt, len(a.trace["logl"]))
    return a, cnt


def _against_oracle(what, a, o, backtracks=True):
    """Iteration count, backtrack trace, support, estimates and loglikelihood trace, at the tolerances of
    test_resident_steps_with_five_thousand_effects."""
    assert a.iter == o["iter"], (what, a.iter, o["iter"])
    if backtracks:
        assert list(a.trace["backtracks"]) == list(o["bt_trace"]), (what, list(a.trace["backtracks"]), list(o["bt_trace"]))
    assert np.array_equal(np.flatnonzero(a.beta), np.flatnonzero(o["beta"])), what
    np.testing.assert_allclose(a.beta, o["beta"], rtol=1e-5, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(a.c, o["c"], rtol=1e-5, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(a.trace["logl"], o["logl_trace"], rtol=1e-9, err_msg=what)


@pytest.fixture(scope="module")
def layouts(mih, oracle):
    """Layouts A and B (gpu_helpers.select_fit_problem) on the device and in the oracle, built on first use."""
    made = {}

    def get(layout):
        cols, y, planted, k, max_iter = select_fit_problem(layout)
        if cols.shape[0] not in made:
            made[cols.shape[0]] = (mih.SnpLinAlg(cols, n=SELECT_FIT_N, center=True, scale=True, impute=True), oracle.Mat.from_bed_columns(cols, SELECT_FIT_N))
        return made[cols.shape[0]] + (y, planted, k, max_iter)
    return get


def test_layout_a_a_spread_list_overflows(mih, oracle, layouts):
    """40 effects at 5 + 512 m among 41 x 512 columns: k_res_collect deals the entries out by j mod 512, so list 5 takes 40 > 32 in
    every projection and k_res_select hands the step back (RES_ABORT, the iterate untouched); the host replays it and the next
    step starts resident again.  No step ever stands resident, so no direct gather is ever queued.
    Observed on the device: 7 steps, resident_steps = 0, resident_handbacks = 7, resident_direct = 0, resident_redos = 0."""
    x, ox, y, planted, k, max_iter = layouts("A")
    a, cnt = _both_modes(mih, "layout A", x, y, None, k=k, max_iter=max_iter)
    assert cnt["resident_handbacks"] >= 1 and cnt["resident_direct"] == 0, cnt
    assert np.isin(planted, np.flatnonzero(a.beta)).all()
    _against_oracle("layout A", a, oracle.fit_iht(ox, y, None, k=k, max_iter=max_iter))


def test_layout_a_in_a_session(mih, oracle, layouts):
    """The same problem as an IHTSession: steps, the model read in between (the iterate comes home and goes back), a run of steps --
    every one of them handed back -- equal to the host-driven session step for step, and to the oracle after as many steps.
    Observed: 6 steps, resident_handbacks = 6, resident_steps = 0."""
    x, ox, y, planted, k, _ = layouts("A")
    mih.profile_enable(x, True)
    mih.profile_counters(x, reset=True)
    a = mih.IHTSession(y, x, None, k=k, step_mode=0)
    b = mih.IHTSession(y, x, None, k=k, step_mode=1)
    try:
        for _ in range(3):
            sa, sb = a.step(), b.step()
            assert abs(sa[0] - sb[0]) <= 4e-16 * abs(sb[0]) and sa[1:] == sb[1:]
        (ba, ca), (bb, cb) = a.model(), b.model()
        assert np.array_equal(ba, bb) and np.array_equal(ca, cb)
        ra, rb = a.run(3), b.run(3)
        assert abs(ra[0] - rb[0]) <= 4e-16 * abs(rb[0]) and ra[1:] == rb[1:]
        (ba, ca), (bb, cb) = a.model(), b.model()
        assert np.array_equal(ba, bb) and np.array_equal(ca, cb)
    finally:
        a.close(); b.close()
        cnt = mih.profile_counters(x, reset=True)
        mih.profile_enable(x, False)
    print("layout A session", cnt)
    assert cnt["resident_steps"] + cnt["resident_handbacks"] == 6 and cnt["resident_handbacks"] >= 1, cnt
    o = oracle.fit_iht(ox, y, None, k=k, max_iter=7)               # fit.jl:170: max_iter = 7 performs 6 steps
    assert o["iter"] == 7 and np.array_equal(np.flatnonzero(ba), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(ba, o["beta"], rtol=1e-5, atol=1e-12)
    assert abs(ra[0] - o["logl"]) <= 1e-9 * abs(o["logl"])


def test_layout_a_in_the_lockstep_lanes(mih, oracle, layouts):
    """... and through cv_iht (path [40, 45], three hash folds): a lane's fit whose step the device hands back -- the path of
    lane_collect_step that no other test reaches.  Held-out losses bit-equal between the step modes, the oracle's at 1e-8.
    Observed: 6 fits in one lane, scores = 64, resident_steps = 0, resident_handbacks = 64."""
    x, ox, y, _, _, _ = layouts("A")
    folds = hash_folds(SELECT_FIT_N, 3)
    got = {}
    for mode in (0, 1):
        mih.set_step_mode(mode)
        mih.profile_enable(x, True)
        mih.profile_counters(x, reset=True)
        try:
            raw = mih.cv_iht(y, x, None, path=[40, 45], q=3, folds=folds, verbose=False, return_raw=True)[1]
        finally:
            mih.set_step_mode(0)
            cnt = mih.profile_counters(x, reset=True)
            mih.profile_enable(x, False)
        got[mode] = (np.asarray(raw), cnt)
    (a, ca), (b, cb) = got[0], got[1]
    print("layout A cv_iht", ca)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert ca["scores"] == cb["scores"] and ca["fits"] == cb["fits"]
    assert cb["resident_steps"] == 0 and cb["resident_handbacks"] == 0, cb
    assert ca["resident_steps"] + ca["resident_handbacks"] == ca["scores"] > 0 and ca["resident_handbacks"] >= 1, ca
    _, want = oracle.cv_iht(ox, y, None, path=[40, 45], q=3, folds=folds)
    np.testing.assert_allclose(a.reshape(want.shape), want, rtol=1e-8)


@pytest.mark.parametrize("layout", ["B", "B_exact64", "B_exact65"])
def test_layout_b_the_direct_gather_overflows(mih, oracle, layouts, layout):
    """70 (64, 65) effects in adjacent columns, all inside ONE block's contiguous range of k_res_grad: the lists of the histogram
    sweeps (j mod 512) hold one or two entries each, so every step stands resident; the direct gather puts them all into one list
    of 32, says so (RES_REDO_SLOW) and the attempt is redone with the sweeps -- the host stops forecasting after three failures.
    The support list of 64 per block overflows for 70 and 65 (the binary search in the sorted model) and is exactly full for 64
    (the last linear scan).
    Observed (B, B_exact64, B_exact65 alike): 7 steps, resident_steps = 7, resident_handbacks = 0, resident_direct = 6,
    resident_redos = 3."""
    x, ox, y, planted, k, max_iter = layouts(layout)
    a, cnt = _both_modes(mih, f"layout {layout}", x, y, None, k=k, max_iter=max_iter)
    assert cnt["resident_handbacks"] == 0 and cnt["resident_redos"] >= 1, cnt
    assert np.isin(planted, np.flatnonzero(a.beta)).all()
    _against_oracle(f"layout {layout}", a, oracle.fit_iht(ox, y, None, k=k, max_iter=max_iter))


@pytest.mark.parametrize("at_boundary", [False, True], ids=["len=4x512x256-1", "len=4x512x256"])
def test_layout_c_the_spread_rules_boundary(mih, oracle, at_boundary):
    """40 effects adjacent inside one 256-aligned run of columns, p + 1 = 4 x 512 x 256 - 1 and 4 x 512 x 256.  Below the boundary
    k_res_collect deals the vector out entry by entry (40 lists, one entry each): the steps stay resident.  At the boundary it
    walks runs of 256: ONE list receives all 40 and every step is handed back.
    The rows: 400 with prior weights of 100 on the planted columns, not ~2000 without -- the oracle has to hold the matrix too
    (131 KB of genotypes per row), the weights make the 40 columns outrank every other by two orders of magnitude from the first
    projection on whatever the noise does, and with them the weighted projection (vectorize! / unvectorize!) is on the path.  That the
    oracle recovers all 40 is asserted here, on the device, since no CPU test can generate this matrix.
    Observed: below, 7 steps, resident_steps = 7, resident_handbacks = 0, resident_direct = 6, resident_redos = 3 (the direct
    gather's contiguous range of 1024 holds the whole run); at the boundary, resident_steps = 0, resident_handbacks = 7."""
    n = SELECT_C_N
    x = mih.SnpLinAlg.synthetic(n, select_layout_c(at_boundary)[0], seed=71)
    maf = np.asarray(x.maf())
    p, planted = select_layout_c(at_boundary, polymorphic=np.minimum(maf, 1.0 - maf) * 2 * n >= 8)      # (synthetic allele frequencies are U(0, 0.5): some columns of 400 rows are monomorphic)
    assert p == x.p and planted[0] % 256 == 0
    cols = x.export_bed()
    ox = oracle.Mat.from_bed_columns(cols, n)
    y = planted_response(cols, n, planted, np.random.default_rng([7, 40, n]))
    w = np.ones(p)
    w[planted] = SELECT_C_WEIGHT
    what = f"layout C, p + 1 = {p + 1}"
    a, cnt = _both_modes(mih, what, x, y, None, k=45, max_iter=8, weight=w)
    if at_boundary:
        assert cnt["resident_handbacks"] >= 1 and cnt["resident_steps"] == 0, cnt
    else:
        assert cnt["resident_handbacks"] == 0 and cnt["resident_steps"] == len(a.trace["logl"]), cnt
    o = oracle.fit_iht(ox, y, None, k=45, max_iter=8, weight=w)
    assert np.isin(planted, np.flatnonzero(o["beta"])).all()
    _against_oracle(what, a, o)


@pytest.mark.parametrize("copies", tied_copy_counts())
def test_massive_ties_fill_and_overflow_the_pool(mih, oracle, copies):
    """SNP 300 and 2047 (2100, 2112) copies of it, k = 2: every projection ties 2048 (2101, 2113) entries at the threshold.  2048
    fill k_res_select's pool of prefix-sharers exactly: it ranks them, finds more survivors than the model may hold and hands the
    step back for _choose! (abort 3).  2101 and 2113 overflow the pool: the buffer exit (abort 2).  The host-driven replay (and every
    step of the step_mode = 1 twin) runs the stand-alone select as the FIT sizes it -- kcap = max(k + q, 64) + 1024 = 1088, a landing
    buffer of kcap + 64 = 1152 pairs, a gather buffer of kcap + 1024 = 2112 (gpu_helpers.fit_select_caps, read from iht_var.hip):
    2048 and 2101 tied entries stay within the gather buffer and, more than kFinishBin, take the host finish and its second copy;
    2113 exceed it, so the 8 x 8-bit radix select runs INSIDE a fit and compact_device grows its buffer.  No counter records the
    way taken: it follows from the counts (proved in the CPU companion); on a scratch build whose compact_device refuses to grow,
    the 2112-copy case fails and the other two pass.
    The same draws from the same lists in the same order as the oracle, the same support, estimates and loglikelihoods, and the
    oracle's backtrack trace as far as it is clear-cut.
    Observed (all three alike): 5 steps, resident_handbacks = 1 (the step whose projection draws; the other draw of the log is
    the initialisation's, before the first step), resident_steps = 4, resident_direct = 2."""
    assert tied_fit_route(copies)["route"] == ("radix" if copies == tied_copy_counts()[2] else "host")
    cols, y, tied = tied_case(copies=select_tied_copies(copies))
    x = mih.SnpLinAlg(cols, n=1000, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(cols, 1000)
    logs = {}
    for mode in (0, 1):
        logs[mode] = []
        mih.profile_enable(x, True)
        mih.profile_counters(x, reset=True)
        try:
            res = mih.fit_iht(y, x, None, k=2, max_iter=6, verbose=False, step_mode=mode, choose=seeded_draw(11, logs[mode]))
        finally:
            cnt = mih.profile_counters(x, reset=True)
            mih.profile_enable(x, False)
        logs[mode] = (logs[mode], res, cnt)
    (la, a, ca), (lb, b, cb) = logs[0], logs[1]
    print(f"ties, {copies} copies: steps", len(a.trace["logl"]), ca, list(a.trace["backtracks"]))
    _same_fit(a, b, f"{copies} copies")
    assert np.array_equal(a.trace["logl"].view(np.uint64), b.trace["logl"].view(np.uint64))
    assert ca["resident_steps"] + ca["resident_handbacks"] == len(a.trace["logl"]) and ca["resident_handbacks"] >= 1, ca
    assert cb["resident_steps"] == 0 and cb["resident_handbacks"] == 0
    lo = []
    o = oracle.fit_iht(ox, y, None, k=2, max_iter=6, choose=seeded_draw(11, lo))
    assert a.choose_fired and b.choose_fired and o["choose_fired"]
    assert la == lb == lo and [(kind, len(lst), excess) for kind, lst, excess in lo] == [(0, copies + 1, copies - 2)] * 2 and lo[0][1] == tied
    # the backtrack trace as far as the oracle's own is clear-cut: after the draw the model is three copies of one column, solved by
    # the next line search, and from then on the oracle's trace moves under ulp-sized nudges -- [0, 3, 0, 0, 0], [0, 1, 3, 3, 0],
    # [0, 0, 0, 0, 0], ... (tests/test_select_edges_cpu.py; test_choose_callback_makes_the_references_random_draw leaves the whole
    # trace out for the same reason).  The entries all those runs share are compared.
    nudged = [oracle.fit_iht(ox, y, np.ones((1000, 1)) * g, k=2, max_iter=6, choose=seeded_draw(11, []))["bt_trace"] for g in _NUDGES]
    clear = clear_cut_backtracks([o["bt_trace"]] + nudged)
    assert clear >= 1 and list(a.trace["backtracks"][:clear]) == list(o["bt_trace"][:clear]), (clear, list(a.trace["backtracks"]), list(o["bt_trace"]))
    _against_oracle(f"{copies} copies", a, o, backtracks=False)


@pytest.fixture(scope="module")
def five_thousand(mih, oracle):
    """The matrix and phenotype of test_resident_steps_with_five_thousand_effects."""
    n, p = 8000, 30_000
    x = mih.SnpLinAlg.synthetic(n, p, seed=61)
    ox = oracle.Mat.from_bed_columns(x.export_bed(), n)
    rng = np.random.default_rng(62)
    supp = np.sort(rng.choice(p, 3000, replace=False))
    z = np.column_stack([np.ones(n), rng.standard_normal(n), rng.standard_normal(n)])
    y = x.xv_sparse(supp, rng.standard_normal(3000) * 0.3) + z @ np.array([0.5, 0.3, 0.0]) + rng.standard_normal(n)
    return x, ox, y, z


@pytest.mark.parametrize("t", range(6), ids=[c[0] for c in model_size_cases()])
def test_model_size_edges(mih, oracle, five_thousand, t):
    """K = k + zkeepn survivors and the 64 the select allows for ties: K + 64 = kResMaxList is the last model k_res_select ranks in
    LDS, one more the first in the scratch block (each once with zkeep = [1, 0, 1], so that zkeepn enters the sum); K + 64 =
    kResBigList is the last resident model, one more steps host-driven from the start (no resident step, none handed back: the
    one case where resident_steps + resident_handbacks is 0, not the number of steps).
    Observed: 5 steps each; resident_steps = 5 and resident_handbacks = 0 up to kResBigList (the LDS select: resident_direct = 10,
    resident_redos = 3; the scratch select takes no direct gather: 0 and 0), resident_steps = 0 and resident_handbacks = 0 beyond."""
    name, k, zkeep, where = model_size_cases()[t]
    x, ox, y, z = five_thousand
    kw = {} if zkeep is None else dict(zkeep=zkeep)
    a, cnt = _both_modes(mih, name, x, y, z, resident=where != "host", k=k, max_iter=6, **kw)
    if where == "host":
        assert cnt["resident_steps"] == 0 and cnt["resident_handbacks"] == 0, cnt
    else:
        assert cnt["resident_handbacks"] == 0 and cnt["resident_steps"] == len(a.trace["logl"]), cnt
    _against_oracle(name, a, oracle.fit_iht(ox, y, z, k=k, max_iter=6, **kw))


_TINY = [c for c in TINY_COMBOS if c not in TINY_DROPPED]


@pytest.mark.parametrize("p,q,k", _TINY, ids=[f"p={p} q={q} k={k}" for p, q, k in _TINY])
def test_tiny_problems(mih, oracle, p, q, k):
    """64 rows, p = 1, 5, 511, 512, 513 columns, one or two covariates, k = 1, p // 2 and p: most of the 512 blocks of every sweep
    own an empty range, k = p keeps everything.  Dropped, because the oracle's own trajectory moves under the ulp-sized nudges of
    gpu_helpers._unstable (a one-SNP model beside the intercept is solved by the first exact line search; every backtracking
    decision after that compares loglikelihoods equal to rounding): (p, q, k) = (1, 1, 1), (5, 1, 1), (511, 1, 1), (512, 1, 1) --
    4 of 26, asserted in the CPU companion.  Observed: every step of the other 22 resident, none handed back.

    p=512 q=2 k=256 found the one defect of this file, outside the select: with k = 256 > n = 64 the fit interpolates, sigma shrinks
    from step to step and the Normal loglikelihood -n/2 (1 + log 2 pi) - n log(sigma) rises through zero (-53.9, -36.9, 11.5,
    58.8 ...).  log(sigma) was taken by the device's libm in b_res_decide and by the host's in IhtVar::mu_loglik; one ulp of it,
    times n, was 1.42e-14 on 11.50356 -- 1.24e-15 of the value against the 4e-16 of _same_fit, and a bit that a backtracking
    decision (logl_cur > logl) could see.  Both sides now take csrc/scalar_log.h's logarithm (the same IEEE operations in the
    same order wherever it runs; tests/test_scalar_log_cpu.py holds it to 1 ulp), and the two traces are equal."""
    assert len(TINY_DROPPED) * 5 <= len(TINY_COMBOS)
    cols, y, z = tiny_problem(p, q)
    x = mih.SnpLinAlg(cols, n=TINY_N, center=True, scale=True, impute=True)
    what = f"tiny p={p} q={q} k={k}"
    a, cnt = _both_modes(mih, what, x, y, z, k=k, max_iter=TINY_MAX_ITER)
    assert cnt["resident_handbacks"] == 0, (what, cnt)
    _against_oracle(what, a, oracle.fit_iht(oracle.Mat.from_bed_columns(cols, TINY_N), y, z, k=k, max_iter=TINY_MAX_ITER))
