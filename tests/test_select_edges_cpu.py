"""The inputs of tests/test_gpu_select_edges.py, checked without a GPU: the constants are read from the sources, the list rules and
the unrolled loop's hand-over are the kernels' own loops, every vector of the stand-alone select sits on the side of its constant
that its name promises (and the oracle keeps exactly the predicted number of entries), and the fits of layouts A and B and of the
massive ties fill the lists they are meant to fill on a trajectory the oracle reproduces under ulp-sized nudges."""
import numpy as np
import pytest

import gpu_helpers as H
from conftest import seeded_draw, tied_case
from gpu_helpers import (clear_cut_backtracks, fit_select_caps, tied_copy_counts, tied_fit_route, PROJECT_LENGTHS, SELECT_FIT_N, SELECT_LAYOUTS, TINY_COMBOS, TINY_DROPPED, TINY_MAX_ITER, TINY_N, model_size_cases,
                         oracle_wavers, prefix22, project_cases, res_list_of, select_constants, select_counts, select_fit_problem,
                         select_layout_c, select_tied_copies, sweep_handover, tiny_problem)


def test_constants_come_from_the_sources(monkeypatch):
    C = select_constants()
    assert set(C) == {name for pats in H._SELECT_PATTERNS.values() for name in pats}
    assert C["collect_blocks"] == C["grad_blocks"] == C["res_hist_blocks"] == C["hist_blocks"]
    assert C["support_list"] == C["support_scan"]
    assert C["finish_bin"] < C["finish_cap"] and C["expect_pad"] < C["cap_pad"] and C["collect_slots"] < C["support_list"]
    assert C["max_in_bin"] <= C["max_list"] < C["big_list"]
    assert PROJECT_LENGTHS[3:] == tuple(m * C["hist_blocks"] * 256 + d for m in (1, 4) for d in (-1, 0, 1))
    # a pattern that no longer matches is an error that names it, not a silently stale constant
    monkeypatch.setattr(H, "_SELECT_CONSTANTS", {})
    monkeypatch.setitem(H._SELECT_PATTERNS["topk.hip"], "finish_cap", r"constexpr int kFinishCapacity = (\d+);")
    with pytest.raises(AssertionError, match="finish_cap"):
        select_constants()


@pytest.mark.parametrize("length", [1, 300, 512 * 256 + 7, 4 * 512 * 256 - 1, 4 * 512 * 256, 4 * 512 * 256 + 300])
def test_list_rules_are_the_kernels_loops(length):
    """res_list_of against the loops of k_res_collect and k_res_grad<true> walked block by block."""
    B = select_constants()["collect_blocks"]
    stride = B * 256
    b, t = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    owner = np.full(length, -1, dtype=np.int64)
    first = t * B + b if length < 4 * stride else b * 256 + t
    for m in range(-(-length // stride)):
        i = first + m * stride
        ok = i < length
        assert np.all(owner[i[ok]] == -1)
        owner[i[ok]] = b[ok]
    assert np.array_equal(owner, res_list_of(np.arange(length), length, "collect"))
    chunk = -(-length // B)
    direct = np.full(length, -1, dtype=np.int64)
    for blk in range(B):
        direct[blk * chunk:min((blk + 1) * chunk, length)] = blk
    assert np.array_equal(direct, res_list_of(np.arange(length), length, "direct"))


@pytest.mark.parametrize("length", PROJECT_LENGTHS)
def test_handover_is_the_unrolled_loops(length):
    blocks = min(-(-length // 256), select_constants()["hist_blocks"])
    stride = 256 * blocks
    unrolled, tail = [], []
    for g in {0, 1, stride // 2, stride - 2, stride - 1}:
        i = g
        while i + 3 * stride < length:
            unrolled += [i + u * stride for u in range(4)]
            i += 4 * stride
        while i < length:
            tail.append(i)
            i += stride
    lu, ft = sweep_handover(length)
    # the sampled threads include the one that owns either index
    assert (lu is None and not unrolled) or (lu is not None and lu % stride in {0, 1, stride // 2, stride - 2, stride - 1} and max(unrolled) == lu)
    assert (ft is None and not tail) or (ft is not None and ft % stride in {0, 1, stride // 2, stride - 2, stride - 1} and min(tail) == ft)
    if length == 4 * stride:
        assert ft is None
    if length in (4 * stride - 1, 4 * stride + 1):
        assert lu is not None and ft is not None


def test_project_cases_sit_where_their_names_say(oracle):
    C = select_constants()
    cases = project_cases()
    assert len({c.name for c in cases}) == len(cases)
    seen, seen_radix = set(), set()
    for c in cases:
        assert not np.isnan(c.v).any() and 1 <= c.k <= c.v.size, c.name
        got = select_counts(c.v, c.k)
        for key, val in c.want.items():
            assert got[key] == val, (c.name, key, val, got)
        assert got["gathered"] == got["A"] + got["S"] and (got["survivors"] <= got["gathered"]), (c.name, got)
        kept = oracle.project_k(c.v, c.k)
        assert np.count_nonzero(kept) == got["survivors"], (c.name, got)
        assert np.array_equal(kept[kept != 0], c.v[kept != 0])
        seen.add((got["route"], got["fetch"], got["grow"]))
        r8 = select_counts(c.v, c.k, radix8=True)
        assert r8["route"] == "radix" and r8["survivors"] == got["survivors"]
        seen_radix.add((r8["fetch"], r8["grow"]))
    # both finishes with and without the second copy, the radix fallback with a buffer that grows -- and all of it under the switch
    assert seen >= {("device", False, False), ("device", True, False), ("host", False, False), ("host", True, False), ("radix", True, True)}, seen
    assert seen_radix == {(False, False), (True, False), (True, True)}
    by = {c.name: select_counts(c.v, c.k) for c in cases}
    FB, FC, EXP, CAP = C["finish_bin"], C["finish_cap"], C["expect_pad"], C["cap_pad"]
    # the constants are crossed one entry at a time
    for where in ("largest", "middle", "smallest"):
        assert [by[f"sharers S={S} k at the {where}"]["route"] for S in (FB - 1, FB, FB + 1)] == ["device", "device", "host"]
        assert all(by[f"sharers S={S} k at the {where}"]["gathered"] <= by[f"sharers S={S} k at the {where}"]["cap"] for S in (FB - 1, FB, FB + 1))
    assert [by[f"candidates A+S={G}"]["route"] for G in (FC - 1, FC, FC + 1)] == ["device", "device", "host"]
    assert all(by[f"candidates A+S={G}"]["S"] < 64 and by[f"candidates A+S={G}"]["gathered"] + 900 < by[f"candidates A+S={G}"]["cap"] for G in (FC - 1, FC, FC + 1))
    for fin in ("device", "host"):
        g = [by[f"threshold ties t={t}, {fin} finish"] for t in (EXP, EXP + 1, EXP + 2)]
        assert [v["route"] for v in g] == [fin] * 3 and [v["fetch"] for v in g] == [False, False, True]
        assert [v["survivors"] - v["expect"] for v in g] == [-1, 0, 1]
    g = [by[f"gather ties t={t}"] for t in (CAP, CAP + 1, CAP + 2)]
    assert [v["gathered"] - v["cap"] for v in g] == [-1, 0, 1] and [v["route"] for v in g] == ["device", "host", "radix"]
    assert [v["grow"] for v in g] == [False, False, True]
    # the geometry cases: both entries share one prefix, one survives
    for c in cases:
        if c.name.startswith("len="):
            a, b = np.flatnonzero(prefix22(c.v) == prefix22(np.array([3.0]))[0])
            kept = oracle.project_k(c.v, c.k)
            assert np.count_nonzero(kept[[a, b]]) == 1 and abs(c.v[[a, b]]).min() == 3.0


@pytest.mark.parametrize("layout", list(SELECT_LAYOUTS))
def test_fit_layouts_fill_the_lists_they_name(oracle, layout):
    """Every iterate of the oracle's own trajectory (max_iter = 2 .. the test's) holds the planted columns where the layout wants
    them, and that trajectory does not move under the nudges: no case needs to be set aside."""
    C = select_constants()
    cols, y, planted, k, max_iter = select_fit_problem(layout)
    p = cols.shape[0]
    ox = oracle.Mat.from_bed_columns(cols, SELECT_FIT_N)
    collect, direct = [], []
    for m in range(2, max_iter + 1):
        o = oracle.fit_iht(ox, y, None, k=k, max_iter=m)
        s = np.flatnonzero(o["beta"])
        assert o["iter"] == m and s.size == k and not o["choose_fired"]
        if m > 2 or layout == "A":
            assert np.isin(planted, s).all(), (layout, m)
        collect.append(int(np.bincount(res_list_of(s, p + 1, "collect")).max()))
        direct.append(int(np.bincount(res_list_of(s, p + 1, "direct")).max()))
    if layout == "A":
        assert min(collect) == 40 > C["collect_slots"] and max(direct) <= 2
        assert set(res_list_of(planted, p + 1, "collect")) == {5}
    else:
        assert max(collect) <= 3 and min(direct) > C["collect_slots"]
        assert len(set(res_list_of(planted, p + 1, "direct"))) == 1
        want = {"B": 70, "B_exact64": C["support_list"], "B_exact65": C["support_list"] + 1}[layout]
        assert max(direct) == want == len(planted) and direct[1:] == [want] * (len(direct) - 1), (layout, direct)
    assert not oracle_wavers(oracle, ox, y, None, k=k, max_iter=max_iter)


def test_layout_c_crosses_the_spread_rule():
    C = select_constants()
    p0, planted = select_layout_c(False)
    p1, same = select_layout_c(True)
    assert p1 == p0 + 1 == C["spread_strides"] * C["collect_blocks"] * 256 - 1 and np.array_equal(planted, same)
    assert planted[0] % 256 == 0 and planted[-1] // 256 == planted[0] // 256
    assert len(set(res_list_of(planted, p0 + 1, "collect"))) == 40
    assert len(set(res_list_of(planted, p1 + 1, "collect"))) == 1 and 40 > C["collect_slots"]
    # ... wherever the run starts: the first run whose 40 columns are all flagged
    ok = np.ones(p1, dtype=bool)
    ok[planted[7]] = ok[planted[0] + 256 + 39] = ok[planted[0] + 512 + 40] = False
    for at in (False, True):
        p, moved = select_layout_c(at, polymorphic=ok)
        assert moved[0] == planted[0] + 512 and len(set(res_list_of(moved, p + 1, "collect"))) == (1 if at else 40)


@pytest.mark.parametrize("copies", tied_copy_counts())
def test_massive_ties_fill_or_overflow_the_pool(oracle, copies):
    C = select_constants()
    cols, y, tied = tied_case(copies=select_tied_copies(copies))
    assert tied_copy_counts()[:2] == (2047, 2100) and len(tied) == copies + 1
    assert len(tied) == C["max_in_bin"] if copies == 2047 else len(tied) > C["max_in_bin"]          # the resident pool: filled / overflowed
    # the stand-alone select of the host-driven replay is sized by the FIT (kcap = max(k + q, 64) + 1024 -> cap = kcap + 1024 = 2112,
    # landing buffer kcap + 64 = 1152), not by k: 2048 and 2101 tied entries stay within its gather buffer and, being more than
    # kFinishBin, take the host finish with the second copy; only the third count exceeds the buffer by the tied entries alone
    route = tied_fit_route(copies)
    assert (route["expect"], route["cap"]) == fit_select_caps(2, 1) == (max(2 + 1, C["fit_kcap_floor"]) + C["fit_kcap_pad"] + C["expect_pad"],
                                                                      max(2 + 1, C["fit_kcap_floor"]) + C["fit_kcap_pad"] + C["cap_pad"])
    if copies in (2047, 2100):
        assert route == dict(route, route="host", fetch=True, grow=False) and len(tied) + 1 <= route["cap"]
    else:
        assert route == dict(route, route="radix", fetch=True, grow=True) and len(tied) > route["cap"]
    ox = oracle.Mat.from_bed_columns(cols, 1000)
    logs, bts = [], []
    for g in [1.0] + H._NUDGES:
        log = []
        o = oracle.fit_iht(ox, y, np.ones((1000, 1)) * g, k=2, max_iter=6, choose=seeded_draw(11, log))
        assert o["choose_fired"]
        logs.append(([(kind, len(lst), excess) for kind, lst, excess in log], [lst for _, lst, _ in log], o["iter"], np.flatnonzero(o["beta"]).tolist()))
        bts.append((list(o["bt_trace"]), o["bt_cond"], o["beta"], o["logl"]))
    assert logs[0][0] == [(0, copies + 1, copies - 2)] * 2 and logs[0][1][0] == tied
    # clear-cut: the same draws from the same lists, the same number of steps, the same support, the same estimates under the nudges
    assert all(entry == logs[0] for entry in logs[1:])
    for bt, cond, beta, logl in bts[1:]:
        np.testing.assert_allclose(beta, bts[0][2], rtol=1e-5, atol=1e-12)
        assert abs(logl - bts[0][3]) <= 1e-9 * abs(bts[0][3])
    # NOT clear-cut, and reported by the oracle itself (bt_cond): once the draw has removed the excess the three survivors are
    # identical columns, the next exact line search solves the model, and every later backtracking decision compares two
    # loglikelihoods that are equal to rounding -- the backtrack trace is [0, 3, 0, 0, 0] on the input as given and [0, 1, 3, 3, 0],
    # [0, 0, 1, 0, 0], [0, 0, 0, 0, 0] ... under the nudges (the other entries of the trajectory do not move)
    assert min(cond for _, cond, _, _ in bts) < H._BT_TIE and len({tuple(bt) for bt, _, _, _ in bts}) > 1
    # ... from its second entry on: the first step's decision is the same everywhere, and that much the GPU file compares
    assert clear_cut_backtracks([bt for bt, _, _, _ in bts]) == 1 and bts[0][0][0] == 0


def test_tiny_problems_and_what_is_dropped(oracle):
    assert len(TINY_COMBOS) == 26 and len(TINY_DROPPED) * 5 <= len(TINY_COMBOS)
    dropped = []
    for p, q, k in TINY_COMBOS:
        cols, y, z = tiny_problem(p, q)
        ox = oracle.Mat.from_bed_columns(cols, TINY_N)
        if oracle_wavers(oracle, ox, y, z, k=k, max_iter=TINY_MAX_ITER):
            dropped.append((p, q, k))
    assert tuple(dropped) == TINY_DROPPED


def test_model_size_cases_straddle_the_lists():
    C = select_constants()
    cases = model_size_cases(q=3)
    K64 = [(k + (3 if zk is None else sum(zk)) + 64, where) for _, k, zk, where in cases]
    assert K64 == [(C["max_list"], "lds"), (C["max_list"] + 1, "scratch")] * 2 + [(C["big_list"], "scratch"), (C["big_list"] + 1, "host")]
