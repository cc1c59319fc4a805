"""The inputs of tests/test_gpu_group_edges.py, checked without a GPU: the radix sort's constants are read from csrc/group.hip and the
lengths follow them; on every case of gpu_helpers.group_edge_cases() the oracle (two walks over a sort permutation, as the
reference) agrees with tests/group_spec.py (the projection stated as sets, with a sequential float64 sum) entry for entry, signs of
zeros included; every case has the property its name promises; and the oracle reproduces the fit of group_fit_problem() under
ulp-sized nudges, so the GPU can be held to it."""
import numpy as np
import pytest

import gpu_helpers as H
import group_spec as S
from gpu_helpers import (GROUP_FIT_CAUSAL, GROUP_FIT_G, GROUP_FIT_N, GROUP_FIT_P, GROUP_G_BYTE2, GROUP_G_BYTE3, _NUDGES, _unstable, group_constants,
                         group_edge_cases, group_fit_problem, group_known_answers, group_lengths)

_CASES = group_edge_cases()
_BY = {c[0]: c for c in _CASES}


def _blocks(n):
    return -(-n // group_constants()["tile"])


def test_constants_come_from_the_sources(monkeypatch):
    C = group_constants()
    assert set(C) == {name for pats in H._GROUP_PATTERNS.values() for name in pats} | {"tile"}
    assert C["tile"] == C["round"] * C["items"] and C["round"] % 64 == 0
    assert C["digits"] == 256 and C["scan_chunk"] == C["scan_threads"]          # 8 bits a pass; a thread per entry of a chunk
    assert (C["key_bits"], C["label_bits"], C["norm_bits"]) == (64, 32, 64)
    T = C["tile"]
    assert group_lengths() == (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T, 2 * T + 1, 4 * T, 4 * T + 1, 5 * T + 1)
    # a pattern that no longer matches is an error that names it, not a silently stale constant
    monkeypatch.setattr(H, "_GROUP_CONSTANTS", {})
    monkeypatch.setitem(H._GROUP_PATTERNS["group.hip"], "items", r"constexpr int kRadixItems = (\d+), kRsTile = \d+ \* kRsItems;")
    with pytest.raises(AssertionError, match="items"):
        group_constants()


def test_lengths_sit_on_their_side_of_the_tile_and_of_the_scan_chunk():
    C = group_constants()
    T, R, L = C["tile"], C["round"], group_lengths()
    assert max(L) == 5 * T + 1 and max(c[1].size for c in _CASES) == 5 * T + 1
    assert [_blocks(n) for n in (T - 1, T, T + 1, 2 * T, 2 * T + 1, 4 * T, 4 * T + 1, 5 * T + 1)] == [1, 1, 2, 2, 3, 4, 5, 6]
    assert all(n % T == 1 for n in (T + 1, 2 * T + 1, 4 * T + 1, 5 * T + 1))                 # a last tile of one key
    assert (T - 1) % R == R - 1 and (T - 1) // R == C["items"] - 1                           # a partial LAST round, one lane short
    assert [n % 64 for n in (63, 64, 65)] == [63, 0, 1] and [n - R for n in (255, 256, 257)] == [-1, 0, 1]
    # the histogram k_rs_scan walks holds `digits` entries a block: one chunk exactly at 4 T, a second chunk (the carry) at 4 T + 1
    assert C["digits"] * _blocks(4 * T) == C["scan_chunk"] and C["digits"] * _blocks(4 * T + 1) == C["scan_chunk"] + C["digits"]
    # every value kind stands on both sides of a tile edge, the stability kind at every length
    for kind in H.GROUP_VALUE_KINDS:
        lens = {c[1].size for c in _CASES if c[0].startswith(kind + " len=")}
        assert any(n <= T for n in lens) and any(_blocks(n) >= 2 for n in lens) and any(n % T == 1 and n > T for n in lens), kind
        assert any(C["digits"] * _blocks(n) > C["scan_chunk"] for n in lens), kind
        if kind in ("equal", "normal"):
            assert lens == set(L)


@pytest.mark.parametrize("t", range(len(_CASES)), ids=[c[0] for c in _CASES])
def test_the_oracle_is_the_set_based_statement(oracle, t):
    name, y, group, J, k = _CASES[t]
    want = S.project_group_sparse(y, group, J, k)
    got = oracle.project_group_sparse(y, group, J, k)
    assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8], np.count_nonzero(got), np.count_nonzero(want))
    assert np.array_equal(np.signbit(got), np.signbit(want)), (name, np.flatnonzero(np.signbit(got) != np.signbit(want))[:8])
    assert np.array_equal(got[got != 0], y[got != 0]) and not np.signbit(got[(got == 0) & (y != 0)]).any()
    known = group_known_answers().get(name)
    if known is not None:
        assert np.array_equal(want, known) and np.array_equal(np.signbit(want), np.signbit(known)), name


def test_the_specs_sum_is_sequential():
    """One float64 add at a time, the largest square first -- not numpy's pairwise sum (blocks from 8 terms on), not a fused
    multiply-add: against a plain Python loop on random groups, and on the tie case whose answer depends on it."""
    rng = np.random.default_rng(626)
    differs = 0
    for trial in range(50):
        n = int(rng.integers(8, 400))
        y = rng.standard_normal(n) * np.exp(rng.normal(0, 2, n))
        group = rng.integers(1, 4, n)
        norms = S.group_norms(y, group, n)
        for g, got in norms.items():
            v = y[group == g]
            v = v[np.argsort(-np.abs(v), kind="stable")]
            acc = 0.0
            for s in (v * v).tolist():
                acc = acc + s
            assert got == acc, (trial, g)
            differs += int(float(np.sum(v * v)) != acc)
    assert differs > 20                                     # the distinction is not vacuous
    name = "tie across the cut by the sequential sum, the lone entry is group 1"
    _, y, group, J, k = _BY[name]
    norms = S.group_norms(y, group, k)
    v = y[group == 2]
    v = v[np.argsort(-np.abs(v), kind="stable")]
    assert norms[1] == norms[2] == 2.0 ** 54 and float(np.sum(v * v)) > 2.0 ** 54       # pairwise: the nine ones meet first and count


def test_every_case_has_the_property_its_name_promises():
    C = group_constants()
    T = C["tile"]
    names = [c[0] for c in _CASES]
    assert len(set(names)) == len(names)
    for name, y, group, J, k in _CASES:
        assert not np.isnan(y).any() and group.min() >= 1 and J >= 0 and np.min(k) >= 0, name
        assert np.ndim(k) == 0 or k.size >= group.max(), name
    kinds = {kind: [c for c in _CASES if c[0].startswith(kind + " len=")] for kind in H.GROUP_VALUE_KINDS}
    # stability: a single |y|, so index order alone decides; scalar k in {1, 3} and vector k, G in {1, 3, 300}, at every length >= T - 1
    for name, y, group, J, k in kinds["equal"]:
        assert np.unique(np.abs(y)).size == 1 and (y.size < 64 or {-1.5, 1.5} == set(y)), name
    for n in (x for x in group_lengths() if x >= T - 1):
        here = [c for c in kinds["equal"] if c[1].size == n]
        assert {c[4] for c in here if np.ndim(c[4]) == 0} == {1, 3} and sum(np.ndim(c[4]) > 0 for c in here) == 2, n
        assert {int(c[0].split("G=")[1].split()[0]) for c in here} == {1, 3, 300}
    for name, y, group, J, k in kinds["zeros"]:
        assert set(np.abs(y)) <= {0.0, 1.0} and (y.size < 65 or (np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all())), name
    for name, y, group, J, k in kinds["extremes"]:
        a = np.abs(y)
        assert y.size < 64 or (np.isinf(a).any() and (a == 5e-324).any() and (a == 1e-323).any() and (a == 1e308).any() and (a == 2.2250738585072014e-308).any()), name
    # one byte: for each of the eight key bytes, two keys that are neighbours in the sorted order and differ in that byte alone
    for name, y, group, J, k in kinds["onebyte"]:
        keys = np.unique(S.abs_bits(y))
        assert all(bin(int(v)).count("1") == 1 for v in keys), name
        x = keys[1:] ^ keys[:-1]
        only = {b for b in range(8) for v in x if int(v) & ~(0xFF << (8 * b)) == 0}
        assert only == set(range(8)), (name, only)
    # label bytes 2 and 3, and G far beyond len: the norm sort has more blocks than the member sort
    b2 = [c for c in _CASES if c[0].startswith("label byte 2")]
    b3 = [c for c in _CASES if c[0].startswith("label byte 3")]
    assert len(b2) == 5 and len(b3) == 1
    for name, y, group, J, k in b2 + b3:
        G = GROUP_G_BYTE3 if "byte 3" in name else GROUP_G_BYTE2
        assert group.max() == G and y.size == 300 and _blocks(G) > _blocks(y.size) and {G - 1, G, 1, 65535, 65536, 65537} <= set(group)
        assert ((group - 1) >> 16 & 0xFF).max() > 0 and len(set((group - 1) >> 16 & 0xFF)) >= 2
        if "byte 3" in name:
            assert {2 ** 24, 2 ** 24 + 1} <= set(group) and len(set((group - 1) >> 24)) == 2 and np.ndim(k) == 0
        else:
            assert ((group - 1) >> 24).max() == 0
    # label layouts
    assert all((c[2] == 300).all() for c in _CASES if c[0].startswith("every entry labelled 300"))
    assert all(set(c[2]) == {1, 300} for c in _CASES if c[0].startswith("labels 1 and 300 only"))
    for c in (c for c in _CASES if c[0].startswith("labels 101..200 empty")):
        assert not ((c[2] > 100) & (c[2] <= 200)).any() and (c[2] <= 100).any() and (c[2] > 200).any() and c[3] > 100
    assert all((c[2] == 1).all() for c in _CASES if c[0].startswith("one group"))
    # degenerate J and k
    for n, G in ((257, 3), (T + 1, 300)):
        tail = f"len={n} G={G}"
        assert {c[3] for c in _CASES if tail in c[0] and c[0].startswith("J=")} == {0, 1, G, G + 3, 2 ** 40}
        assert {c[4] for c in _CASES if tail in c[0] and c[0].startswith("k=")} == {0, 1, 3, 2 ** 62}
        _, y, group, J, k = _BY[f"vector k with a 0 at a populated label {tail}"]
        assert group.max() == G and k.size == G and (k[np.unique(group) - 1] == 0).any() and set(k) <= {0, 1, 2, 3}
        assert (_BY[f"vector k with 2^62 inside {tail}"][4] == 2 ** 62).sum() == 1
        assert _BY[f"vector k longer than G {tail}"][4].size == G + 7
    # ties: bit-equal norms by the spec's sequential sum, on either side of the cut
    for lone in (1, 2):
        _, y, group, J, k = _BY[f"tie across the cut by the sequential sum, the lone entry is group {lone}"]
        norms = S.group_norms(y, group, k)
        assert np.float64(norms[1]).view(np.uint64) == np.float64(norms[2]).view(np.uint64) and norms[1] > norms[3] and J == 1
    for J in (2, 3):
        _, y, group, _, k = _BY[f"3^2 + 4^2 against 5^2 across the cut J={J}"]
        norms = S.group_norms(y, group, k)
        assert np.float64(norms[2]).view(np.uint64) == np.float64(norms[5]).view(np.uint64) and norms[1] > norms[2] > norms[3] and 4 not in norms
    for J in (4, 5, 8, 10):
        _, y, group, _, k = _BY[f"J beyond the non-empty groups: zero norms rank by label J={J}"]
        norms = S.group_norms(y, group, k)
        assert sorted(norms) == [2, 5, 9, 10] and [norms[g] for g in (5, 9, 10)] == [0.0, 0.0, 0.0] and norms[2] > 0 and J > 1
    assert set(group_known_answers()) <= set(names) and len(group_known_answers()) == 8


@pytest.mark.parametrize("family", ["normal", "bernoulli"])
@pytest.mark.parametrize("setting", [0, 1])
def test_the_oracle_reproduces_the_group_fit(oracle, family, setting):
    """The fit the GPU file compares: interleaved labels, one absent, a projection of three radix tiles.  The oracle recovers the
    six causal SNPs and reproduces its own trajectory -- iterations, support, beta to 1e-9 -- under the nudges of
    gpu_helpers._NUDGES, so no implementation is excused from it."""
    P = group_fit_problem()
    T = group_constants()["tile"]
    assert P["cols"].shape[0] == GROUP_FIT_P and 2 * T < GROUP_FIT_P <= 3 * T
    group = P["group"]
    assert group.size == GROUP_FIT_P and group.max() == GROUP_FIT_G and 13 not in group and (np.diff(group) != 0).all()
    assert sorted(set(group)) == [g for g in range(1, GROUP_FIT_G + 1) if g != 13]
    assert [int(np.sum(group[P["causal"]] == g)) for g in GROUP_FIT_CAUSAL] == [2, 2, 2]
    k, J = P["settings"][setting]
    if setting == 1:
        assert k.size == GROUP_FIT_G and k[12] == 0 and list(k[np.array(GROUP_FIT_CAUSAL) - 1]) == [2, 2, 2] and k.sum() == GROUP_FIT_G + 2
    y, z = P["y"][family], P["z"]
    kw = dict(k=k, J=J, group=group, **({"dist": "bernoulli", "link": "logit"} if family == "bernoulli" else {}))
    ox = oracle.Mat.from_bed_columns(P["cols"], GROUP_FIT_N)
    o = oracle.fit_iht(ox, y, z, **kw)
    supp = np.flatnonzero(o["beta"])
    print(family, setting, "iter", o["iter"], "support", supp, "groups", group[supp])
    assert np.isin(P["causal"], supp).all() and o["iter"] < 100
    assert len(set(group[supp])) <= J and all(np.sum(group[supp] == g) <= (k[g - 1] if setting else k) for g in set(group[supp]))
    pick = lambda d, g=1.0: dict(iter=d["iter"], beta=d["beta"], nz=(d["beta"] != 0).astype(float), c=d["c"] * g, logl=d["logl"])
    assert np.abs(o["c"]).min() > 0.05
    for g in _NUDGES:
        v = oracle.fit_iht(ox, y, z * g, **kw)
        assert not _unstable(pick(o), pick(v, g), 1e-9, atol=1e-12), (family, setting, g)
