"""tests/sets_spec.py, the numpy statement of the set-based tests, held to independent references on the CPU: its saddlepoint value
against the same formula in 50-digit mpmath (eigenvalues from mpmath.eigsy of the spec's M), the approximation itself against the
exact tail of the mixture (spectra of equal pairs in closed form, generic ones by Imhof's integral), the identities of one-member
and duplicated-column sets, the margins of the edge inputs, and csrc/mixture_tail.h -- the host's finish -- compiled into
tests/mixture_tail_harness.cpp with g++ (plainly and under -fsanitize=address,undefined as a stand-alone program) against the spec."""
import math
import os
import subprocess

import numpy as np
import pytest

import assoc_spec as S
import sets_spec as T
from conftest import ROOT

LN10 = math.log(10.0)
CPU_CASES = (T.EDGE_CASES[0], T.EDGE_CASES[3], T.EDGE_CASES[8])       # a share of the GPU test's inputs, the one with the spec's largest error among them


# ---- the references -----------------------------------------------------------------------------------------------------------------
def mp_saddle(lam, Q, dps=50):
    """-log10 of the saddlepoint tail in mpmath from eigenvalues lam (mpf, any order, <= 0 dropped) and Q."""
    import mpmath as mp
    mp.mp.dps = dps
    lam = sorted((v for v in lam if v > 0), reverse=True)
    Q = mp.mpf(Q)
    k1 = lambda t: sum(v / (1 - 2 * v * t) for v in lam)
    hi = 1 / (2 * lam[0])
    lo = -mp.mpf(1)
    while k1(lo) > Q:
        lo *= 2
    a, b = lo, hi
    for _ in range(400):                       # bisection: K' is increasing on t < 1 / (2 lambda_1)
        mid = (a + b) / 2
        if k1(mid) > Q:
            b = mid
        else:
            a = mid
    t = (a + b) / 2
    K = -sum(mp.log1p(-2 * v * t) for v in lam) / 2
    K2 = 2 * sum((v / (1 - 2 * v * t)) ** 2 for v in lam)
    w = mp.sign(t) * mp.sqrt(2 * (t * Q - K))
    v = t * mp.sqrt(K2)
    r = w + mp.log(v / w) / w
    return -mp.log(mp.erfc(r / mp.sqrt(2)) / 2) / mp.log(10)


def exact_pairs(lam, Q, dps=80):
    """-log10 P(sum_i lambda_i (chi2_1 + chi2_1') > Q) for distinct lambda_i, each counted twice: a sum of exponentials,
    sum_i exp(-Q / (2 lambda_i)) prod_{k != i} lambda_i / (lambda_i - lambda_k)."""
    import mpmath as mp
    mp.mp.dps = dps
    lam = [mp.mpf(float(v)) for v in lam]
    tot = mp.mpf(0)
    for i, a in enumerate(lam):
        term = mp.exp(-mp.mpf(Q) / (2 * a))
        for k, b in enumerate(lam):
            if k != i:
                term *= a / (a - b)
        tot += term
    return -mp.log10(tot)


def exact_imhof(lam, Q):
    """-log10 of the tail by Imhof's integral, P(X > x) = 1/2 + 1/pi int_0^inf sin(theta(u)) / (u rho(u)) du with
    theta(u) = 1/2 sum atan(lambda_i u) - x u / 2 and rho(u) = prod (1 + lambda_i^2 u^2)^(1/4), integrated between the zeros of the
    asymptotic oscillation."""
    import mpmath as mp
    mp.mp.dps = 30
    lam = [mp.mpf(float(v)) for v in lam]
    x = mp.mpf(Q)

    def f(u):
        if u == 0:
            return (sum(lam) - x) / 2
        th = sum(mp.atan(v * u) for v in lam) / 2 - x * u / 2
        rho = mp.mpf(1)
        for v in lam:
            rho *= (1 + v * v * u * u) ** mp.mpf("0.25")
        return mp.sin(th) / (u * rho)
    val = mp.quadosc(f, [0, mp.inf], omega=x / 2)
    return -mp.log10(mp.mpf(1) / 2 + val / mp.pi)


# ---- 1. the spec against mpmath ----------------------------------------------------------------------------------------------------------
def test_the_saddlepoint_value_against_mpmath_on_the_edge_inputs():
    import mpmath as mp
    worst, checked = 0.0, 0
    for case in CPU_CASES:
        res = T.edge_inputs(case)[7]
        for d in res["detail"]:
            if d["tail"]["state"] != 1 or len(d["cols"]) > 40:
                continue
            mp.mp.dps = 50
            ev = mp.eigsy(mp.matrix(d["M"].tolist()), eigvals_only=True)
            ref = mp_saddle(list(ev), d["Q"])
            worst = max(worst, float(abs(mp.mpf(d["tail"]["neglog10p"]) - ref) / ref))
            checked += 1
    print(f"spec against mpmath: {checked} sets, worst relative error in log p {worst:.3g} (SPEC_ERR {T.SPEC_ERR:.3g})")
    assert checked >= 12 and worst <= T.SPEC_ERR


# ---- 2. the approximation against the exact tail ------------------------------------------------------------------------------------------
def test_the_approximation_against_the_exact_mixture_tail():
    rng = np.random.default_rng(11)
    worst, n = 0.0, 0
    for m in (1, 2, 3, 5, 10, 30):                            # m pairs: spectra of 2 .. 60 eigenvalues
        lam = np.sort(rng.uniform(0.05, 1.0, m) * np.exp(rng.uniform(-1, 1)))[::-1]
        full = np.sort(np.repeat(lam, 2))[::-1]
        mean, sd = full.sum(), math.sqrt(2 * (full ** 2).sum())
        for zq in (-1.0, 0.0, 1.0, 3.0, 6.0, 12.0, 20.0):
            Q = mean + zq * sd
            if Q <= 0.05 * mean:
                continue
            tl = T.skat_tail(full, Q)
            assert tl["state"] in (1, 3), (m, zq, tl)
            err = abs(tl["neglog10p"] - float(exact_pairs(lam, Q)))
            worst, n = max(worst, err), n + 1
    for lam in ([1.0, 0.6, 0.3], [1.0, 0.9, 0.5, 0.2, 0.1], [2.0, 0.1, 0.1, 0.05]):
        lam = np.array(lam)
        mean, sd = lam.sum(), math.sqrt(2 * (lam ** 2).sum())
        for zq in (0.5, 2.0, 4.0):
            Q = mean + zq * sd
            tl = T.skat_tail(lam, Q)
            err = abs(tl["neglog10p"] - float(exact_imhof(lam, Q)))
            worst, n = max(worst, err), n + 1
    print(f"saddlepoint against the exact tail: {n} points, worst |delta neglog10p| = {worst:.4g} (APPROX_ERR {T.APPROX_ERR:.4g})")
    assert n >= 40 and worst <= 2 * T.APPROX_ERR


# ---- 3. identities ------------------------------------------------------------------------------------------------------------------------
def test_one_member_sets_duplicated_columns_and_the_order_of_sets():
    case = CPU_CASES[2]
    codes, A, w, Z, sets, omega, sp, res, _ = T.edge_inputs(case)
    nlp = S.neglog10p(sp["z"][:, 0])
    ok = np.flatnonzero(~np.isnan(sp["V"]))[:40]
    one = T.set_test(sp, w, [np.array([j]) for j in ok])
    assert np.array_equal(one["neglog10p_burden"], nlp[ok]) and np.array_equal(one["neglog10p_skat"], nlp[ok]) and (one["skat_state"] == 2).all()
    k = len(sets) - 2                                          # the duplicated-column set
    assert sets[k].tolist() == list(T.DUP) and res["skat_state"][k] == 2
    assert abs(res["neglog10p_skat"][k] - nlp[T.DUP[0]]) <= 1e-12 * nlp[T.DUP[0]]
    dead = T.set_test(sp, w, [np.array([3, 17, T.EDGE_P - 2])])
    assert dead["m_used"][0] == 0 and dead["skat_state"][0] == 0 and np.isnan(dead["neglog10p_skat"][0]) and np.isnan(dead["burden_z"][0])
    rev = T.set_test(sp, w, sets[::-1], omega[::-1])
    for name in ("burden_z", "neglog10p_burden", "skat_q", "neglog10p_skat", "skat_state", "m_used"):
        assert np.array_equal(rev[name][::-1], res[name], equal_nan=True), name
    # the limit at the mean continues the saddlepoint value: the tail falls as Q rises, so the value at the mean lies between
    # those at Q one part in 1000 below and above it (the sign of the limit, r = +kappa_3 / 6, decides this)
    lam = np.array([1.0, 0.7, 0.2])
    below, at, above = (T.skat_tail(lam, lam.sum() * f) for f in (1 - 1e-3, 1.0, 1 + 1e-3))
    assert at["state"] == 3 and below["state"] == above["state"] == 1 and below["neglog10p"] < at["neglog10p"] < above["neglog10p"]
    assert above["neglog10p"] - below["neglog10p"] < 5e-3
    assert T.skat_tail(lam, 0.0)["state"] == 4 and T.skat_tail(lam, 0.0)["neglog10p"] == 0.0
    assert T.skat_tail(lam, 1e-300)["state"] == 5 and T.skat_tail(np.array([0.0, 0.0]), 1.0)["state"] == 0


# ---- 4. the edge inputs keep every decision clear --------------------------------------------------------------------------------------------
def test_the_edge_inputs_have_clear_decisions_and_few_redrawn_sets():
    states = set()
    for case in CPU_CASES:
        res, share = T.edge_inputs(case)[7:9]
        assert share <= T.MAX_REDRAWN, (case, share)
        for d in res["detail"]:
            assert T.clear(d), case
            lam, tl = d["lam"], d["tail"]
            if lam.size > 1 and lam[0] > 0:
                assert not (2.0 ** -50 <= lam[1] / lam[0] <= 2.0 ** -30) and tl["evals"] <= 96
                assert d["S"] / np.abs(d["M"]).sum() >= 1e-3
            if tl["state"] == 1:
                assert not (2.0 ** -30 <= math.sqrt(tl["w2"]) <= 2.0 ** -10)
        states |= set(res["skat_state"].tolist())
        assert sorted(len(s) for s in T.edge_inputs(case)[4][:10]) == sorted(T.EDGE_SIZES)
    assert states == {0, 1, 2}
    ns = [c[1] for c in T.EDGE_CASES]
    assert min(ns) < 4 * 4 and min(ns) % 4 and T.CHUNK in ns and T.CHUNK + 1 in ns and any(n > 3 * T.CHUNK and n % T.CHUNK for n in ns)
    assert {c[4] for c in T.EDGE_CASES} == set(S.EDGE_FLAGS) and {c[3] for c in T.EDGE_CASES} == {0.0, 0.03}
    assert {c[5] for c in T.EDGE_CASES if c[0] == "assoc"} == set(S.EDGE_WEIGHTS) and any(c[0] == "spa" for c in T.EDGE_CASES)


# ---- 5. csrc/mixture_tail.h -------------------------------------------------------------------------------------------------------------------
def build(tmp_path, sanitize):
    exe = tmp_path / ("mix_san" if sanitize else "mix")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mendeliht.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "mixture_tail_harness.cpp"), "-o", str(exe)]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_finish_against_the_spec(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    items = []                                                  # (lam, Q, T, S)
    for case in CPU_CASES[:2]:
        res = T.edge_inputs(case)[7]
        items += [(d["lam"], d["Q"], d["T"], d["S"]) for d in res["detail"]]
    rng = np.random.default_rng(5)
    for m in (2, 3, 7, 50, 128):
        lam = np.sort(rng.uniform(0.0, 1.0, m) ** 3)[::-1] * 10.0 ** rng.integers(-6, 6)
        mean, sd = lam.sum(), math.sqrt(2 * (lam ** 2).sum())
        for zq in (-2.0, -0.5, 0.0, 0.5, 3.0, 10.0, 40.0):
            items.append((lam, max(mean + zq * sd, 1e-3 * mean), float(rng.standard_normal()), float(rng.uniform(0.1, 2.0))))
    items += [(np.array([2.0, 1.0, 1.0]), 4.0, 1.0, 0.0), (np.array([2.0, 1.0, 1.0]), 0.0, 1.0, -1.0), (np.array([2.0, 1.0, 1.0]), 1e-300, 0.0, 1.0),
              (np.array([0.0, 0.0]), 1.0, 1.0, 1.0), (np.zeros(0), 0.0, 0.0, 0.0), (np.array([math.nan, math.nan]), 1.0, 1.0, 1.0),
              (np.array([3.0, 1e-14]), 5.0, -2.0, 3.0), (np.array([1.0] * 128), 1000.0, 3.0, 1.0), (np.array([1.0, 0.0, 0.0]), 2.0, 3.0, 1.0)]
    text, want = [], []
    for lam, Q, Tt, Ss in items:
        text.append(f"{len(lam)} {float(Q)!r} {float(Tt)!r} {float(Ss)!r}")
        text += [repr(float(v)) for v in lam]
        tl = T.skat_tail(lam, Q)
        bz = Tt / math.sqrt(Ss) if Ss > 0 else math.nan
        want.append((tl, bz, float(S.neglog10p(np.float64(bz)))))
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(want) and len(want) > 60
    states = set()

    def same(a, b, rel):
        return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rel * abs(b) + 1e-300

    for row, (tl, bz, bn) in zip(rows, want):
        assert int(row[0]) == tl["state"] and int(row[3]) == tl["evals"], (row, tl)
        assert same(float(row[1]), tl["neglog10p"], 1e-12), (row, tl)
        assert same(float(row[2]), tl["t_hat"], 1e-13), (row, tl)
        assert same(float(row[4]), bz, 1e-15) and same(float(row[5]), bn, 1e-13), (row, bz, bn)
        states.add(tl["state"])
    print(f"harness: {len(want)} sets, states {sorted(states)}")
    assert states == {0, 1, 2, 3, 4, 5}


def test_the_entry_point_is_declared_and_exported():
    import re
    from mendeliht_amd import api
    hdr = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"\b(mih_[a-z0-9_]+)\s*\(", hdr))
    assert "mih_assoc_sets" in declared and "mih_assoc_sets" in api.exported_symbols()
    assert "assoc_sets.hip" in open(os.path.join(ROOT, "mendeliht.jl_amd", "csrc", "Makefile")).read()
