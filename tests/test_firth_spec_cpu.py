"""tests/firth_spec.py, the numpy statement of the Firth-penalised test of the association scan, checked on the CPU: against
50-digit mpmath with a bracketed root of the stated equation, against a direct maximisation of the penalised likelihood, on the
boundary columns the saddlepoint refuses, on a common-allele column where it must agree with the score test, on the states and
on a NaN sum; the margins of the GPU test's inputs; csrc/firth_finish.h -- the control of the root iteration the device runs and
the host's finish -- compiled into tests/firth_finish_harness.cpp with g++ (plainly and under -fsanitize=address,undefined as a
stand-alone program) against the spec; and the declaration of the entry point."""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import assoc_spec as S
import firth_spec as F
import spa_spec as P
from conftest import ROOT

LD = np.longdouble


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def mp_firth(c, h, q):
    """(b_hat, se_firth, neglog10p_firth) of a column in 50-digit mpmath from the same float64 c, h, q: the root of
    g(b) = K1 - K3 / (2 K2) = q by a bracketed Newton solve of the stated equation (below), then dev, se and the chi^2_1 tail as
    the module docstring of firth_spec states them."""
    import mpmath as mp
    mp.mp.dps = 50
    c = [mp.mpf(float(v)) for v in c]
    h = [mp.mpf(float(v)) for v in h]
    mu = [1 / (1 + mp.exp(-x)) for x in h]
    sp0 = [mp.log1p(mp.exp(x)) for x in h]
    m1 = mp.fsum(ci * mi for ci, mi in zip(c, mu))
    q = mp.mpf(float(q))

    def sums(b):
        t1, t2, t3, t4 = [], [], [], []
        for ci, hi, mi in zip(c, h, mu):
            sg = 1 / (1 + mp.exp(-(hi + ci * b)))
            s = sg * (1 - sg)
            c2 = ci * ci
            t1.append(ci * (sg - mi)); t2.append(c2 * s); t3.append(c2 * ci * s * (1 - 2 * sg)); t4.append(c2 * c2 * s * (1 - 6 * s))
        return mp.fsum(t1), mp.fsum(t2), mp.fsum(t3), mp.fsum(t4)

    def f_and_slope(b):
        k1, k2, k3, k4 = sums(b)
        return k1 - k3 / (2 * k2) - q, k2 - (k4 * k2 - k3 * k3) / (2 * k2 * k2), k2

    # g - q may change sign more than once (L* has two maxima on some separated columns), so WHICH root is part of the
    # statement: the one the stated iteration reaches.  It is run here in exact arithmetic -- Newton from 0 with slope D inside
    # the bracket of the signs seen, midpoint / doubling where a step leaves it -- until the step is below 1e-42, and the root
    # is then certified by a sign change of g - q across b -+ 1e-38 max(|b|, 1).
    I0 = f_and_slope(mp.mpf(0))[2]
    b, lo, hi = mp.mpf(0), -mp.inf, mp.inf
    for _ in range(300):
        f, d, k2 = f_and_slope(b)
        if f < 0:
            lo = b
        else:
            hi = b
        bn = b - f / (d if d > 0 else k2)
        if abs(bn - b) <= mp.mpf(10) ** -42 * max(abs(b), mp.mpf(10) ** -30):
            b = bn
            break
        if not (lo < bn < hi):
            if f < 0:
                bn = (b + hi) / 2 if hi != mp.inf else (2 * b if b > 0 else mp.mpf(1))
            else:
                bn = (lo + b) / 2 if lo != -mp.inf else (2 * b if b < 0 else mp.mpf(-1))
        b = bn
    else:
        raise AssertionError("no root")
    eps = mp.mpf(10) ** -38 * max(abs(b), 1)
    assert f_and_slope(b - eps)[0] < 0 < f_and_slope(b + eps)[0], "no sign change at the root"
    K = mp.fsum(mp.log1p(mp.exp(hi_ + ci * b)) - s0 for ci, hi_, s0 in zip(c, h, sp0)) - b * m1
    K2 = sums(b)[1]
    dev = max(2 * (b * q - K + mp.log(K2 / I0) / 2), mp.mpf(0))
    nlp = -mp.log10(mp.erfc(mp.sqrt(dev / 2)))
    return b, 1 / mp.sqrt(K2), nlp


def spec_errors(d, c, h, q):
    """The spec's errors on a state-1 column against mpmath: (|b - ref| / se, relative error of se, relative error of neglog10p)."""
    b, se, nlp = mp_firth(c, h, q)
    return (float(abs(d["beta"] - b) / se), float(abs(d["se"] - se) / se), float(abs(d["nlp"] - nlp) / nlp) if nlp > 0 else 0.0)


@functools.lru_cache(maxsize=None)
def prepared(case, cutoff=P.CUTOFF):
    """The inputs of an edge case and the answers of the plain, the saddlepoint and the Firth spec, computed once and shared."""
    codes, y, eta, A, w, Z, _ = P.edge_inputs(case)
    sp = S.score(codes, case[4], A, w, Z)
    dz = S.bound(sp, codes, case[4], A, w, Z)[0]
    return codes, y, eta, A, w, Z, sp, dz, F.firth(sp, eta, Z, cutoff)


ALL_CASES = tuple(P.edge_cases()) + tuple(P.EXTRA_CASES)


# ---- 1. against mpmath ---------------------------------------------------------------------------------------------------------------
def test_spec_against_mpmath_on_a_share_of_the_gpu_inputs():
    """One tried column of every case (the middle one of those in state 1) and the boundary column of every case that has one:
    the errors stay below the figures recorded in firth_spec, which the device tolerance is built on."""
    worst, checked = [0.0, 0.0, 0.0], 0
    for case in ALL_CASES:
        codes, y, eta, A, w, Z, sp, dz, res = prepared(case)
        ones = np.flatnonzero(res["state"] == 1)
        cols = set(ones[len(ones) // 2:][:1].tolist())
        if case[1] >= 31 and case[0] <= 600 and res["state"][7] == 1:
            cols.add(7)
        for j in sorted(cols):
            d = res["detail"][j]
            err = spec_errors(d, d["c"], eta, sp["U"][j, 0])
            worst = [max(a, b) for a, b in zip(worst, err)]
            checked += 1
    print(f"spec against mpmath on the edge inputs: {checked} columns, worst |db| / se {worst[0]:.3g} (SPEC_ERR_BETA {F.SPEC_ERR_BETA:.3g}), "
          f"se {worst[1]:.3g} ({F.SPEC_ERR_SE:.3g}), neglog10p {worst[2]:.3g} ({F.SPEC_ERR_NLP:.3g})")
    assert checked >= 30
    assert worst[0] <= F.SPEC_ERR_BETA and worst[1] <= F.SPEC_ERR_SE and worst[2] <= F.SPEC_ERR_NLP


# ---- 2. properties ----------------------------------------------------------------------------------------------------------------------
def penalised_loglik(col, b):
    """L*(b) in longdouble."""
    x = col.h + col.c * LD(b)
    e, r = P._parts(x)
    x0 = col.h
    e0, r0 = P._parts(x0)
    K = np.sum(P.softplus(x) - P.softplus(x0)) - LD(b) * np.sum(col.c * col.mu)
    k2 = np.sum((col.c * col.c) * ((e * r) * r))
    k20 = np.sum((col.c * col.c) * ((e0 * r0) * r0))
    return LD(b) * LD(col.q) - K + np.log(k2 / k20) / 2


def test_the_root_maximises_the_penalised_likelihood():
    """A direct scalar maximisation of L* in longdouble (Brent, no derivative) against the root of g = q.  L* is formed relative
    to its value at the spec's b_hat before it is rounded to float64; near the maximum L* falls by (db / se)^2 / 2, so a
    maximiser that resolves differences of 1e-19 |L*| (|L*| < 1000 here) finds the maximum to about 1.4e-8 se: 1e-6 se is asked."""
    from scipy.optimize import minimize_scalar
    worst, done = 0.0, 0
    for case in [c for c in P.edge_cases() if c[1] == 33][::2] + [P.EXTRA_CASES[1]]:
        codes, y, eta, A, w, Z, sp, dz, res = prepared(case)
        for j in sorted(res["detail"])[:6] + ([7] if 7 in res["detail"] else []):
            d = res["detail"][j]
            if d["state"] != 1:
                continue
            col = d["col"]
            col.q = float(sp["U"][j, 0])
            top = penalised_loglik(col, d["beta"])
            assert abs(float(top)) < 1000
            with np.errstate(all="ignore"):
                opt = minimize_scalar(lambda b: float(top - penalised_loglik(col, b)), bracket=(d["beta"] - 3 * d["se"], d["beta"], d["beta"] + 2 * d["se"]),
                                      method="brent", options=dict(xtol=1e-13))
            worst = max(worst, abs(opt.x - d["beta"]) / d["se"])
            assert float(opt.fun) <= 0.0 + 1e-15
            done += 1
    print(f"root against a direct maximisation of L*: {done} columns, worst |db| / se {worst:.3g}")
    assert done >= 30 and worst <= 1e-6


def test_every_column_the_saddlepoint_refuses_gets_a_finite_estimate():
    """The boundary columns of spa_spec.edge_inputs (every carrier a case: the saddlepoint's state 2) and every other column the
    saddlepoint refuses: Firth state 1, a finite b_hat of the sign of U, and a finite p-value that is less extreme than the
    normal tail's."""
    seen = 0
    for case in ALL_CASES:
        codes, y, eta, A, w, Z, sp, dz, res = prepared(case)
        spa = P.spa(sp, eta, Z, P.CUTOFF, columns=sorted(res["detail"]))
        for j in np.flatnonzero(spa["state"] == 2):
            d = res["detail"][j]
            assert d["state"] == 1 and math.isfinite(d["beta"]) and d["beta"] * sp["U"][j, 0] > 0, (case, j, d["state"], d["beta"])
            assert math.isfinite(d["nlp"]) and d["nlp"] < res["neglog10p"][j], (case, j)
            assert d["evals"] <= 16, (case, j, d["evals"])
            seen += 1
        if case[1] >= 31 and case[2] == 1:
            assert spa["state"][7] == 2, case
    print(f"columns the saddlepoint refuses: {seen}, all with Firth state 1")
    assert seen >= 10


def test_common_allele_column_agrees_with_the_score_test():
    """n = 1000, half of the rows cases, allele frequency 0.3, no effect, an intercept only.  There mu = 1/2, omega = 0 and K3(0) = 0
    exactly, so the penalty's term vanishes at 0 and the leading difference between the penalised estimate and the one-step U / V
    is the quartic term of K: b_hat / (U / V) - 1 ~ -K4 b^2 / (6 K2) with K4 / K2 ~ -c^2 / 2 ~ -0.3 and b = z / sqrt(V) ~ 0.2 for
    |z| ~ 2, i.e. a few parts in a thousand, and the same order for dev / z^2 (plus the penalty's 1 / n terms).  2 % is asked
    of both; the spec's own figures are printed."""
    n = 1000
    rng = np.random.default_rng(31)
    y = np.zeros(n)
    y[rng.permutation(n)[:n // 2]] = 1.0
    Z = np.ones((n, 1))
    null = P.null_model(y, Z)
    mu = P.sigma(null.eta)
    codes = rng.binomial(2, 0.3, (n, 40)).astype(np.int64)
    sp = S.score(codes, (1, 1, 1), y - mu, mu * (1 - mu), Z)
    res = F.firth(sp, null.eta, Z, 1.0)
    assert len(res["detail"]) >= 5
    wd, wb = 0.0, 0.0
    for j, d in res["detail"].items():
        assert d["state"] == 1
        wd = max(wd, abs(d["dev"] / sp["z"][j, 0] ** 2 - 1))
        wb = max(wb, abs(d["beta"] / sp["beta"][j, 0] - 1))
        assert abs(d["se"] / sp["se"][j] - 1) <= 0.02
    print(f"common allele, n = 1000: {len(res['detail'])} columns, worst |dev / z^2 - 1| {wd:.3g}, |b_hat / (U / V) - 1| {wb:.3g}")
    assert wd <= 0.02 and wb <= 0.02


def test_states_0_and_2_return_the_plain_values_and_a_nan_sum_ends_in_state_2():
    case = (129, 33, 2, 0.03, (1, 1, 1), 4243)
    codes, y, eta, A, w, Z, _ = P.edge_inputs(case)
    sp = S.score(codes, case[4], A, w, Z)
    nlp = S.neglog10p(sp["z"][:, 0])
    none = F.firth(sp, eta, Z, math.inf)
    assert (none["state"] == 0).all() and (none["evals"] == 0).all() and not none["detail"]
    for got, plain in ((none["beta_firth"], sp["beta"][:, 0]), (none["se_firth"], sp["se"]), (none["neglog10p_firth"], nlp)):
        assert got.tobytes() == np.asarray(plain, dtype=np.float64).tobytes()
    two = F.firth(sp, eta, Z, 2.0)
    tried = ~sp["deg"] & (np.abs(sp["z"][:, 0]) >= 2.0)
    assert np.array_equal(two["state"] != 0, tried) and tried.sum() >= 1 and sp["deg"].sum() == 3
    assert two["beta_firth"][~tried].tobytes() == sp["beta"][~tried, 0].tobytes() and two["neglog10p_firth"][~tried].tobytes() == nlp[~tried].tobytes()
    every = F.firth(sp, eta, Z, 0.0)
    assert np.array_equal(every["state"] == 0, sp["deg"])
    assert np.array_equal(two["beta_firth"][tried], every["beta_firth"][tried])
    # a NaN among the sums of an evaluation, the first or a later one: not converged, state 2, the plain values as given
    j = int(np.flatnonzero(tried)[0])
    d = every["detail"][j]
    plain = (float(sp["beta"][j, 0]), float(sp["se"][j]), float(nlp[j]))
    # (K1, K2 or K3: they enter g.  A NaN K4 enters the slope only, which then falls back to K2 by the rule for D.)
    for at, which in ((1, 0), (2, 0), (1, 2), (3, 2), (2, 1)):
        col = F.Column(d["c"], eta)

        def sums(b, col=col, at=at, which=which):
            k = list(col.k1234(b))
            if col.evals == at:
                k[which] = math.nan
            return tuple(k)
        bad = F.column(d["c"], eta, float(sp["U"][j, 0]), float(sp["V"][j]), plain, sums=sums)
        assert bad["state"] == 2 and not bad["converged"] and bad["evals"] == at, (at, which, bad["state"], bad["evals"])
        assert (bad["beta"], bad["se"], bad["nlp"]) == plain
    # K2(b_hat) below the guard: state 2 whatever else holds
    assert F.finish(1.0, True, 0.5, 2.0 ** -41, 1.0, 1.0, 1.0)[0] == 2 and F.finish(1.0, True, 0.5, 2.0 ** -39, 1.0, 1.0, 1.0)[0] == 1
    assert F.finish(1.0, False, 0.5, 1.0, 1.0, 1.0, 1.0)[0] == 2 and F.finish(math.inf, True, 0.5, 1.0, 1.0, 1.0, 1.0)[0] == 2
    assert F.finish(1.0, True, 2.0, 1.0, 1.0, 1.0, 1.0) == (1, 0.0)                      # a negative dev is 0


# ---- 3. clear decisions -----------------------------------------------------------------------------------------------------------------
def test_few_columns_of_the_gpu_inputs_have_an_unclear_decision():
    shares = []
    for case in ALL_CASES:
        codes, y, eta, A, w, Z, sp, dz, res = prepared(case)
        tried = sorted(res["detail"])
        unclear = [j for j in range(case[1]) if not F.clear(sp, res, j, P.CUTOFF, dz)]
        shares.append(len(unclear) / max(len(tried), 1))
        assert len(unclear) <= F.MAX_UNCLEAR * max(len(tried), 1), (case, unclear)
        assert all(d["evals"] <= 16 for d in res["detail"].values()), case
    case = [c for c in P.edge_cases() if c[:2] == (513, 150)][0]
    codes, y, eta, A, w, Z, sp, dz, _ = prepared(case)
    res = F.firth(sp, eta, Z, 0.0)
    unclear = [j for j in range(150) if not F.clear(sp, res, j, 0.0, dz)]
    assert len(res["detail"]) == 147 and len(unclear) <= F.MAX_UNCLEAR * 147, unclear
    k2v = min(d["K2"] / sp["V"][j] for j, d in res["detail"].items())
    ev = [d["evals"] for d in res["detail"].values()]
    print(f"largest share of tried columns with an unclear decision: {max(shares):.3g}; cutoff 0 on (513, 150): {len(unclear)} unclear, "
          f"evaluations mean {np.mean(ev):.2f} max {max(ev)}, smallest K2(b_hat) / V {k2v:.3g}")


# ---- 4. csrc/firth_finish.h ---------------------------------------------------------------------------------------------------------------
def build(tmp_path, sanitize):
    exe = tmp_path / ("firth_san" if sanitize else "firth")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mendeliht.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "firth_finish_harness.cpp"), "-o", str(exe)]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_finish_and_iteration_control_against_the_spec(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    text, want = [], []
    for case in [(64, 33, 1, 0.03, (0, 0, 1), 15004), (257, 33, 1, 0.0, (1, 1, 1), 15016), (256, 33, 2, 0.0, (0, 0, 1), 15013)]:
        codes, y, eta, A, w, Z, _ = P.edge_inputs(case)
        sp = S.score(codes, case[4], A, w, Z)
        res = F.firth(sp, eta, Z, 0.0)
        for k, (j, d) in enumerate(res["detail"].items()):
            plain = (float(sp["beta"][j, 0]), float(sp["se"][j]), float(res["neglog10p"][j]))
            nan_at = (k % 3) + 1 if k % 7 == 3 else 0              # some columns with a NaN sum: state 2
            if nan_at:
                col = F.Column(d["c"], eta)

                def sums(b, col=col, at=nan_at):
                    kk = list(col.k1234(b))
                    if col.evals == at:
                        kk[0] = math.nan
                    return tuple(kk)
                d = F.column(d["c"], eta, float(sp["U"][j, 0]), float(sp["V"][j]), plain, sums=sums)
            text.append(f"{case[0]} {float(sp['U'][j, 0])!r} {float(sp['V'][j])!r} {plain[0]!r} {plain[1]!r} {plain[2]!r} {nan_at}")
            text += [f"{float(ci)!r} {float(hi)!r}" for ci, hi in zip(d["c"], eta)]
            want.append((d["state"], d["beta"], d["se"], d["nlp"], d["evals"], plain))
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    print(f"harness: {len(want)} columns")
    assert len(rows) == len(want) and len(want) > 60
    states = set()
    for row, (st, b, se, nlp, evals, plain) in zip(rows, want):
        assert int(row[0]) == st and int(row[4]) == evals, (row, st, evals)
        got = [float(v) for v in row[1:4]]
        if st == 1:
            assert abs(got[0] - b) <= 1e-13 * abs(b) and abs(got[1] - se) <= 1e-13 * se and abs(got[2] - nlp) <= 1e-12 * nlp + 1e-300, (row, b, se, nlp)
        else:
            assert tuple(got) == plain, (row, plain)
        states.add(st)
    assert states == {1, 2}


# ---- 5. the declaration -----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_listed():
    from mendeliht_amd import api
    text = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(mih_\w+)\s*\(", text))
    assert "mih_assoc_score_firth" in declared and "mih_assoc_score_firth" in api.exported_symbols()
    m = re.search(r"int\s+mih_assoc_score_firth\s*\((.*?)\);", text, flags=re.S)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "A", "w", "Z", "c", "eta", "cutoff", "slice_rows", "z", "beta", "se", "neglog10p", "beta_firth",
                                                       "se_firth", "neglog10p_firth", "firth_state", "firth_evals", "neglog10p_spa", "spa_state", "t_hat"]
