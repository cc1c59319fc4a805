"""tests/spa_spec.py, the numpy statement of the saddlepoint p-value of the association scan, checked on the CPU: against 40-digit
mpmath with a bracketed root, against the exact distribution of the score statistic at n = 16, on the boundary column, on the
opposite tail outside the range and on the cutoff; the margins of the GPU test's inputs; and csrc/spa_finish.h -- the control of
the root iteration the device runs and the host's finish -- compiled into tests/spa_finish_harness.cpp with g++ (plainly and under
-fsanitize=address,undefined as a stand-alone program) against the spec."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import assoc_spec as S
import spa_spec as P
from conftest import ROOT

LN10 = math.log(10.0)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def mp_neglog10p(c, h, q, V=None):
    """-log10 of the two-sided saddlepoint p-value of a column in 40-digit mpmath, from the same float64 c, h, q: each computed
    tail's root by bisection of a sign-changing bracket to 1e-35, out-of-range rule as the spec's.  None where a tail has no root
    mpmath can bracket, or r has the wrong sign."""
    import mpmath as mp
    mp.mp.dps = 40
    c = [mp.mpf(float(v)) for v in c]
    h = [mp.mpf(float(v)) for v in h]
    sig = [1 / (1 + mp.e ** (-x)) for x in h]
    sp0 = [mp.log1p(mp.e ** x) for x in h]
    m1 = mp.fsum(ci * mi for ci, mi in zip(c, sig))
    smin = mp.fsum(min(ci, 0) for ci in c) - m1
    smax = mp.fsum(max(ci, 0) for ci in c) - m1

    def k1(t):
        return mp.fsum(ci * (1 / (1 + mp.e ** (-(hi + ci * t))) - mi) for ci, hi, mi in zip(c, h, sig))

    def k2(t):
        out = []
        for ci, hi in zip(c, h):
            s = 1 / (1 + mp.e ** (-(hi + ci * t)))
            out.append(ci * ci * s * (1 - s))
        return mp.fsum(out)

    def k0(t):
        return mp.fsum(mp.log1p(mp.e ** (hi + ci * t)) - s0 for ci, hi, s0 in zip(c, h, sp0)) - t * m1
    q = mp.mpf(float(q))
    aq = abs(q)
    tails = []
    for k, s in ((0, aq), (1, -aq)):
        obs = (k == 0) == (q >= 0)
        if not obs and (s >= smax if k == 0 else s <= smin):
            continue
        if not (smin < s < smax):
            return None
        sgn = 1 if s > 0 else -1
        lo, hi = mp.mpf(0), mp.mpf(sgn)
        for _ in range(60):                         # the outer end: doubling until the sign changes
            if (k1(hi) - s) * sgn > 0:
                break
            lo, hi = hi, 2 * hi
        else:
            return None
        # Newton inside the bracket, bisection where it leaves: both keep the sign change
        t = (lo + hi) / 2
        for _ in range(200):
            f = k1(t) - s
            if f * sgn > 0:
                hi = t
            else:
                lo = t
            if abs(hi - lo) <= mp.mpf(10) ** -35 * abs(hi):
                break
            tn = t - f / k2(t)
            t = tn if min(lo, hi) < tn < max(lo, hi) else (lo + hi) / 2
        t = (lo + hi) / 2
        w = mp.sign(t) * mp.sqrt(2 * (t * s - k0(t)))
        v = t * mp.sqrt(k2(t))
        r = w + mp.log(v / w) / w
        if not (r * t > 0):
            return None
        tails.append(mp.ncdf(-abs(r)))
    return float(-mp.log10(mp.fsum(tails)))


def rel_err_in_logp(got, ref):
    return abs(got - ref) / abs(ref)


def small_problem(seed, n, effect, c=2):
    """A seeded column with an intercept and one covariate, 3 % .. 10 % cases, allele frequency 0.01 .. 0.1 and a planted effect on
    the logit scale; redrawn until the null model exists and the column is not degenerate."""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        Z = np.stack([np.ones(n), rng.standard_normal(n)], axis=1)[:, :c]
        g = rng.binomial(2, rng.uniform(0.01, 0.1), n).astype(np.int64)
        share = rng.uniform(0.03, 0.10)
        lin = math.log(share / (1 - share)) + (0.3 * Z[:, 1] if c > 1 else 0.0) + effect * g
        y = (rng.random(n) < 1 / (1 + np.exp(-lin))).astype(np.float64)
        if y.sum() < 2 or S.degenerate(g[:, None])[0]:
            continue
        null = P.null_model(y, Z)
        if null is None:
            continue
        mu = P.sigma(null.eta)
        A, w = y - mu, mu * (1 - mu)
        sp = S.score(g[:, None], (0, 0, 1), A, w, Z)
        if np.isnan(sp["z"][0, 0]):
            continue
        return g[:, None], y, null.eta, A, w, Z, sp
    raise AssertionError(seed)


# ---- 1. against mpmath ---------------------------------------------------------------------------------------------------------------
def test_spec_against_mpmath():
    worst, done, moved = 0.0, 0, 0
    for k in range(42):
        n = (128, 257, 385)[k % 3]
        codes, y, eta, A, w, Z, sp = small_problem(7000 + k, n, (0.0, 1.5, 3.0)[(k // 3) % 3])
        res = P.spa(sp, eta, Z, 0.0)
        if res["state"][0] != 1:
            continue
        ref = mp_neglog10p(res["detail"][0]["c"], eta, sp["U"][0, 0])
        assert ref is not None, k
        err = rel_err_in_logp(res["neglog10p_spa"][0], ref)
        worst = max(worst, err)
        done += 1
        moved += abs(res["neglog10p_spa"][0] - res["neglog10p"][0]) > 0.05 * res["neglog10p"][0]
    print(f"spec against mpmath: {done} columns, worst relative error in log p {worst:.3g}; SPA moved {moved} of them by more than 5 %")
    assert done >= 30 and moved >= 5
    assert worst < 2.0 ** -40


def test_the_size_of_the_correction():
    """The issue's example: few cases among 128 samples, a column with z near 7 -- the normal value overstates by orders of magnitude."""
    best = None
    for k in range(40):
        codes, y, eta, A, w, Z, sp = small_problem(7100 + k, 128, 3.0)
        if abs(sp["z"][0, 0]) > 5:
            res = P.spa(sp, eta, Z, 2.0)
            if res["state"][0] == 1:
                best = (sp["z"][0, 0], res["neglog10p"][0], res["neglog10p_spa"][0])
                break
    assert best is not None
    print("z = %.3g: normal -log10 p = %.3g, saddlepoint %.3g" % best)
    assert best[1] - best[2] > 1.0


# ---- 2. the boundary column ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ncase", [(128, 3), (385, 8), (1000, 5)])
def test_boundary_column_falls_back_to_the_normal_value(n, ncase):
    y = np.zeros(n)
    y[np.random.default_rng(n).choice(n, ncase, replace=False)] = 1.0
    Z = np.ones((n, 1))
    null = P.null_model(y, Z)
    mu = P.sigma(null.eta)
    codes = y.astype(np.int64)[:, None]              # the carriers are exactly the cases
    for flags in S.EDGE_FLAGS:
        sp = S.score(codes, flags, y - mu, mu * (1 - mu), Z)
        res = P.spa(sp, null.eta, Z, 2.0)
        d = res["detail"][0]
        obs = d["tails"][0 if sp["U"][0, 0] >= 0 else 1]
        assert abs(sp["U"][0, 0] - d["col"].smax) <= 1e-12 * d["col"].smax        # the statistic is at the end of its range
        assert res["state"][0] == 2 and res["neglog10p_spa"][0] == res["neglog10p"][0]
        assert not obs["converged"] or obs["K2"] < P.MIN_K2 * sp["V"][0], obs     # the guard (or the limit) is what refuses it
        print(f"boundary n={n}: evals {obs['evals']}, t_hat {obs['t']:.4g}, K''/V {obs['K2'] / sp['V'][0]:.3g}")


# ---- 3. the opposite tail outside the range -----------------------------------------------------------------------------------------------
def opposite_tail_problem():
    """The carriers are the three cases the null model finds least likely, and one such control (so that it is no boundary column):
    their weights mu (1 - mu) are small, the projection hardly moves the other rows, so S_min -- the sum of the negative c_i less M1
    -- is small while q is near S_max: the target -|q| lies below S_min, the lower tail is impossible."""
    n = 300
    for seed in range(9000, 9050):
        rng = np.random.default_rng(seed)
        Z = np.stack([np.ones(n), rng.standard_normal(n)], axis=1)
        y = (rng.random(n) < P.sigma(-2.5 + 1.5 * Z[:, 1])).astype(np.float64)
        null = P.null_model(y, Z)
        if null is None:
            continue
        mu = P.sigma(null.eta)
        g = np.zeros(n, dtype=np.int64)
        cases, controls = np.flatnonzero(y == 1.0), np.flatnonzero(y == 0.0)
        g[cases[np.argsort(mu[cases])[:3]]] = 1
        g[controls[np.argmin(mu[controls])]] = 1
        sp = S.score(g[:, None], (0, 0, 1), y - mu, mu * (1 - mu), Z)
        res = P.spa(sp, null.eta, Z, 2.0)
        if 0 in res["detail"] and sp["U"][0, 0] > 0 and -sp["U"][0, 0] <= res["detail"][0]["col"].smin and res["state"][0] == 1:
            return sp, res, null.eta
    raise AssertionError("no such column")


def test_opposite_tail_outside_the_range_contributes_exactly_zero():
    sp, res, eta = opposite_tail_problem()
    d = res["detail"][0]
    q = sp["U"][0, 0]
    assert q > 0 and -q <= d["col"].smin and q < d["col"].smax
    assert d["tails"][1] is None and np.isnan(res["t_hat"][0, 1]) and res["state"][0] == 1
    assert res["neglog10p_spa"][0] == -d["tails"][0]["logp"] / LN10          # exactly the one tail: the other adds 0
    ref = mp_neglog10p(d["c"], eta, q)
    assert rel_err_in_logp(res["neglog10p_spa"][0], ref) < 2.0 ** -40
    print(f"opposite tail: q {q:.4g} in [{d['col'].smin:.4g}, {d['col'].smax:.4g}], -log10 p {res['neglog10p_spa'][0]:.4g} (normal {res['neglog10p'][0]:.4g})")


# ---- 4. the cutoff ---------------------------------------------------------------------------------------------------------------------
def test_cutoff_semantics():
    case = (129, 33, 2, 0.03, (1, 1, 1), 4243)
    codes, y, eta, A, w, Z, _ = P.edge_inputs(case)
    sp = S.score(codes, case[4], A, w, Z)
    none = P.spa(sp, eta, Z, math.inf)
    assert (none["state"] == 0).all() and np.array_equal(none["neglog10p_spa"], none["neglog10p"], equal_nan=True)
    every = P.spa(sp, eta, Z, 0.0)
    assert np.array_equal(every["state"] == 0, sp["deg"]) and sp["deg"].sum() == 3
    two = P.spa(sp, eta, Z, 2.0)
    tried = ~sp["deg"] & (np.abs(sp["z"][:, 0]) >= 2.0)
    assert np.array_equal(two["state"] != 0, tried)
    assert np.array_equal(two["neglog10p_spa"][tried], every["neglog10p_spa"][tried])
    assert np.array_equal(two["neglog10p_spa"][~tried], two["neglog10p"][~tried], equal_nan=True)


# ---- 5. K''(0) is V ---------------------------------------------------------------------------------------------------------------------
def test_second_derivative_at_zero_is_the_variance():
    for case in [c for c in P.edge_cases() if c[1] == 33][::2]:
        codes, y, eta, A, w, Z, _ = P.edge_inputs(case)
        sp = S.score(codes, case[4], A, w, Z)
        al = P.alpha_of(sp["b"], sp["Linv"])
        dV = None
        for j in np.flatnonzero(~sp["deg"]):
            col = P.Column(P.adjusted(sp["X"][:, j], Z, al[j]), eta)
            k1, k2 = col.k12(0.0)
            assert k1 == 0.0                                  # term by term
            if dV is None:                                    # the plain bound on V: dse / se = dV / V (assoc_spec.bound)
                dV = S.bound(sp, codes, case[4], A, w, Z)[2] / sp["se"] * sp["V"]
            assert abs(k2 - sp["V"][j]) <= dV[j] + 1e-12 * sp["V"][j], (case, j, k2, sp["V"][j])


# ---- 6. against the exact distribution ----------------------------------------------------------------------------------------------------
def test_closer_to_the_exact_distribution_than_the_normal_tail():
    """n = 16, all 2^16 outcomes: P(|S| >= |s_obs|) under the null model's mu against both approximations, s_obs the attainable value
    nearest 2.5 standard deviations."""
    n = 16
    outcomes = np.array(list(itertools.product((0.0, 1.0), repeat=n)))
    d_spa, d_norm, closer, done = [], [], 0, 0
    for k in range(60):
        rng = np.random.default_rng(8000 + k)
        Z = np.stack([np.ones(n), rng.standard_normal(n)], axis=1)
        eta = -1.2 + 0.4 * Z[:, 1]
        mu = P.sigma(eta)
        w = mu * (1 - mu)
        g = rng.binomial(2, 0.3, n).astype(np.float64)
        if len(set(g)) < 2:
            continue
        coef = np.linalg.solve(Z.T @ (w[:, None] * Z), Z.T @ (w * g))
        c = g - Z @ coef
        V = float(np.sum(c * c * w))
        stat = (outcomes - mu[None, :]) @ c
        prob = np.prod(np.where(outcomes == 1.0, mu[None, :], 1 - mu[None, :]), axis=1)
        q = float(stat[np.argmin(np.abs(np.abs(stat) - 2.5 * math.sqrt(V)))])
        exact = float(prob[np.abs(stat) >= abs(q) - 1e-12].sum())
        nlp = float(S.neglog10p(np.array([q / math.sqrt(V)]))[0])
        st, val, _, _, _ = P.column(c, eta, q, V, nlp)
        if st != 1:
            continue
        done += 1
        d_spa.append(abs(val + math.log10(exact)))
        d_norm.append(abs(nlp + math.log10(exact)))
        closer += d_spa[-1] < d_norm[-1]
        if done == 30:
            break
    assert done == 30
    print(f"exact distribution: mean |dlog10 p| saddlepoint {np.mean(d_spa):.3g}, normal {np.mean(d_norm):.3g}; closer in {closer} of 30")
    assert np.mean(d_spa) < np.mean(d_norm)


# ---- 7. the GPU test's inputs -----------------------------------------------------------------------------------------------------------
def test_margins_redraw_few_columns_and_the_spec_error_on_these_inputs():
    """The share of columns redrawn for an unclear decision stays below the cap, the planted boundary column of the intercept-only
    cases reaches state 2, and the spec's own error against mpmath on one tried column of every case stays below spa_spec.SPEC_ERR,
    the figure the device tolerance is built on."""
    worst, checked, shares = 0.0, 0, []
    cases = P.edge_cases()
    assert sorted(set(c[0] for c in cases)) == sorted(P.EDGE_N) and sorted(set(c[1] for c in cases)) == sorted(P.EDGE_P)
    assert set(c[2] for c in cases) == set(P.EDGE_C) and all(3 * c[2] <= c[0] for c in cases)
    for case in cases + list(P.EXTRA_CASES):
        n, p, c = case[:3]
        codes, y, eta, A, w, Z, share = P.edge_inputs(case)
        assert share <= P.MAX_REDRAWN, (case, share)
        shares.append(share)
        assert 2 <= y.sum() <= 0.16 * n + 3 * c, case
        sp = S.score(codes, case[4], A, w, Z)
        res = P.spa(sp, eta, Z, P.CUTOFF)
        if p >= 31:
            assert np.array_equal(np.flatnonzero(sp["deg"]), [3, 17, p - 2]) and (res["state"][sp["deg"]] == 0).all()
            if c == 1:
                assert res["state"][7] == 2, case
        ones = np.flatnonzero(res["state"] == 1)
        for j in ones[len(ones) // 2:][:1]:
            ref = mp_neglog10p(res["detail"][j]["c"], eta, sp["U"][j, 0])
            assert ref is not None, (case, j)
            worst = max(worst, rel_err_in_logp(res["neglog10p_spa"][j], ref))
            checked += 1
    print(f"largest share of columns redrawn for an unclear decision: {max(shares):.3g}")
    print(f"spec against mpmath on the edge inputs: {checked} columns, worst relative error in log p {worst:.3g} (SPEC_ERR {P.SPEC_ERR:.3g})")
    assert checked >= 20 and worst <= P.SPEC_ERR


# ---- 8. csrc/spa_finish.h -----------------------------------------------------------------------------------------------------------------
def build(tmp_path, sanitize):
    exe = tmp_path / ("spa_san" if sanitize else "spa")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mendeliht.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "spa_finish_harness.cpp"), "-o", str(exe)]
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
        res = P.spa(sp, eta, Z, 0.0)
        for j, d in res["detail"].items():
            text.append(f"{case[0]} {float(sp['U'][j, 0])!r} {float(sp['V'][j])!r} {float(res['neglog10p'][j])!r}")
            text += [f"{float(ci)!r} {float(hi)!r}" for ci, hi in zip(d["c"], eta)]
            want.append((int(res["state"][j]), float(res["neglog10p_spa"][j]), res["t_hat"][j], [tl["evals"] if tl else 0 for tl in d["tails"]]))
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    print(f"harness: {len(want)} columns")
    assert len(rows) == len(want) and len(want) > 60
    states = set()
    for row, (st, val, that, evals) in zip(rows, want):
        assert int(row[0]) == st and [int(row[4]), int(row[5])] == evals, (row, st, evals)
        assert abs(float(row[1]) - val) <= 1e-13 * abs(val), (row, val)
        got_t = np.array([float(row[2]), float(row[3])])
        assert np.array_equal(np.isnan(got_t), np.isnan(that)) and np.allclose(got_t, that, rtol=1e-13, atol=0, equal_nan=True), (row, that)
        states.add(st)
    assert states == {1, 2}
