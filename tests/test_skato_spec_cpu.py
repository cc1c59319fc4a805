"""tests/skato_spec.py, the numpy statement of SKAT-O, held to independent references on the CPU: the closed form of M_rho against
the Cholesky form, the quantiles by a round trip through the tail, every state, the one-member identity, a seeded Monte Carlo of
the min-p statistic, the whole value against 50-digit mpmath (SPEC_ERR_O, with the quadrature's share of it with and without
panels cut at the kinks), the margins of the device test's inputs, and csrc/skato_tail.h -- the host step and the integrand --
compiled into tests/skato_tail_harness.cpp with g++ (plainly and under -fsanitize=address,undefined, a stand-alone program)."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import sets_spec as T
import skato_spec as K
from conftest import ROOT

LN10 = math.log(10.0)


@functools.lru_cache(maxsize=None)
def inputs(k, grid=None):
    return K.inputs(K.CASES[k], grid)


def random_set(rng, m, shift=0.0, scale=1.6):
    """dict like a set's detail of sets_spec.set_test from a random covariance M and a score drawn from it."""
    B = rng.standard_normal((m, max(40, 2 * m))) + shift
    M = B @ B.T / B.shape[1]
    M = np.tril(M) + np.tril(M, -1).T
    a = np.linalg.cholesky(M) @ rng.standard_normal(m) * scale
    rs = K.row_sums(M)
    Q = K.dot_fixed(a, a)
    return dict(M=M, S=float(rs.sum()), T=float(a.sum()), Q=Q, tail=T.skat_tail(T.eigenvalues(M), Q))


# ---- 1. M_rho ---------------------------------------------------------------------------------------------------------------------------
def test_the_closed_form_of_m_rho_has_the_eigenvalues_of_the_cholesky_form():
    rng = np.random.default_rng(1)
    for m in (1, 2, 3, 17, 64):
        d = random_set(rng, m, shift=0.3)
        rs = K.row_sums(d["M"])
        for rho in K.grid_of(K.GRID16):
            A = K.m_rho(d["M"], rs, d["S"], float(rho))
            L = np.linalg.cholesky((1 - rho) * np.eye(m) + rho * np.ones((m, m)))
            want = np.linalg.eigvalsh(L.T @ d["M"] @ L)
            got = np.linalg.eigvalsh(A)
            assert np.abs(got - want).max() <= 64 * m * T.U * np.abs(want).max(), (m, rho)
            assert np.array_equal(A, A.T)
        assert np.array_equal(K.m_rho(d["M"], rs, d["S"], 0.0), d["M"])                  # rho = 0: M itself, to the bit
        Mt = K.m_tilde(d["M"], rs, d["S"])
        assert np.abs(Mt @ np.ones(m)).max() <= 64 * m * T.U * np.abs(d["M"]).sum()       # M~ annihilates 1


# ---- 2. the quantiles ---------------------------------------------------------------------------------------------------------------------
def test_quantiles_round_trip_through_the_tail():
    """tail_rho(q_rho) against p_min.  The iteration stops at 2^-40 relative in log p, the tail's own root at 2^-40 relative in Q
    followed by a Newton step (an error of the second order), and both evaluate w^2 = s q + sum log1p(-mu s) with the cancellation
    sets_spec.SPEC_ERR describes.  Where that noise keeps the iteration from its first tolerance it stops on a bracket of 2^-40
    relative in y = 1 / (1 - s); log p moves by |d log p / d log y| of that, and with q ~ lambda_1 (y + const) and
    -log p ~ q / (2 lambda_1) - (m / 2) log q the slope is below 16 |log p| for m <= 128 away from p = 1.  Together:
    (4 + 16) x 2^-40 + 2 SPEC_ERR relative, and 1e-13 absolute for the values near 0."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for m, shift, scale in ((2, 0, 1.6), (3, 0, 1), (5, 0.5, 2.5), (17, 0.8, 1.6), (40, 0, 6.0)):
        d = random_set(rng, m, shift, scale)
        ev, p = K.set_skato(d, K.grid_of(K.GRID16))
        assert ev["state"] in (K.INTEGRAL, K.CLAMPED), (m, ev["state"])
        pmin = ev["nlp_rho"].max()
        for r in range(16):
            back = T.skat_tail(p["lam_rho"][r], ev["q"][r])["neglog10p"]
            err = abs(back - pmin)
            worst = max(worst, err / pmin)
            assert err <= (20 * K.TOL_P + 2 * T.SPEC_ERR) * pmin + 1e-13, (m, r, back, pmin)
        assert ev["q"][ev["rho"]] == (1 - K.grid_of(K.GRID16)[ev["rho"]]) * d["Q"] + K.grid_of(K.GRID16)[ev["rho"]] * d["T"] ** 2
    # a rank-one lambda^(rho): the chi2_1 quantile
    q = K.chi1_quantile(2.5, 7.0)
    assert abs(T.skat_tail([2.5], q)["neglog10p"] - 7.0) <= 1e-12
    print(f"quantile round trip: worst relative error in log p {worst:.3g}")


# ---- 3. the states ------------------------------------------------------------------------------------------------------------------------
def test_every_state_and_the_one_member_identity():
    rng = np.random.default_rng(3)
    grid = K.grid_of()
    d = random_set(rng, 1)
    ev, _ = K.set_skato(d, grid)
    assert ev["state"] == K.RANK_ONE and ev["neglog10p"] == d["tail"]["neglog10p"] and d["tail"]["state"] == 2 and ev["rho"] == -1
    d = random_set(rng, 5)
    ev, p = K.set_skato(d, grid)
    assert ev["state"] == K.INTEGRAL and ev["nlp_rho"][0] == d["tail"]["neglog10p"]
    assert ev["nlp_rho"].max() - math.log10(8) <= ev["neglog10p"] <= ev["nlp_rho"].max()
    one, _ = K.set_skato(d, K.grid_of((0.0,)))                  # R = 1: the interval [p_min, R p_min] is a point
    assert one["state"] == K.CLAMPED and one["neglog10p"] == d["tail"]["neglog10p"]
    none = dict(d, S=-1.0)
    assert K.set_skato(none, grid)[0]["state"] == K.NONE and math.isnan(K.set_skato(none, grid)[0]["neglog10p"])
    empty = dict(M=np.zeros((0, 0)), S=0.0, T=0.0, Q=0.0, tail=T.skat_tail([], 0.0))
    assert K.set_skato(empty, grid)[0]["state"] == K.NONE
    zero = dict(d, T=0.0, Q=0.0, tail=T.skat_tail(T.eigenvalues(d["M"]), 0.0))          # Q_rho = 0 everywhere: p = 1
    ev0, _ = K.set_skato(zero, grid)
    assert ev0["state"] == K.FALLBACK and ev0["neglog10p"] == 0.0 and (ev0["st_rho"] == 4).all()
    tiny = dict(d, T=1e-160, Q=1e-300, tail=T.skat_tail(T.eigenvalues(d["M"]), 1e-300))   # the root iteration gives up: state 5
    evt, _ = K.set_skato(tiny, grid)
    assert evt["state"] == K.FALLBACK and (evt["st_rho"] == 5).any()
    # the device test's inputs hold every state, within the redraw rule
    states = set()
    for k in range(len(K.CASES)):
        sk, share = inputs(k)[8:10]
        assert share <= K.MAX_REDRAWN, (k, share)
        assert all(K.clear(ev) for ev, _ in sk), k
        states |= {ev["state"] for ev, _ in sk}
        assert sorted(p["m"] for _, p in sk)[-3:] == [64, 65, 128], k
    for grid_ in ((0.0,), (1.0,), K.GRID16):
        sk, share = inputs(0, grid_)[8:10]
        assert share <= K.MAX_REDRAWN and all(K.clear(ev) for ev, _ in sk), grid_
        states |= {ev["state"] for ev, _ in sk}
    assert states >= {0, 1, 2, 3}                             # (the fallback: `zero` and `tiny` above, and zero scores on the device)
    top = len(K.DEFAULT_GRID) - 1
    assert inputs(2)[8][-1][0]["rho"] == top and inputs(3)[8][-1][0]["rho"] == 0      # same-sign scores: the burden end; alternating: SKAT


# ---- 4. Monte Carlo -----------------------------------------------------------------------------------------------------------------------
def test_a_monte_carlo_of_the_min_p_statistic():
    """P(min_rho p_rho <= p_min) under the null is P(some Q_rho > q_rho): 20 000 seeded draws of a ~ N(0, M), within 4 standard
    errors of the spec's integral."""
    rng = np.random.default_rng(4)
    grid = K.grid_of()
    for m, shift in ((5, 0.0), (17, 0.8)):
        d = random_set(rng, m, shift)
        ev, _ = K.set_skato(d, grid)
        assert ev["state"] == K.INTEGRAL
        Z = np.linalg.cholesky(d["M"]) @ rng.standard_normal((m, 20000))
        Td, Qd = Z.sum(axis=0), (Z * Z).sum(axis=0)
        hit = np.zeros(Z.shape[1], dtype=bool)
        for r, rho in enumerate(grid):
            hit |= (1 - rho) * Qd + rho * Td * Td > ev["q"][r]
        pm = 10.0 ** -ev["nlp_int"]
        se = math.sqrt(pm * (1 - pm) / hit.size)
        print(f"monte carlo m = {m}: {hit.mean():.4f} against {pm:.4f} +- {se:.4f}")
        assert abs(hit.mean() - pm) <= 4 * se, (m, hit.mean(), pm, se)


# ---- 5. the spec against mpmath -----------------------------------------------------------------------------------------------------------
def mp_tail(mp, lam, Q):
    """the saddlepoint tail (not its logarithm) in mpmath; 1 at Q <= 0"""
    if Q <= 0:
        return mp.mpf(1)
    lam = sorted((v for v in lam if v > 0), reverse=True)
    if len(lam) == 1 or lam[1] <= mp.mpf(2) ** -40 * lam[0]:     # rank one: the exact chi2_1 tail (state 2)
        return mp.erfc(mp.sqrt(Q / lam[0] / 2))
    l1 = max(lam)
    mus = [v / l1 for v in lam]
    q = Q / l1
    sx, lo, hi = mp.mpf(0), None, mp.mpf(1)                    # the safeguarded Newton iteration of sets_spec.root, to 1e-45
    for _ in range(400):
        g = sum(u / (1 - u * sx) for u in mus)
        g2 = sum((u / (1 - u * sx)) ** 2 for u in mus)
        f = g - q
        if abs(f) <= mp.mpf(10) ** -45 * q:
            break
        if f < 0:
            lo = sx
        else:
            hi = sx
        sn = sx - f / g2
        if not ((lo is None or lo < sn) and sn < hi):
            sn = (sx + hi) / 2 if f < 0 else ((lo + sx) / 2 if lo is not None else (2 * sx if sx < 0 else -mp.mpf(1)))
        sx = sn
    t = sx / (2 * l1)
    Kt = -sum(mp.log1p(-2 * v * t) for v in lam) / 2
    K2 = 2 * sum((v / (1 - 2 * v * t)) ** 2 for v in lam)
    w = mp.sign(t) * mp.sqrt(2 * (t * Q - Kt))
    if abs(w) < mp.mpf(10) ** -20:                              # at the mean: the limit of r
        r = (8 * sum(v ** 3 for v in lam) / (2 * sum(v * v for v in lam)) ** mp.mpf("1.5")) / 6
    else:
        r = w + mp.log(t * mp.sqrt(K2) / w) / w
    return mp.erfc(r / mp.sqrt(2)) / 2


def mp_skato(d, grid):
    """-log10 of the SKAT-O integral of a set in 50-digit mpmath: eigenvalues by mpmath.eigsy, the quantiles by root finding on the
    tail, the integral by mpmath.quad split at the kinks of delta."""
    import mpmath as mp
    mp.mp.dps = 50
    M = mp.matrix(d["M"].tolist())
    m = M.rows
    one = mp.ones(m, 1)
    rs = M * one
    S = sum(rs)
    Q, Tt = mp.mpf(d["Q"]), mp.mpf(d["T"])
    lams, qs, taus = [], [], []
    tails = []
    for rho in grid:
        rho = mp.mpf(float(rho))
        c = mp.sqrt(1 - rho)
        dd = (mp.sqrt(1 - rho + m * rho) - c) / m
        Mr = c * c * M + c * dd * (rs * one.T + one * rs.T) + dd * dd * S * one * one.T
        lam = [v for v in mp.eigsy(Mr, eigvals_only=True)]
        lams.append(lam)
        tails.append(mp_tail(mp, lam, (1 - rho) * Q + rho * Tt * Tt))
        taus.append(rho * S + (1 - rho) * (rs.T * rs)[0] / S)
    pmin = min(tails)
    best = tails.index(pmin)
    for r, rho in enumerate(grid):
        rho = mp.mpf(float(rho))
        Qr = (1 - rho) * Q + rho * Tt * Tt
        if r == best:
            qs.append(Qr)
            continue
        lam = lams[r]
        mean = sum(v for v in lam if v > 0)
        hi = max(Qr, mean)
        while mp_tail(mp, lam, hi) > pmin:
            hi *= 2
        lo_, hi_ = Qr, hi
        for _ in range(180):
            mid = (lo_ + hi_) / 2
            if mp_tail(mp, lam, mid) > pmin:
                lo_ = mid
            else:
                hi_ = mid
        qs.append((lo_ + hi_) / 2)
    Mt = M - rs * rs.T / S
    lam_t = [v for v in mp.eigsy(Mt, eigvals_only=True) if v > mp.mpf(10) ** -30 * abs(S)]
    mu = sum(lam_t)
    vxi = 4 * (rs.T * Mt * rs)[0] / S
    v = 2 * sum(x * x for x in lam_t) + vxi
    kf = mp.sqrt((v - vxi) / v)
    omr = [1 - mp.mpf(float(r)) for r in grid]
    x0 = min(q / t for q, t in zip(qs, taus))
    u0 = mp.sqrt(x0)

    def f(u):
        x = u * u
        dl = min((qs[r] - taus[r] * x) / omr[r] for r in range(len(grid)))
        dp = (dl - mu) * kf + mu
        return mp_tail(mp, lam_t, dp) * mp.npdf(u)
    kn = K.kinks([float(q) for q in qs], [float(t) for t in taus], [float(g) for g in grid], float(x0))
    pts = [mp.mpf(0)] + [mp.sqrt(mp.mpf(x)) for x in kn] + [u0]
    mp.mp.dps = 30
    val = 2 * mp.quad(f, pts) + mp.erfc(u0 / mp.sqrt(2))
    return float(-mp.log10(val))


def test_the_spec_against_mpmath_on_the_device_tests_sets():
    """SPEC_ERR_O: the relative error in log p of the spec's integral on the sets of tests/test_gpu_assoc_skato.py (those in the
    integral state with at most 17 members -- mpmath.eigsy and a nested root per node bound what a test can afford), and the same
    with 16 equal panels, not cut at the kinks."""
    worst = cut = 0.0
    checked = 0
    grid = K.grid_of()
    for k, picks in ((0, (1, 2, 3)), (1, (1, 2, 7, 8, 10))):      # 2, 3, 17 and 2, 3, 4, 3 (the spec's worst), 8 members
        res, sk = inputs(k)[7:9]
        for s in picks:
            d, (ev, p) = res["detail"][s], sk[s]
            assert ev["state"] == K.INTEGRAL and 2 <= p["m"] <= 17, (k, s)
            ref = mp_skato(d, grid)
            e1 = abs(ev["nlp_int"] - ref) / ref
            e2 = abs(K.set_skato(d, grid, cut=False)[0]["nlp_int"] - ref) / ref
            print(f"case {k} m = {p['m']}: spec {ev['nlp_int']:.10g} mpmath {ref:.10g} relative error {e1:.3g}, with 16 equal panels {e2:.3g}")
            worst, cut = max(worst, e1), max(cut, e2)
            checked += 1
    print(f"spec against mpmath: {checked} sets, worst relative error in log p {worst:.3g} (SPEC_ERR_O {K.SPEC_ERR_O:.3g}); "
          f"with 16 equal panels {cut:.3g} ({K.SPEC_ERR_O_EQUAL_PANELS:.3g})")
    assert checked == 8 and worst <= 2 * K.SPEC_ERR_O and cut <= 2 * K.SPEC_ERR_O_EQUAL_PANELS


# ---- 6. csrc/skato_tail.h -----------------------------------------------------------------------------------------------------------------
def build(tmp_path, sanitize):
    exe = tmp_path / ("skato_san" if sanitize else "skato")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mendeliht.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "skato_tail_harness.cpp"), "-o", str(exe)]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_step_against_the_spec(tmp_path, sanitize):
    """The states, skato_rho, p_rho, q_rho, tau_rho, u0 and the value of every set of the device test's inputs, and of sets that
    reach the states these do not.  p_rho and the quantiles agree as the quantile round trip does; the value to 1e-9 (the same
    256 terms in the same order, libm against numpy)."""
    exe = build(tmp_path, sanitize)
    items = []                                                  # (d, grid)
    for k, grid in ((0, None), (2, None), (0, (1.0,)), (0, K.GRID16)):
        res = inputs(k, grid)[7]
        items += [(d, K.grid_of(grid)) for d in res["detail"]]
    rng = np.random.default_rng(6)
    d5 = random_set(rng, 5)
    items += [(dict(d5, S=-1.0), K.grid_of()), (dict(d5, T=0.0, Q=0.0, tail=T.skat_tail(T.eigenvalues(d5["M"]), 0.0)), K.grid_of()),
              (dict(d5, T=1e-160, Q=1e-300, tail=T.skat_tail(T.eigenvalues(d5["M"]), 1e-300)), K.grid_of()),
              (random_set(rng, 9, 0.5, 9.0), K.grid_of()), (random_set(rng, 2, 0.0, 12.0), K.grid_of((0.0, 0.5)))]
    text, want = [], []
    for d, grid in items:
        ev, p = K.set_skato(d, grid)
        m = p["m"]
        text.append(f"{m} {len(grid)} {float(d['Q'])!r} {float(d['T'])!r} {float(d['S'])!r} {float(p['rr'])!r} {float(p['wt'])!r} "
                    f"{float(d['tail']['neglog10p'])!r} {int(d['tail']['state'])}")
        text.append(" ".join(repr(float(g)) for g in grid))
        for lam in p["lam_rho"] + [p["lam_t"]]:
            text.append(" ".join(repr(float(v)) for v in lam))
        want.append((ev, len(grid)))
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(want) + sum(R for _, R in want)

    def same(a, b, rel, ab=0.0):
        return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rel * abs(b) + ab

    i, states = 0, set()
    tolq = 20 * K.TOL_P + 2 * T.SPEC_ERR
    for ev, R in want:
        head, per = rows[i], rows[i + 1:i + 1 + R]
        i += 1 + R
        states.add(ev["state"])
        assert int(head[0]) == ev["state"] and int(head[1]) == ev["rho"], (head, ev)
        assert same(float(head[2]), ev["neglog10p"], 1e-9, 1e-13), (head, ev)
        for r in range(R):
            assert int(per[r][0]) == ev["st_rho"][r] and same(float(per[r][1]), ev["nlp_rho"][r], 1e-12, 1e-300), (per[r], ev)
        if ev["state"] in (K.INTEGRAL, K.CLAMPED):
            assert same(float(head[3]), ev["nlp_int"], 1e-9, 1e-13) and same(float(head[4]), ev["u0"], 1e-9) and same(float(head[5]), ev["mu"], 1e-13)
            for r in range(R):
                # a quantile's relative error is the tail's divided by |d log p / d log q| >= 1/2 beyond the mean; 1e-9 covers it
                assert same(float(per[r][2]), ev["q"][r], max(1e-9, 8 * tolq)) and same(float(per[r][3]), ev["tau"][r], 1e-13), (per[r], ev["q"][r])
    print(f"harness: {len(want)} sets, states {sorted(states)}")
    assert states == {0, 1, 2, 3, 4}


def test_the_entry_point_is_declared_and_exported():
    import re
    from mendeliht_amd import api
    hdr = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"\b(mih_[a-z0-9_]+)\s*\(", hdr))
    assert "mih_assoc_sets_skato" in declared and "mih_assoc_sets_skato" in api.exported_symbols()
    assert "assoc_skato.hip" in open(os.path.join(ROOT, "mendeliht.jl_amd", "csrc", "Makefile")).read()
    assert "SKAT-O" not in hdr.split("Not offered:")[1].split("*/")[0]
