"""The kinship matrix and the related-pair screen on the device (csrc/grm.hip: mih_grm, mih_grm_pairs; grm and related_pairs
of SnpLinAlg and DosageMatrix) against the numpy statement tests/grm_spec.py.

Tolerance, derived and not measured: u = 2^-53, S = |X| |X|' (|C| |C|' for Robust) over the m kept columns, div the method's
divisor.  Any order of an m-term float64 sum is within m u S_ik of the exact value, numpy's too, and the entries carry at
most two roundings each: |Phi_dev - Phi_spec|_ik <= 2 (m + 8) u S_ik / div + 1e-300, elementwise (grm_spec.bound).

The shapes are those where the kernels change path: one sample, the 16 rows of a matrix-core block and of a dword of the
2-bit image, the 64 rows of a wave's share of the tile, the 128 of the tile and of the block pair, more than one tile (257:
a 3 x 3 triangle of tile pairs), and column counts around the 4 of a matrix-core step and the 8 of an LDS stage, across
several panels (panel_cols 4, 32, 64 against up to 150 columns)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grm_spec as K
import qc_spec as Q
from conftest import FIX, free_device_bytes
from test_gpu_hardcall_pack import MISSING, codes_of, edge_codes, from_bed, numerators

from mendeliht_amd import api

pytestmark = pytest.mark.gpu

EDGE_N = [1, 15, 16, 17, 63, 65, 127, 128, 129, 257]
EDGE_P = [1, 3, 4, 5, 33, 70, 150]
PANELS = [0, 4, 32, 64]
BAD_ARG = 2


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def selections(p, rng):
    half = rng.random(p) < 0.5
    half[rng.integers(p)] = True
    one = np.zeros(p, dtype=bool)
    one[rng.integers(p)] = True
    return [("all", np.ones(p, dtype=bool)), ("half", half), ("one", one)]


def last_error(mih):
    buf = C.create_string_buffer(512)
    mih.lib().mih_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
def test_edge_shapes(mih, n):
    for p in EDGE_P:
        codes = edge_codes(n, p, 9000 * n + p)
        x = from_bed(mih, codes)
        g = K.genotypes(codes)
        mu, sinv = x.mu_sigma()
        rng = np.random.default_rng(31 * n + p)
        r = rng.standard_normal(n)
        before = x.xtv(r)
        for name, cols in selections(p, rng):
            for method in K.METHODS:
                want, tol = K.grm(g, mu, sinv, cols, method), K.bound(g, mu, sinv, cols, method)
                first = None
                for pc in PANELS:
                    what = (n, p, name, method, pc)
                    phi = x.grm(method=method, cols=cols, panel_cols=pc)
                    K.check(phi, want, tol, what)
                    assert bits(phi) == bits(phi.T), what                                    # Phi == Phi', bit for bit
                    assert bits(x.grm(method=method, cols=cols, panel_cols=pc)) == bits(phi), what      # and so is a second call
                    first = phi if first is None else first
                    assert bits(phi) == bits(first), what            # one chain over the columns, however they are cut into panels
        assert bits(x.xtv(r)) == bits(before), (n, p)                # the source is only read


def test_index_selection_and_method_names(mih):
    codes = edge_codes(65, 70, 5)
    x = from_bed(mih, codes)
    idx = np.array([0, 5, 6, 33, 69])
    mask = np.zeros(70, dtype=bool)
    mask[idx] = True
    assert bits(x.grm(cols=idx)) == bits(x.grm(cols=mask)) == bits(x.grm(method=0, cols=mask, panel_cols=3))
    with pytest.raises(api.ArgumentError, match="MoM"):
        x.grm(method="MoM")
    with pytest.raises(api.ArgumentError):
        x.grm(cols=idx[::-1])


# ---- 2. the shipped fixture ---------------------------------------------------------------------------------------------------
def test_shipped_fixture_with_the_default_minmaf(mih):
    n = 1000
    bed = mih.read_bed(os.path.join(FIX, "normal.bed"), n)
    x = mih.SnpLinAlg(bed, n, center=True, scale=True, impute=True)
    codes = codes_of(bed, n)
    assert codes.shape == (1000, 10000)
    with np.errstate(invalid="ignore"):
        keep = Q.maf(Q.counts(codes)[0]) >= 0.01
        assert int(np.count_nonzero(x.maf() >= 0.01)) == int(np.count_nonzero(keep)) and 0 < np.count_nonzero(keep)
    g = K.genotypes(codes)
    mu, sinv = x.mu_sigma()
    for method in K.METHODS:
        phi = x.grm(method=method)
        K.check(phi, K.grm(g, mu, sinv, keep, method), K.bound(g, mu, sinv, keep, method), method)
        assert bits(phi) == bits(phi.T)


# ---- 3. a sample without any genotype -------------------------------------------------------------------------------------------
def test_a_row_with_every_genotype_missing(mih):
    codes = edge_codes(129, 70, 77).copy()
    codes[64] = -1
    x = from_bed(mih, codes)
    d = mih.DosageMatrix(numerators(codes, unit=1), 2)
    g = K.genotypes(codes)
    for h, gg in ((x, g), (d, g / 2.0)):
        mu, sinv = h.mu_sigma()
        for method in K.METHODS:
            phi = h.grm(method=method, cols=np.ones(70, dtype=bool), panel_cols=32)
            assert np.all(phi[64] == 0.0) and np.all(phi[:, 64] == 0.0)
            K.assert_within(phi, gg, mu, sinv, None, method, method)


# ---- 4. dosage handles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 129])
@pytest.mark.parametrize("p", [5, 70])
def test_dosage_handles(mih, n, p):
    hard = mih.DosageMatrix(numerators(edge_codes(n, p, 300 * n + p), unit=1), 2)
    fine = mih.DosageMatrix.synthetic(n, p, seed=17 * n + p, denom=255, missing_rate=0.05)
    rng = np.random.default_rng(n + p)
    for d in (hard, fine):
        num = d.export()
        g = np.where(num == MISSING, np.nan, num / float(d.denom))
        mu, sinv = d.mu_sigma()                                      # the handle's own
        r = rng.standard_normal(n)
        before = d.xtv(r)
        for name, cols in selections(p, rng)[:2]:
            for method in K.METHODS:
                want, tol = K.grm(g, mu, sinv, cols, method), K.bound(g, mu, sinv, cols, method)
                for pc in (0, 4):
                    phi = d.grm(method=method, cols=cols, panel_cols=pc)
                    K.check(phi, want, tol, (d.denom, name, method, pc))
                    assert bits(phi) == bits(phi.T)
        assert bits(d.xtv(r)) == bits(before)
    # the default column rule of a dosage handle: min(mu / 2, 1 - mu / 2) >= minmaf
    mu, sinv = fine.mu_sigma()
    keep = np.minimum(mu / 2.0, 1.0 - mu / 2.0) >= 0.05
    assert keep.any() and bits(fine.grm(minmaf=0.05)) == bits(fine.grm(cols=keep))


# ---- 5. related pairs -----------------------------------------------------------------------------------------------------------
DUP = (10, 200)
TRIOS = ((20, 21, 150), (40, 260, 41), (299, 100, 101))             # parent, parent, child


def family_codes():
    rng = np.random.default_rng(2024)
    n, p = 300, 2000
    f = rng.uniform(0.1, 0.5, p)
    codes = rng.binomial(2, f[None, :], size=(n, p))
    codes[DUP[1]] = codes[DUP[0]]
    for a, b, c in TRIOS:                                            # the child draws one allele from each parent
        codes[c] = (rng.random(p) < codes[a] / 2.0).astype(int) + (rng.random(p) < codes[b] / 2.0)
    codes[rng.random((n, p)) < 0.01] = -1
    return codes


PLANTED = sorted([DUP] + [tuple(sorted((par, c))) for a, b, c in TRIOS for par in (a, b)])


@pytest.fixture(scope="module")
def family(mih):
    codes = family_codes()
    x = from_bed(mih, codes)
    phi = x.grm()
    phi.setflags(write=False)
    return codes, x, phi


def test_related_pairs_are_the_devices_own_matrix_above_the_threshold(mih, family):
    codes, x, phi = family
    g = K.genotypes(codes)
    mu, sinv = x.mu_sigma()
    with np.errstate(invalid="ignore"):
        keep = Q.maf(Q.counts(codes)[0]) >= 0.01
    want, tol = K.grm(g, mu, sinv, keep, "GRM"), K.bound(g, mu, sinv, keep, "GRM")
    K.check(phi, want, tol)
    low = np.tril_indices(300, -1)
    assert np.all(np.abs(want[low] - 0.125) > tol[low])              # no spec value within the bound of the threshold
    i, k, v, diag = x.related_pairs(0.125)
    wi, wk = K.related_pairs(phi, 0.125)
    assert i.dtype == np.int64 and k.dtype == np.int64
    assert np.array_equal(i, wi) and np.array_equal(k, wk) and bits(v) == bits(phi[wi, wk])
    assert list(zip(i.tolist(), k.tolist())) == PLANTED              # the planted pairs and only they
    assert bits(diag) == bits(np.diag(phi))
    # the recipe of the docstring
    mask = np.zeros(300, dtype=bool)
    mask[k] = True
    y = x.subset(rows=~mask)
    assert y.n == 300 - len(set(k.tolist())) and y.related_pairs(0.125)[0].size == 0


def test_threshold_is_strict_and_methods_agree_with_their_own_matrix(mih, family):
    codes, x, phi = family
    i, k, v, _ = x.related_pairs(0.125)
    t = 3
    j, l, w, _ = x.related_pairs(float(v[t]))                        # one pair's exact value excludes that pair
    stay = v > v[t]
    assert np.array_equal(j, i[stay]) and np.array_equal(l, k[stay]) and bits(w) == bits(v[stay]) and 0 < j.size < i.size
    rob = x.grm(method="Robust", panel_cols=64)
    i, k, v, diag = x.related_pairs(0.125, method="Robust", panel_cols=64)
    wi, wk = K.related_pairs(rob, 0.125)
    assert np.array_equal(i, wi) and np.array_equal(k, wk) and bits(v) == bits(rob[wi, wk]) and bits(diag) == bits(np.diag(rob))
    i, k, v, _ = x.related_pairs(-1.0, cols=np.arange(0, 2000, 7))   # every pair of the 300: the list is the strict triangle
    sub = x.grm(cols=np.arange(0, 2000, 7))
    wi, wk = np.triu_indices(300, 1)
    assert np.array_equal(i, wi) and np.array_equal(k, wk) and bits(v) == bits(sub[wi, wk])


def test_cap_cuts_the_list_and_reports_the_full_count(mih, family):
    codes, x, phi = family
    full = x.related_pairs(0.125)
    ck = (x.maf() >= 0.01).astype(np.uint8)
    ri, rk, rv = np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int64), np.full(4, -7.0)
    count = C.c_int64(-1)
    rc = mih.lib().mih_grm_pairs(x._h, ptr(ck), 0, 0, 0.125, 1, ptr(ri), ptr(rk), ptr(rv), C.byref(count), None)
    assert rc == 0 and count.value == len(PLANTED)
    assert (ri[0], rk[0]) == PLANTED[0] and rv[0] == full[2][0]
    assert np.all(ri[1:] == -7) and np.all(rk[1:] == -7) and np.all(rv[1:] == -7.0)         # nothing beyond cap is written
    count = C.c_int64(-1)
    assert mih.lib().mih_grm_pairs(x._h, ptr(ck), 0, 0, 0.125, 0, None, None, None, C.byref(count), None) == 0
    assert count.value == len(PLANTED)
    i, k, v, diag = x.related_pairs(0.125, cap=3)
    assert np.array_equal(i, full[0][:3]) and np.array_equal(k, full[1][:3]) and bits(v) == bits(full[2][:3])
    got = x.related_pairs(0.125, _first_cap=2)                       # cap = None with a first cap that is too small
    for a, b in zip(got, full):
        assert bits(a) == bits(b) and a.shape == b.shape


# ---- 5b. an accumulator of more than 2^31 entries -------------------------------------------------------------------------------
def test_an_accumulator_with_more_than_2_to_31_entries(mih):
    """46 400 samples: the accumulator has 46 464^2 = 2.16e9 entries, so a 32-bit index anywhere in the update, the pair scan
    or the diagonal would show in the far rows.  Eight columns keep the arithmetic small; the host checks the whole diagonal,
    and the whole pair list through Cauchy-Schwarz: Phi_ik^2 <= Phi_ii Phi_kk, so only rows with a large Phi_ii can be in a pair."""
    n, p, thr = 46_400, 8, 0.9
    rng = np.random.default_rng(99)
    codes = rng.binomial(2, 0.5, size=(n, p))
    codes[rng.random((n, p)) < 0.01] = -1
    codes[n - 1] = codes[n - 2] = 2 * (np.arange(p) % 2)             # identical all-homozygous rows in the far corner ...
    codes[46_000] = codes[5] = 2 - 2 * (np.arange(p) % 2)            # ... and across the whole height
    x = from_bed(mih, codes)
    mu, sinv = x.mu_sigma()
    a, div = K.operand(K.genotypes(codes), mu, sinv, None, "GRM")
    scale = 2.0 * (p + 8) * K.U / div
    want_diag = (a * a).sum(axis=1) / div
    i, k, v, diag = x.related_pairs(thr, cols=np.ones(p, dtype=bool), cap=200_000)
    assert np.all(np.abs(diag - want_diag) <= scale * div * want_diag + 1e-300)
    cand = np.flatnonzero(want_diag * want_diag.max() >= thr * thr * (1.0 - 1e-9))
    assert 2 <= cand.size <= 5000
    sub, tol = (a[cand] @ a[cand].T) / div, scale * (np.abs(a[cand]) @ np.abs(a[cand]).T) + 1e-300
    up = np.triu_indices(cand.size, 1)
    assert np.all(np.abs(sub[up] - thr) > tol[up])                   # no spec value within the bound of the threshold
    ii, kk = np.nonzero(np.triu(sub > thr, 1))
    assert np.array_equal(i, cand[ii]) and np.array_equal(k, cand[kk]) and i.size < 200_000
    assert np.all(np.abs(v - sub[ii, kk]) <= tol[ii, kk])
    found = set(zip(i.tolist(), k.tolist()))
    assert (n - 2, n - 1) in found and (5, 46_000) in found


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(mih):
    L = mih.lib()
    codes = edge_codes(17, 5, 1)
    x = from_bed(mih, codes)
    dense = mih.DenseMatrix(np.random.default_rng(0).standard_normal((17, 5)))
    out = np.full((17, 17), -7.0)
    ri, rk, rv = np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int64), np.full(4, -7.0)
    diag = np.full(17, -7.0)
    none = np.zeros(5, dtype=np.uint8)

    def pairs(h, ck, method, thr, cap):
        count = C.c_int64(-7)
        rc = L.mih_grm_pairs(h, None if ck is None else ptr(ck), method, 0, thr, cap, ptr(ri), ptr(rk), ptr(rv), C.byref(count), ptr(diag))
        return rc, count.value

    for what, call in (("dense", lambda: L.mih_grm(dense._h, None, 0, 0, ptr(out))),
                       ("empty", lambda: L.mih_grm(x._h, ptr(none), 0, 0, ptr(out))),
                       ("method", lambda: L.mih_grm(x._h, None, 7, 0, ptr(out)))):
        assert call() == BAD_ARG and last_error(mih), what
        assert np.all(out == -7.0), what
    for what, args in (("dense", (dense._h, None, 0, 0.125, 4)), ("empty", (x._h, none, 1, 0.125, 4)), ("method", (x._h, None, 7, 0.125, 4)),
                       ("nan", (x._h, None, 0, float("nan"), 4)), ("cap", (x._h, None, 0, 0.125, -1))):
        rc, count = pairs(*args)
        assert rc == BAD_ARG and count == -7 and last_error(mih), what
        assert np.all(ri == -7) and np.all(rk == -7) and np.all(rv == -7.0) and np.all(diag == -7.0), what
    with pytest.raises(api.ArgumentError):
        x.grm(cols=np.zeros(5, dtype=bool))
    with pytest.raises(api.ArgumentError):
        x.related_pairs(float("nan"))
    assert np.all(np.isfinite(x.grm(cols=np.ones(5, dtype=bool))))   # and the handle still serves


def test_a_matrix_the_device_cannot_hold_is_refused_before_anything_is_allocated(mih):
    x = mih.SnpLinAlg.synthetic(300_000, 32)
    before = free_device_bytes()
    with pytest.raises(MemoryError) as e:
        x.grm()
    need, free = (int(v) for v in re.findall(r"(\d{9,}) bytes", str(e.value)))
    assert need >= 8 * 300_032 ** 2 and need > free and abs(free - before) <= 64 << 20
    with pytest.raises(MemoryError):
        x.related_pairs()
    assert abs(free_device_bytes() - before) <= 64 << 20
