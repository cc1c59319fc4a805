"""The numpy statement of the kinship matrix (tests/grm_spec.py) against exact rational arithmetic, and the interface of the
two entry points: the header declares them, the library exports them, the mirror offers them (no GPU needed)."""
import os
from fractions import Fraction

import numpy as np
import pytest

import grm_spec as K
from conftest import ROOT


def exact(g, mu, sinv, cols, method):
    """Phi in rational arithmetic from the float64 values of g, mu and sinv: nothing is rounded."""
    n, p = g.shape
    keep = [j for j in range(p) if cols is None or cols[j]]
    fin = [j for j in keep if np.isfinite(mu[j])]
    c = [[Fraction(0) if np.isnan(g[i, j]) or j not in fin else Fraction(float(g[i, j])) - Fraction(float(mu[j])) for j in keep]
         for i in range(n)]
    if method == "GRM":
        s = [Fraction(float(sinv[j])) for j in keep]
        c = [[v * sj for v, sj in zip(row, s)] for row in c]
        div = Fraction(2 * len(keep))
    else:
        div = 2 * sum((Fraction(float(mu[j])) * (1 - Fraction(float(mu[j])) / 2) for j in fin), Fraction(0))
    phi = [[sum((a * b for a, b in zip(c[i], c[k])), Fraction(0)) / div for k in range(n)] for i in range(n)]
    mag = [[sum((abs(a * b) for a, b in zip(c[i], c[k])), Fraction(0)) / div for k in range(n)] for i in range(n)]
    return phi, mag, len(keep)


def crafted():
    """17 x 9 allele counts: missing entries, a monomorphic column (3) and a column that is all missing (6)."""
    rng = np.random.default_rng(11)
    codes = rng.integers(0, 3, (17, 9))
    codes[rng.random((17, 9)) < 0.1] = -1
    codes[:, 3] = 2
    codes[:, 6] = -1
    return codes


@pytest.mark.parametrize("method", K.METHODS)
@pytest.mark.parametrize("cols", [None, np.arange(9) % 2 == 0])
def test_spec_against_exact_rational_arithmetic(method, cols):
    g = K.genotypes(crafted())
    mu, sinv = K.mu_sigma(g)
    assert np.isnan(mu[6]) and sinv[6] == 1.0 and mu[3] == 2.0 and sinv[3] == 1.0
    got = K.grm(g, mu, sinv, cols, method)
    tol = K.bound(g, mu, sinv, cols, method)
    phi, mag, m = exact(g, mu, sinv, cols, method)
    assert m == (9 if cols is None else 5) and np.all(np.isfinite(got))
    for i in range(17):
        for k in range(17):
            # the spec's own error: half the bound; the bound itself is 2 (m + 8) u S / div
            assert abs(Fraction(float(got[i, k])) - phi[i][k]) <= Fraction(float(tol[i, k])) / 2, (i, k)
            assert abs(Fraction(float(tol[i, k])) - 2 * (m + 8) * Fraction(1, 2 ** 53) * mag[i][k]) <= Fraction(float(tol[i, k])) / 1000, (i, k)
    assert np.array_equal(got, got.T)


@pytest.mark.parametrize("method", K.METHODS)
def test_two_identical_rows(method):
    codes = crafted()
    codes[9] = codes[4]
    g = K.genotypes(codes)
    mu, sinv = K.mu_sigma(g)
    phi = K.grm(g, mu, sinv, None, method)
    assert phi[4, 9] == phi[4, 4] == phi[9, 9] == phi[9, 4]
    assert np.array_equal(phi[4], phi[9])
    i, k = K.related_pairs(phi, phi[4, 9] - 1e-9)
    assert (4, 9) in set(zip(i.tolist(), k.tolist()))
    i, k = K.related_pairs(phi, phi[4, 9])                       # strictly above
    assert (4, 9) not in set(zip(i.tolist(), k.tolist()))


def test_hand_computed_example():
    """Three samples, two SNPs: genotypes (0, 1, 2) and (1, missing, 1).
    mu = (1, 1); sigma_1 = sqrt(1 * 1/2), so sinv_1 = sqrt(2); column 2 is monomorphic: sigma = sqrt(1/2) as well (mu = 1).
    c = [[-1, 0], [0, 0], [1, 0]] (the missing entry is imputed by the mean, the observed ones of column 2 equal it)."""
    g = np.array([[0.0, 1.0], [1.0, np.nan], [2.0, 1.0]])
    mu, sinv = K.mu_sigma(g)
    assert np.array_equal(mu, [1.0, 1.0]) and np.array_equal(sinv, [1.0 / np.sqrt(0.5)] * 2)
    s2 = (1.0 / np.sqrt(0.5)) ** 2                               # 2 up to the rounding of the root
    assert np.array_equal(K.grm(g, mu, sinv, None, "GRM"), np.array([[s2, 0, -s2], [0, 0, 0], [-s2, 0, s2]]) / 4.0)
    # Robust: the divisor is 2 (1/2 + 1/2) = 2
    assert np.array_equal(K.grm(g, mu, sinv, None, "Robust"), np.array([[0.5, 0, -0.5], [0, 0, 0], [-0.5, 0, 0.5]]))
    assert np.array_equal(K.grm(g, mu, sinv, [0], "Robust"), np.array([[1.0, 0, -1.0], [0, 0, 0], [-1.0, 0, 1.0]]))
    with pytest.raises(ValueError):
        K.grm(g, mu, sinv, np.zeros(2, dtype=bool), "GRM")
    with pytest.raises(ValueError):
        K.grm(g, mu, sinv, None, "MoM")


def test_an_all_missing_column_contributes_exactly_zero():
    g = K.genotypes(crafted())
    mu, sinv = K.mu_sigma(g)
    without = np.arange(9) != 6
    for method in K.METHODS:
        a, div = K.operand(g, mu, sinv, None, method)
        assert np.all(a[:, 6] == 0.0) and np.all(np.isfinite(a))
        b, div_b = K.operand(g, mu, sinv, without, method)
        assert np.array_equal(np.delete(a, 6, axis=1), b) and div == (div_b + 2 if method == "GRM" else div_b)


def test_entry_points_are_declared_exported_and_mirrored(mih):
    import ctypes as C
    import re

    from mendeliht_amd import api
    header = open(os.path.join(ROOT, "include", "mendeliht_hip.h")).read()
    declared = set(re.findall(r"^int\s+(mih_\w+)\s*\(", header, flags=re.M))
    L = C.CDLL(mih.library_path())
    for name in ("mih_grm", "mih_grm_pairs"):
        assert name in declared and name in api.exported_symbols()
        getattr(L, name)
    for cls in (mih.SnpLinAlg, mih.DosageMatrix):
        assert callable(cls.grm) and callable(cls.related_pairs)
        assert "MoM" in cls.grm.__doc__ and "subset(rows=~mask)" in cls.related_pairs.__doc__
    assert not hasattr(mih.DenseMatrix, "grm")
