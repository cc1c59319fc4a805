"""SnpLinAlg.xb / score and predict_eta (csrc/xb.hip: mih_xb_dense over the row image of csrc/transpose.hip) against
tests/xb_spec.py: every entry within the derived bound of the exact value, for every flag combination, for column counts on both
sides of the 19-residual pass, for three residual formats; a column of the result bit for bit independent of its company, of the
call and of the row image's age and flags; agreement with the sparse product; weights that stress the fixed point; the score's
semantics; the argument errors."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import xb_spec as S
from test_gpu_hardcall_pack import bed_of, edge_codes, from_bed

pytestmark = pytest.mark.gpu

FLAGS = [(c, s, i) for c in (0, 1) for s in (0, 1) for i in (0, 1)]
FORMATS = (None, 428, 1316)
T_LIST = (1, 2, 19, 20, 39)                  # one pass, a full pass, a pass boundary crossed once and twice
TALL = (33, 2 ** 18 + 33)                    # the image's passes cross a row slice
SHAPES = [(1, 1), (1, 385), (513, 1), (513, 385), (16, 32), (17, 33), (33, 127), (127, 31), (128, 128), (129, 129), (257, 385),
          (32, 129), TALL]
RATIOS = []


def finite_codes(n, p, seed):
    """edge_codes with its all-missing SNP given genotypes again (mu = NaN makes every entry NaN: test_all_missing_snp), and,
    where there is room, a sample without any genotype."""
    codes = edge_codes(n, p, seed) if (n, p) != TALL else None
    rng = np.random.default_rng(seed + 1)
    if codes is None:
        codes = rng.integers(0, 3, size=(n, p)).astype(np.int64)
        codes[rng.random((n, p)) < 0.01] = -1
    if p >= 31:
        codes[:, p - 2] = rng.integers(0, 3, size=n)
    if n >= 16 and p >= 2:
        codes[n // 3, :] = -1
    for j in np.flatnonzero((codes < 0).all(axis=0)):           # (a SNP the missing sample left without any genotype)
        codes[0, j] = 1
    return codes


def base_columns(rng, p):
    """Four columns of weights: Gaussian; one weight 10^12 x the rest; a k-sparse beta; a wide dynamic range."""
    b = rng.standard_normal((p, 4))
    b[rng.integers(p), 1] *= 1e12
    keep = rng.choice(p, size=min(p, 5), replace=False)
    sparse = np.zeros(p)
    sparse[keep] = b[keep, 2]
    b[:, 2] = sparse
    b[:, 3] *= 2.0 ** rng.integers(-30, 31, size=p)
    return b


def spread(base, t, rng):
    """t columns, column k = +-2^e base[:, k % nb]: its exact value is that multiple of the base column's (a power of two is exact)."""
    nb = base.shape[1]
    sgn, e = rng.choice([-1.0, 1.0], size=t), rng.integers(-8, 9, size=t)
    sgn[:nb], e[:nb] = 1.0, 0
    mult = sgn * 2.0 ** e
    return base[:, np.arange(t) % nb] * mult[None, :], mult


def worst_ratio(got, exact, bound):
    worst = 0.0
    for i in range(exact.shape[0]):
        for t in range(exact.shape[1]):
            assert math.isfinite(got[i, t]), (i, t, got[i, t])
            err = abs(Fraction(float(got[i, t])) - exact[i, t])
            if err:
                assert bound[i, t] > 0, (i, t, float(err))
                worst = max(worst, float(err / Fraction(float(bound[i, t]))))
    return worst


def spread_exact(ex_base, mult):
    out = np.empty((ex_base.shape[0], mult.size), dtype=object)
    for k, m in enumerate(mult):
        out[:, k] = [v * Fraction(float(m)) for v in ex_base[:, k % ex_base.shape[1]]]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_xb_within_the_bound_of_the_exact_value(mih, shape):
    n, p = shape
    tall = shape == TALL
    rng = np.random.default_rng(n * 1009 + p)
    codes = finite_codes(n, p, 5000 * n + p)
    x = from_bed(mih, codes)                                     # center, scale, impute
    mu, sinv = x.mu_sigma()
    smu, ssinv = S.mu_sigma(codes)
    assert np.array_equal(mu, smu) and np.array_equal(sinv, ssinv)
    base = base_columns(rng, p)[:, :1 if tall else 4]            # (the exact sums of a 2^18-term column take a second each)
    B, mult = spread(base, max(T_LIST), rng)
    parts = {s: S.exact_parts(codes, base, s) for s in (0, 1)}
    worst = 0.0
    # every column count, every format, the handle's own flags
    ex = spread_exact(S.exact(codes, base, 1, 1, 1, parts[1]), mult)
    cols = np.arange(mult.size) % base.shape[1]
    for dg, bound in zip(FORMATS, S.bound(codes, base, (1, 1, 1), FORMATS)):
        bound = bound[:, cols] * np.abs(mult)[None, :]           # (a power of two times the base column's: exact)
        for t in T_LIST:
            got = x.xb(B[:, :t], xtv_digits=dg)
            assert got.shape == (n, t)
            r = worst_ratio(got, ex[:, :t], bound[:, :t])
            assert r <= 1.0, (shape, dg, t, r)
            worst = max(worst, r)
    # every combination of the flags, every format
    nb = base.shape[1]
    for flags in FLAGS:
        ex = S.exact(codes, base, *flags, parts=parts[flags[1]])
        formats = FORMATS if not tall else (None,)               # (the tall image: every format above, every flag set here)
        for dg, bound in zip(formats, S.bound(codes, base, flags, formats)):
            got = x.xb(base, xtv_digits=dg, center=flags[0], scale=flags[1], impute=flags[2])
            r = worst_ratio(got, ex, bound)
            assert r <= 1.0, (shape, flags, dg, r)
            worst = max(worst, r)
        y = mih.SnpLinAlg(bed_of(codes), n, center=bool(flags[0]), scale=bool(flags[1]), impute=bool(flags[2])) if not tall else None
        if y is not None:                                        # the flags as the handle's own: the same bits as the override
            assert np.array_equal(y.xb(base).view(np.uint64), x.xb(base, center=flags[0], scale=flags[1], impute=flags[2]).view(np.uint64))
    one = x.xb(base[:, 0])
    assert one.shape == (n,) and np.array_equal(one.view(np.uint64), x.xb(base[:, :1])[:, 0].view(np.uint64))
    RATIOS.append((shape, worst))
    print(f"xb {n} x {p}: largest |error| / bound {worst:.3g} over {nb} base columns, {len(FLAGS)} flag sets, {len(FORMATS)} formats")


def test_report_largest_ratio():
    if RATIOS:
        shape, worst = max(RATIOS, key=lambda r: r[1])
        print(f"xb: largest |error| / bound over {len(RATIOS)} shapes: {worst:.3g} at {shape}")
        assert worst <= 1.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("shape", [(257, 385), (129, 33)])
def test_a_column_depends_on_nothing_but_itself(mih, shape):
    n, p = shape
    codes = finite_codes(n, p, 77 * n + p)
    x = from_bed(mih, codes)
    rng = np.random.default_rng(n + p)
    B, _ = spread(base_columns(rng, p), 39, rng)
    for dg in FORMATS:
        full = x.xb(B, xtv_digits=dg)
        for k in range(39):
            assert np.array_equal(_bits(full[:, k]), _bits(x.xb(B[:, k], xtv_digits=dg))), (dg, k)
        assert np.array_equal(_bits(full), _bits(x.xb(B, xtv_digits=dg)))                            # two calls
        assert np.array_equal(_bits(full[:, 5:25]), _bits(x.xb(B[:, 5:25], xtv_digits=dg)))          # other company, other passes
    full = x.xb(B)
    assert x.row_image(True) > 0
    assert x.row_image(False) == 0 and x._rows is None
    assert np.array_equal(_bits(full), _bits(x.xb(B)))                                               # a fresh row image
    for kw in (dict(), dict(center=False, scale=False, impute=False), dict(center=True, scale=False, impute=True)):
        assert np.array_equal(_bits(full), _bits(x.xb(B, rows=x.transpose(**kw)))), kw               # an image with other flags


def test_agrees_with_the_sparse_product(mih):
    n, p = 257, 385
    codes = finite_codes(n, p, 31)
    rng = np.random.default_rng(31)
    idx = np.sort(rng.choice(p, size=7, replace=False))
    val = rng.standard_normal(7)
    b = np.zeros(p)
    b[idx] = val
    for flags in FLAGS:
        x = mih.SnpLinAlg(bed_of(codes), n, center=bool(flags[0]), scale=bool(flags[1]), impute=bool(flags[2]))
        dense, sparse = x.xb(b), x.xv_sparse(idx, val)
        # the sparse product: a = sinv v, b = mu a, then nnz + 1 additions of terms no larger than the sums below -- nnz + 3
        # roundings relative to sum_j (code_ij + mu_j [missing, impute] + mu_j [center]) |a_j|
        mu, sinv = S.mu_sigma(codes)
        a = np.abs((sinv if flags[1] else 1.0) * b)
        mag = np.where(codes < 0, 0, codes) @ a + (flags[2] * (codes < 0)) @ (mu * a) + flags[0] * (mu * a).sum()
        tol = S.bound(codes, b, flags)[:, 0] + (7 + 3) * S.U * mag
        assert np.all(np.abs(dense - sparse) <= tol), (flags, float(np.max(np.abs(dense - sparse) / tol)))


def test_weights_that_stress_the_fixed_point(mih):
    n, p = 129, 385
    codes = finite_codes(n, p, 8)
    x = from_bed(mih, codes)
    rng = np.random.default_rng(8)
    base = base_columns(rng, p)
    assert np.array_equal(x.xb(np.zeros(p)), np.zeros(n))
    assert np.array_equal(x.xb(np.zeros((p, 3))), np.zeros((n, 3)))
    clean = x.xb(base)
    for bad in (np.nan, np.inf, -np.inf):
        B = base.copy()
        B[p // 2, 1] = bad
        got = x.xb(B)
        assert np.isnan(got[:, 1]).all()
        keep = [0, 2, 3]
        assert np.array_equal(_bits(got[:, keep]), _bits(clean[:, keep]))


def test_all_missing_snp(mih):
    """mu = NaN: every entry of X B is NaN when the call centres or imputes, and the raw product stays within its bound."""
    n, p = 33, 70
    codes = edge_codes(n, p, 12)
    assert (codes[:, p - 2] < 0).all()
    x = from_bed(mih, codes)
    b = np.random.default_rng(12).standard_normal((p, 2))
    for flags in FLAGS:
        got = x.xb(b, center=flags[0], scale=flags[1], impute=flags[2])
        ex = S.exact(codes, b, *flags)
        if flags[0] or flags[2]:
            assert ex[0, 0] is None and np.isnan(got).all(), flags
        else:
            assert worst_ratio(got, ex, S.bound(codes, b, flags)) <= 1.0


def test_score(mih):
    n, p = 129, 200
    codes = finite_codes(n, p, 21)
    rng = np.random.default_rng(21)
    w = rng.standard_normal(p)
    mask = rng.random(p) < 0.3
    idx = np.flatnonzero(mask)
    for x in (from_bed(mih, codes), mih.SnpLinAlg(bed_of(codes), n, center=False, scale=False, impute=False)):   # whatever the flags
        for weights, cols, full, scored in ((w, None, w, p), (w[idx], idx, np.where(mask, w, 0.0), idx.size), (w[idx], mask, np.where(mask, w, 0.0), idx.size)):
            ex = S.exact(codes, full, 0, 0, 1)
            bound = S.bound(codes, full, (0, 0, 1))
            got = x.score(weights, cols=cols)
            assert got.shape == (n,)
            assert worst_ratio(got[:, None], ex, bound) <= 1.0
            assert np.allclose(got, S.score(codes, weights, cols=cols), rtol=1e-12, atol=1e-12)
            avg = x.score(weights, cols=cols, average=True)
            assert np.array_equal(avg, got / (2.0 * scored))
            assert np.allclose(avg, S.score(codes, weights, cols=cols, average=True), rtol=1e-12, atol=1e-12)
    with pytest.raises(mih.api.DimensionMismatch):
        x.score(w[:-1])
    with pytest.raises(mih.api.DimensionMismatch):
        x.score(w[:3], cols=idx)


def test_predict_eta(mih, normal_data):
    n = normal_data["n"]
    x = mih.SnpLinAlg(mih.read_bed(normal_data["bed"], n), n, center=True, scale=True, impute=True)
    z = normal_data["z"]
    res = mih.fit_iht(normal_data["y"], x, z, k=7, verbose=False)
    eta = res.predict_eta(x, z)
    assert np.array_equal(eta, x.xb(res.beta) + z @ res.c)
    idx = np.flatnonzero(res.beta)
    assert np.allclose(eta, x.xv_sparse(idx, res.beta[idx]) + z @ res.c, rtol=1e-10, atol=1e-10)
    Y = np.stack([normal_data["y"], normal_data["y"] ** 2])
    mv = mih.fit_iht(Y, x, z.T, k=5, verbose=False)
    assert np.array_equal(mv.predict_eta(x, z.T), x.xb(mv.beta.T).T + mv.c @ z.T)


def test_argument_errors(mih):
    codes = finite_codes(33, 70, 2)
    x = from_bed(mih, codes)
    for bad in (np.zeros(69), np.zeros((71, 2)), np.zeros((70, 2, 2)), np.zeros((2, 70)), np.zeros((70, 0))):
        with pytest.raises(mih.api.DimensionMismatch):
            x.xb(bad)
    with pytest.raises(mih.api.ArgumentError):
        x.xb(np.zeros(70), xtv_digits=777)
    other = from_bed(mih, finite_codes(33, 71, 3)).transpose()
    out, b = np.empty(33), np.zeros(70)
    rc = mih.lib().mih_xb_dense(x._h, other._h, b.ctypes.data_as(C.c_void_p), 1, -1, -1, -1, 0, out.ctypes.data_as(C.c_void_p))
    assert rc == 2                                                                                   # MIH_BAD_ARG
    msg = C.create_string_buffer(512)
    mih.lib().mih_last_error(msg, 512)
    assert b"71 x 33" in msg.value and b"33 x 70" in msg.value, msg.value
    with pytest.raises(mih.api.ArgumentError, match="71 x 33"):
        x.xb(b, rows=other)
    with pytest.raises(mih.api.ArgumentError):                                                       # the matrix itself is no row image of itself
        x.xb(b, rows=x)
    d = mih.DosageMatrix(np.where(codes < 0, 0xFFFF, codes).astype(np.uint16), 1)
    with pytest.raises(mih.api.ArgumentError, match="2-bit"):
        d.xb(b)
    with pytest.raises(mih.api.ArgumentError, match="2-bit"):
        mih.DenseMatrix(np.zeros((5, 70))).xb(b)
    rc = mih.lib().mih_xb_dense(d._h, x.transpose()._h, b.ctypes.data_as(C.c_void_p), 1, -1, -1, -1, 0, out.ctypes.data_as(C.c_void_p))
    assert rc == 2
