"""The numpy statement of initialize_beta!'s p univariate regressions y ~ 1 + x_j (utilities.jl:776-842; on the device
init_beta_regress_device of csrc/iht_var.hip, reached on its own through mih_probe_init_beta).  It is the yardstick of
tests/test_gpu_init_beta.py; tests/test_init_beta_spec_cpu.py checks it against np.linalg.lstsq and fixes the cases.

Training rows T = {i : w_i != 0}, N = |T|.  x_ij is the entry of the matrix as mih_xtv multiplies it (assoc_spec.class_values /
xtilde: the handle's own mu_j, sinv_j and its (center, scale, impute)).  Per column j and trait t
    Sx = sum_T x,  Sxy = sum_T x y_t,  Sxx = sum_T x^2,  Sy = sum_T y_t
    u11 = sqrt N,  u12 = Sx / u11,  d = Sxx - u12^2
    N > 0 and d > 0:  b1 = (Sxy - u12 Sy / u11) / d,  b0 = (Sy / u11 - u12 b1) / u11;      otherwise (b0, b1) = (Sy, Sxy), unsolved
    beta = clamp(b1, -2, 2),  icpt = b0,  icpt_sum_t = sum_j b0_jt.

Three evaluations:

exact_snp / exact_dense: everything in rationals.  For a 2-bit matrix the four values of a column are the rationals
    v(g) = (g - [center] mu_j) * ([scale] sinv_j, else 1),   g = 0, 1, 2 and, for a missing entry, [impute] mu_j (else 0)
over the doubles mu_j and sinv_j (the reference of gpu_helpers.xtv_std_exact, which the X'r bound below belongs to; the floats of
assoc_spec.class_values are these values rounded twice).  The traits are multiples of 2^-20 below 2^10 in size, so the per-class
counts and the per-class sums of 2^20 y over T are integers below 2^45, exact in a float64 matrix product; Sx, Sxy and Sxx are
four class terms each and no row is ever touched in rational arithmetic.  b1 = (Sxy - Sx Sy / N) / (Sxx - Sx^2 / N) and
b0 = (Sy - Sx b1) / N are rational too.  For a dense or dosage matrix the entries are doubles, taken as integers over one power
of two.

solve_mp: the six operations in mpmath (50 digits) from GIVEN Sx, Sxy, Sxx, N, Sy -- the reference of the device's k_ib_solve
fed with the device's own X'R values.

solve_bound: what k_ib_solve may differ from solve_mp by, first-order propagation of its roundings counted from the source
(u = 2^-53; contraction into FMAs only removes roundings; * marks solve_mp's values; Sx, Sxy, Sy, N and the counts enter exact):
    sxx     2-bit: s * s * (c0 cm cm + c1 (1 - cm)(1 - cm) + c2 (2 - cm)(2 - cm) + nm xm xm): a term carries the rounding of its
            difference twice and two products (4), the three additions 3, s * s and the last product 2: e_xx = 9 u relative,
            every term being non-negative.  Dense and dosage: the device's own sxx is fed to solve_mp, e_xx = 0.
    u11     = fl(sqrt N): 1.        u12 = fl(sx / u11): 2 in all.        u12 * u12: 5 relative to Sx^2 / N <= Sxx.
    d       = fl(sxx - u12^2): |dd| <= (e_xx + 5 u) Sxx + u d*, that is  rd = dd / d* <= (e_xx + 5 u) Sxx / d* + u.
    w1      = fl(Sy / u11): 2.      u12 * w1: 5 relative to Sx Sy / N.
    num     = fl(sxy - u12 w1): |dnum| <= 5 u |Sx Sy| / N + u |num*|.
    u22     = fl(sqrt d): rd / 2 + u.    w2 = fl(num / u22), b1 = fl(w2 / u22): u22 twice and two divisions,
            |db1| <= |dnum| / d* + |b1*| (rd + 4 u) = 5 u |Sx Sy| / (N d*) + |b1*| (rd + 5 u).
    b0      = fl((w1 - u12 b1) / u11): the product u12 b1 carries |Sx| |db1| / sqrt N and 3 u of itself, w1 2 u, the difference 1,
            u11 and the division 2:
            |db0| <= (2 u |Sy| + |Sx| |db1| + 3 u |Sx b1*|) / N + 3 u |b0*|.
The neglected second-order terms are at most (rd + 5 u) times these; the cases keep d* / Sxx >= 0.1, so rd < 2e-14 and a factor
1 + 1e-6 covers them and the conversion of the bound to float64.  Nothing is measured.  The clamp adds nothing: min and max are exact, and
the cases keep |b1| 1e-6 away from 2.

The cases (snp_cases, dense_cases, inputs) sit at the edges of the kernels (tests/test_gpu_init_beta.py says why each is there);
conditions() states in exact arithmetic what the device test relies on."""
import functools
from fractions import Fraction

import numpy as np

import assoc_spec as A

U = 2.0 ** -53
YQ = 2 ** 20                       # the traits are multiples of 1 / YQ
E_XX_SNP = 9 * U
SECOND_ORDER = 1.0 + 1e-6
MIN_D_OVER_SXX = Fraction(1, 10)
COUNT_BLOCK_ROWS = 64 * 128        # kIbBpPerBlock tiles of 128 rows: what one block of k_ib_counts walks


# ---- the solve -----------------------------------------------------------------------------------------------------------------
def solve_exact(N, Sx, Sxy, Sxx, Sy):
    """(b0, b1, d) in rationals; the failure branch returns the unsolved right-hand side (Sy, Sxy)."""
    if not N > 0:
        return Sy, Sxy, None
    d = Sxx - Sx * Sx / N
    if not d > 0:
        return Sy, Sxy, d
    b1 = (Sxy - Sx * Sy / N) / d
    return (Sy - Sx * b1) / N, b1, d


def _mpf(v):
    import mpmath as mp
    return mp.mpf(v.numerator) / v.denominator if isinstance(v, Fraction) else mp.mpf(float(v))


def solve_mp(N, sx, sxy, sxx, Sy):
    """(b0, b1, d) as mpmath numbers at 50 digits, operation by operation as the statement has them."""
    import mpmath as mp
    with mp.workdps(50):
        N, sx, sxy, sxx, Sy = _mpf(N), _mpf(sx), _mpf(sxy), _mpf(sxx), _mpf(Sy)
        if not N > 0:
            return Sy, sxy, None
        u11 = mp.sqrt(N)
        u12 = sx / u11
        d = sxx - u12 * u12
        if not d > 0:
            return Sy, sxy, d
        b1 = (sxy - u12 * Sy / u11) / d
        return (Sy / u11 - u12 * b1) / u11, b1, d


def solve_bound(N, sx, sxy, sxx, Sy, b0, b1, d, e_xx):
    """(db0, db1) of the module docstring, floats, from solve_mp's own values."""
    N, sx, sxy, sxx, Sy, b0, b1, d = (abs(float(v)) for v in (N, sx, sxy, sxx, Sy, b0, b1, d))
    rd = (e_xx + 5 * U) * sxx / d + U
    db1 = 5 * U * sx * Sy / (N * d) + b1 * (rd + 5 * U)
    db0 = (2 * U * Sy + sx * db1 + 3 * U * sx * b1) / N + 3 * U * b0
    return db0 * SECOND_ORDER, db1 * SECOND_ORDER


def err(x, ref):
    """|x - ref| of a double against an mpmath reference, as a float."""
    import mpmath as mp
    with mp.workdps(50):
        return float(abs(mp.mpf(float(x)) - ref))


def clamp(b1):
    return -2.0 if b1 < -2 else (2.0 if b1 > 2 else float(b1))


# ---- exact sums ------------------------------------------------------------------------------------------------------------------
def y_ints(Y):
    """2^20 Y as exact integers in float64 (asserted), n x m."""
    Yi = np.asarray(Y, dtype=np.float64).reshape(Y.shape[0], -1) * YQ
    assert np.array_equal(Yi, np.rint(Yi)) and np.abs(Yi).max() < YQ * 2 ** 10
    return Yi


def class_values_exact(mu, sinv, flags):
    """p lists of the four rationals v(0), v(1), v(2), v(missing)."""
    center, scale, impute = flags
    out = []
    for m, s in zip(mu, sinv):
        m = Fraction(float(m))
        s = Fraction(float(s)) if scale else Fraction(1)
        cm = m if center else Fraction(0)
        out.append([(g - cm) * s for g in (Fraction(0), Fraction(1), Fraction(2), m if impute else Fraction(0))])
    return out


def train_counts(codes, w):
    """(4, p) int64: the training rows of every column with dosage 0, 1, 2 and missing."""
    t = np.asarray(w) != 0
    return np.stack([(codes[t] == g).sum(axis=0) for g in (0, 1, 2, -1)]).astype(np.int64)


class Exact:
    """N, Sy[t], Sx[j], Sxx[j], Sxy[t][j], d[j] (None for N = 0), b0[t][j], b1[t][j]: Fractions.  cnt: (4, p) for a 2-bit matrix."""
    def __init__(self, N, Sy, Sx, Sxx, Sxy, cnt=None):
        self.N, self.Sy, self.Sx, self.Sxx, self.Sxy, self.cnt = N, Sy, Sx, Sxx, Sxy, cnt
        self.p, self.m = len(Sx), len(Sy)
        sol = [[solve_exact(N, Sx[j], Sxy[t][j], Sxx[j], Sy[t]) for j in range(self.p)] for t in range(self.m)]
        self.b0 = [[s[0] for s in row] for row in sol]
        self.b1 = [[s[1] for s in row] for row in sol]
        self.d = [s[2] for s in sol[0]]


def exact_snp(codes, stats, flags, w, Y):
    """The regressions of a 2-bit matrix in rationals, from the class counts and class sums of y over the training rows."""
    n, p = codes.shape
    Yi = y_ints(Y)
    t = (np.asarray(w) != 0).astype(np.float64)
    R = np.concatenate([t[:, None], t[:, None] * Yi], axis=1)                       # n x (1 + m): integers
    cls = [R.T @ (codes == g).astype(np.float64) for g in (0, 1, 2, -1)]            # 4 of (1 + m) x p, exact below 2^53
    assert all(np.abs(c).max(initial=0.0) < 2.0 ** 52 for c in cls)
    V = class_values_exact(*stats, flags)
    N = int(t.sum())
    m = Yi.shape[1]
    Sy = [Fraction(int(v), YQ) for v in (t @ Yi)]
    Sx = [sum(V[j][k] * int(cls[k][0, j]) for k in range(4)) for j in range(p)]
    Sxx = [sum(V[j][k] * V[j][k] * int(cls[k][0, j]) for k in range(4)) for j in range(p)]
    Sxy = [[sum(V[j][k] * int(cls[k][1 + tt, j]) for k in range(4)) / YQ for j in range(p)] for tt in range(m)]
    return Exact(N, Sy, Sx, Sxx, Sxy, np.stack([c[0] for c in cls]).astype(np.int64))


def exact_dense(X, w, Y):
    """The same for a matrix of doubles X (n x p): every entry an integer over one power of two."""
    n, p = X.shape
    Yi = y_ints(Y)
    rows = np.flatnonzero(np.asarray(w) != 0)
    Yo = np.array([[int(v) for v in r] for r in Yi[rows]], dtype=object).reshape(rows.size, -1)
    N, m = int(rows.size), Yi.shape[1]
    Sy = [Fraction(int(sum(Yo[:, tt])), YQ) for tt in range(m)]
    Sx, Sxx, Sxy = [], [], [[] for _ in range(m)]
    for j in range(p):
        ratios = [float(v).as_integer_ratio() for v in X[rows, j]]
        D = max([q for _, q in ratios], default=1)
        a = np.array([num * (D // q) for num, q in ratios], dtype=object)
        Sx.append(Fraction(int(a.sum()), D))
        Sxx.append(Fraction(int((a * a).sum()), D * D))
        for tt in range(m):
            Sxy[tt].append(Fraction(int((a * Yo[:, tt]).sum()), D * YQ))
    return Exact(N, Sy, Sx, Sxx, Sxy)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
SNP_N = (17, 128, 129, 8192, 8193, 8320, 16500)        # a dword and a row; a tile; + a row; one count block; + a row; + a tile; three, ragged
SNP_P = (1, 32, 33, 65)                                # one ragged group; one full; + one column; two and a ragged third
SNP_SHAPES = tuple([(n, 33) for n in SNP_N] + [(n, p) for n in (129, 8320) for p in (1, 32, 65)] + [(17, 1), (17, 65), (16500, 1), (16500, 65)])
SNP_MASKS = ("all", "random80", "one_out", "blocks")
SNP_MISSING = (0.0, 0.03)
TRAIT_SHAPES = ((129, 33), (8320, 65))
TRAIT_M = (2, 17, 32)                                  # 3, 18 and 33 right-hand sides: 33 take more than one fused pass
DENSE_KINDS = ("f64", "f32", "dosage")
DENSE_N = (255, 256, 257, 1000)                        # the 256-row stride of k_ib_dense_sxx
DENSE_P = 5
DOSAGE_DEN = 1000
PLANT_MIN_P = 32


class Case:
    def __init__(self, kind, n, p, m, mask, flags=None, missing=0.0, seed=0):
        self.kind, self.n, self.p, self.m, self.mask, self.flags, self.missing, self.seed = kind, n, p, m, mask, flags, missing, seed

    @property
    def id(self):
        f = "" if self.flags is None else "-f{}{}{}-miss{}".format(*self.flags, int(round(100 * self.missing)))
        return f"{self.kind}-n{self.n}-p{self.p}-m{self.m}-{self.mask}{f}"

    @property
    def one_training_row(self):
        """n = 8193 under the `blocks` mask: the 8192 rows of the first count block are held out and one row is left.  Every column
        is then constant over T like a planted (c) column (d = 0 exactly, the branch undetermined), N >= 8 cannot hold, and the case is
        there for the counts, the X'R pass and the bits: its slopes only have to be finite and clamped."""
        return self.mask == "blocks" and self.n == COUNT_BLOCK_ROWS + 1


@functools.lru_cache(maxsize=None)
def snp_cases():
    """Every shape under every mask that fits it (blocks: n > 8192), m = 1; the flags and the missing share cycle so that every mask
    meets every flag set and both shares.  Then m = 2, 17, 32 at TRAIT_SHAPES under random80 (and blocks where it fits)."""
    out, t = [], 0
    for n, p in SNP_SHAPES:
        for mask in SNP_MASKS:
            if mask == "blocks" and n <= COUNT_BLOCK_ROWS:
                continue
            out.append(Case("snp", n, p, 1, mask, A.EDGE_FLAGS[t % 4], SNP_MISSING[(t // 4 + t) % 2], 7000 + t))
            t += 1
    for n, p in TRAIT_SHAPES:
        for m in TRAIT_M:
            for mask in ("random80", "blocks") if n > COUNT_BLOCK_ROWS else ("random80",):
                out.append(Case("snp", n, p, m, mask, A.EDGE_FLAGS[t % 4], SNP_MISSING[(t // 4 + t) % 2], 7000 + t))
                t += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dense_cases():
    out, t = [], 0
    for kind in DENSE_KINDS:
        for n in DENSE_N:
            for m in (1, 3):
                for mask in ("all", "random80"):
                    out.append(Case(kind, n, DENSE_P, m, mask, seed=8000 + t))
                    t += 1
    return tuple(out)


def train_mask(case, rng):
    n = case.n
    w = np.ones(n)
    if case.mask == "random80":
        w[rng.random(n) >= 0.8] = 0.0
    elif case.mask == "one_out":
        w[n - 1] = 0.0
    elif case.mask == "blocks":
        w[:COUNT_BLOCK_ROWS] = 0.0                                   # the first count block contributes nothing
        for word in range(1, 8, 2):                                  # the following tile: every other 16-row word
            w[COUNT_BLOCK_ROWS + 16 * word:COUNT_BLOCK_ROWS + 16 * word + 16] = 0.0
        w[COUNT_BLOCK_ROWS + 6 * 128:COUNT_BLOCK_ROWS + 7 * 128] = 0.0        # and a whole tile further on (where n reaches it)
    else:
        assert case.mask == "all"
    return w


def _traits(rng, n, m):
    """n x m multiples of 2^-20: Gaussian noise of scale 1/4 (trait 0) or exp(U(-1, 1)) around an offset."""
    scale = np.concatenate([[0.25], np.exp(rng.uniform(-1, 1, m - 1))])
    Y = rng.standard_normal((n, m)) * scale[None, :] + rng.uniform(-2, 2, m)[None, :]
    return np.rint(Y * YQ) / YQ


class Inputs:
    """What a case feeds the probe: codes (n x p allele counts, -1 missing) or X (n x p doubles, the entries mih_xtv multiplies; for
    f32 exactly representable; for dosage with num, den beside it), w, Y (n x m), planted = {name: column}."""
    pass


def _draw_snp(case, attempt):
    n, p, m = case.n, case.p, case.m
    rng = np.random.default_rng([case.seed, attempt])
    w = train_mask(case, rng)
    T, H = np.flatnonzero(w != 0), np.flatnonzero(w == 0)
    lo = 0.3 if n == 17 else 0.05
    codes = rng.binomial(2, rng.uniform(lo, 0.5, p)[None, :], size=(n, p)).astype(np.int64)
    if case.missing > 0:
        codes[rng.random((n, p)) < case.missing] = -1
    planted = {}
    if p >= PLANT_MIN_P:
        planted["a"] = 3
        codes[:, 3] = 0                                              # (a) all zero: every sum is exactly 0
        planted["jstar"] = p - 2
        jb = p - 1                                                   # (b) missing rows all in T (the last column of a ragged group)
        planted["b_in"] = jb
        col = codes[:, jb]
        col[col < 0] = rng.integers(0, 3, int((col < 0).sum()))
        col[rng.choice(T, min(3, max(T.size - 8, 1)), replace=False)] = -1
        if H.size:
            planted["b_out"] = 5                                     # (b) missing rows all held out
            col = codes[:, 5]
            col[col < 0] = rng.integers(0, 3, int((col < 0).sum()))
            col[rng.choice(H, min(3, H.size), replace=False)] = -1
            planted["c"] = 17                                        # (c) non-zero genotypes in held-out rows only
            codes[:, 17] = 0
            codes[H, 17] = rng.integers(1, 3, H.size)
    Y = _traits(rng, n, m)
    if "jstar" in planted:                                           # (d) b1 ~ 3 in trait 0: the clamp returns exactly 2
        x = A.xtilde(codes[:, planted["jstar"]:planted["jstar"] + 1], case.flags)[:, 0]
        Y[:, 0] = np.rint((Y[:, 0] + 3.0 * x) * YQ) / YQ
    inp = Inputs()
    inp.case, inp.codes, inp.w, inp.Y, inp.planted, inp.attempt = case, codes, w, Y, planted, attempt
    return inp


def _draw_dense(case, attempt):
    n, p, m = case.n, case.p, case.m
    rng = np.random.default_rng([case.seed, attempt])
    w = train_mask(case, rng)
    inp = Inputs()
    if case.kind == "dosage":
        import gpu_helpers as H
        num = rng.integers(0, 2 * DOSAGE_DEN + 1, (n, p)) * rng.uniform(0.1, 1.0, p)[None, :]
        num = np.rint(num).astype(np.int64)
        num[rng.random((n, p)) < 0.03] = 0xFFFF
        inp.num, inp.den = num.astype(np.uint16), DOSAGE_DEN
        _, _, mu, sinv = H.dosage_host_stats(inp.num, inp.den)
        inp.X = H.standardized(inp.num, inp.den, mu, sinv)
    else:
        X = rng.standard_normal((n, p)) * np.exp(rng.uniform(-2, 2, p))[None, :] + rng.uniform(-0.5, 0.5, p)[None, :]
        inp.X = np.asfortranarray(X.astype(np.float32).astype(np.float64) if case.kind == "f32" else X)
    inp.case, inp.w, inp.Y, inp.planted, inp.attempt = case, w, _traits(rng, n, m), {}, attempt
    return inp


def exact_of(inp, stats=None, X=None):
    """The exact evaluation of a case's inputs; stats / X: the handle's own (mu, sinv) or standardized dosage entries where the
    caller has them (they are what host_stats / dosage_host_stats give: the device forms them by the same correctly rounded steps)."""
    if inp.case.kind == "snp":
        return exact_snp(inp.codes, A.host_stats(inp.codes) if stats is None else stats, inp.case.flags, inp.w, inp.Y)
    return exact_dense(inp.X if X is None else X, inp.w, inp.Y)


def undetermined(inp):
    """The columns the device test leaves out of the beta / intercept comparison, by index: planted (c) (every column where one
    training row is all there is)."""
    if inp.case.one_training_row:
        return list(range(inp.case.p))
    return [inp.planted["c"]] if "c" in inp.planted else []


def conditions(inp, ex=None):
    """The list of what does NOT hold of the conditions the device test relies on, in exact arithmetic (empty: all hold)."""
    ex = exact_of(inp) if ex is None else ex
    case, bad = inp.case, []
    zero_d = {inp.planted[k] for k in ("a", "c") if k in inp.planted}
    if case.one_training_row:
        if ex.N != 1 or any(d != 0 for d in ex.d):
            bad.append(("one training row", ex.N))
        return bad
    if ex.N < 8:
        bad.append(("N", ex.N))
    for j in range(case.p):
        if j in zero_d:
            if ex.d[j] != 0:
                bad.append(("planted d", j, float(ex.d[j])))
            continue
        if not (ex.Sxx[j] > 0 and ex.d[j] >= MIN_D_OVER_SXX * ex.Sxx[j]):
            bad.append(("d / Sxx", j, float(ex.d[j] / ex.Sxx[j]) if ex.Sxx[j] > 0 else None))
            continue
        for t in range(case.m):
            if abs(abs(ex.b1[t][j]) - 2) <= Fraction(1, 10 ** 6):
                bad.append(("b1 near 2", j, t, float(ex.b1[t][j])))
    if "jstar" in inp.planted and not abs(ex.b1[0][inp.planted["jstar"]]) >= Fraction(5, 2):
        bad.append(("jstar", float(ex.b1[0][inp.planted["jstar"]])))
    if case.kind == "snp":
        T, codes = inp.w != 0, inp.codes
        if "b_out" in inp.planted and not ((codes[:, inp.planted["b_out"]] < 0).sum() > 0 and (codes[T, inp.planted["b_out"]] < 0).sum() == 0):
            bad.append(("b_out",))
        if "b_in" in inp.planted and not ((codes[T, inp.planted["b_in"]] < 0).sum() > 0 and (codes[~T, inp.planted["b_in"]] < 0).sum() == 0):
            bad.append(("b_in",))
        if "c" in inp.planted and not ((codes[T, inp.planted["c"]] == 0).all() and (codes[~T, inp.planted["c"]] > 0).all()):
            bad.append(("c",))
        if (codes >= 0).sum(axis=0).min() == 0:
            bad.append(("all-missing column",))
    return bad


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The inputs of a case: the first draw (attempt 0, 1, ...) of its seed for which conditions() holds, with its exact evaluation
    in .exact.  Deterministic; tests/test_init_beta_spec_cpu.py asserts the conditions again for every case."""
    for attempt in range(40):
        inp = (_draw_snp if case.kind == "snp" else _draw_dense)(case, attempt)
        ex = exact_of(inp)
        if not conditions(inp, ex):
            inp.exact = ex
            return inp
    raise AssertionError(("no draw meets the conditions", case.id))


def sxx_gamma(n):
    """k_ib_dense_sxx / k_ib_dosage_sxx: a thread walks ceil(n / 256) rows (that many FMAs; the square and the weight 0 / 1 are
    two more roundings of a term), block_sum is an eight-level tree."""
    return (-(-n // 256) + 8 + 2) * U


def icpt_sum_gamma(p):
    """k_ib_sum over 64 blocks of 256 threads (a thread's grid-stride walk: ceil(p / 16384) terms, eight tree levels) and k_final_sum
    over the 64 partials (a 256-thread tree: eight levels)."""
    return (-(-p // 16384) + 16) * U


def fsum_exact(v):
    return sum((Fraction(float(x)) for x in v), Fraction(0))
