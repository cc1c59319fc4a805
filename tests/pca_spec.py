"""The numpy statement of pca() (csrc/pca.hip: mih_grm_eig) -- the k leading eigenpairs of the kinship matrix Phi of
tests/grm_spec.py -- and of the blocked subspace iteration the device runs.  It is the yardstick of the device path.

top(phi, k): numpy.linalg.eigh, the k largest eigenvalues in descending order, unit eigenvectors with the sign rule: the
entry of largest magnitude (lowest index on a tie) is positive.

iterate(phi, k, ...): the device's algorithm, step for step:
    b = block or round_up(max(2 k, k + 8), 16), b_l = min(b, n)
    Q = start(seed, n, b_l), entries a counter-based hash of (seed, row, column) in (-1, 1); Q <- orth(orth(Q))
    repeat: Y = Phi Q; T = sym(Q' Y) = S Theta S'; rho_i = |Y s_i - theta_i Q s_i| for the k leading Ritz pairs;
            stop when max rho <= tol theta_1 or at max_iter; else Q <- orth(orth(Y))
    orth(Y): G = Y' Y = W D W' with D descending; the directions with d_i <= 2^-52 d_1 are dropped for the rest of the run;
             Q = Y W D^(-1/2).  A pass through the Gram matrix loses orthogonality in proportion to u cond(Y)^2; the second
             pass starts from a block whose condition number is near 1 and repairs it ("twice is enough").
The device's sums run in another order, so the two agree within the bounds below and not bit for bit.

planted(n, p, k): k + 1 populations of sizes proportional to 1, 2, 3, ..., Balding-Nichols allele frequencies with
F_ST = 0.25 around ancestral frequencies U(0.1, 0.9), 5 % missing genotypes, and where p >= 31 a monomorphic-0, a
monomorphic-2 and an all-missing column (columns 3, 17 and p - 2, as edge_codes has them); seed 1000 n + p.

Bounds (u = 2^-53; E = grm_spec.bound, the entrywise distance between the device's Phi and the spec's; rho_i the residual
of the returned pair against the spec's Phi, evaluated in numpy; gap_i the distance from the spec's i-th eigenvalue to the
nearest other one):
    residual_bound:  rho_i <= tol lambda_1 + |E|_F + 8 (n + b) u |Phi|_F -- the contract, the distance of the two matrices,
                     and the rounding of the two residual evaluations and of the final rotation
    value_bound:     |lambda_i - lambda^s_i| <= rho_i + 8 n u lambda^s_1 -- a Ritz value of a symmetric matrix lies within
                     its residual of an eigenvalue, and eigh's own error
    vector_bound:    |u_i - v^s_i|_2 <= (2 rho_i + 16 n u lambda^s_1) / gap_i -- Davis-Kahan for the device's vector plus
                     eigh's own error over the same gap
    orth_bound:      |U' U - I| <= 8 (n + b) u, elementwise"""
import numpy as np

U = 2.0 ** -53
SHAPES = [(16, 4, 1), (17, 33, 2), (63, 70, 3), (65, 150, 3), (128, 5, 2), (129, 150, 3), (257, 150, 4), (257, 600, 4),
          (300, 1000, 5)]
MASK = (1 << 64) - 1


def sign_rule(v):
    """Columns of v (or a vector) with the entry of largest magnitude, lowest index on a tie, made positive."""
    v = np.array(v, dtype=np.float64)
    cols = v.reshape(v.shape[0], -1)
    for c in range(cols.shape[1]):
        if cols[np.argmax(np.abs(cols[:, c])), c] < 0.0:           # argmax returns the first of equals
            cols[:, c] = -cols[:, c]
    return cols.reshape(v.shape)


def top(phi, k):
    """(values (k,), vectors (n, k)) of the k largest eigenvalues, descending, with the sign rule."""
    w, v = np.linalg.eigh(phi)
    order = np.argsort(-w, kind="stable")[:k]
    return w[order], sign_rule(v[:, order])


def block_size(k, n, block=0):
    b = block if block else -(-max(2 * k, k + 8) // 16) * 16
    return b, min(b, n)


def start(seed, n, bl):
    """Q[i, c] = ((z >> 12) + 1/2) 2^-51 - 1 with z = splitmix64's output function of seed + 0x9E3779B97F4A7C15 (128 i + c + 1),
    all modulo 2^64: in (-1, 1), never 0."""
    i, c = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(bl, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(128) * i + c + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -51 - 1.0


def rank_rule(d):
    """How many of the descending d survive: d_i > 2^-52 d_1, none if d_1 is not positive."""
    d = np.asarray(d, dtype=np.float64)
    if d.size == 0 or not d[0] > 0.0:
        return 0
    return int(np.count_nonzero(d > 2.0 ** -52 * d[0]))


def eig_desc(a):
    w, v = np.linalg.eigh((a + a.T) / 2.0)
    order = np.argsort(-w, kind="stable")
    return w[order], v[:, order]


def orth(y):
    d, w = eig_desc(y.T @ y)
    r = rank_rule(d)
    return (y @ w[:, :r]) / np.sqrt(d[:r])[None, :]


class RankError(ValueError):
    pass


def iterate(phi, k, tol=1e-10, max_iter=500, block=0, seed=0):
    """(values, vectors, residuals, iters, converged) of the blocked subspace iteration on phi."""
    n = phi.shape[0]
    b, bl = block_size(k, n, block)
    q = orth(orth(start(seed, n, bl)))
    it = 0
    while True:
        if q.shape[1] < k:
            raise RankError(f"numerical rank {q.shape[1]} is below k = {k}")
        y = phi @ q
        theta, s = eig_desc(q.T @ y)
        theta, s = theta[:k], s[:, :k]
        res = np.linalg.norm(y @ s - (q @ s) * theta[None, :], axis=0)
        it += 1
        done = bool(res.max() <= tol * theta[0])
        if done or it >= max_iter:
            break
        q = orth(orth(y))
    u = sign_rule(q @ s)
    return theta, u / np.linalg.norm(u, axis=0)[None, :], res, it, done


def planted(n, p, k, seed=None):
    """n x p allele counts, -1 for a missing one, with k + 1 populations."""
    rng = np.random.default_rng(1000 * n + p if seed is None else seed)
    pops = k + 1
    share = np.arange(1, pops + 1, dtype=np.float64)
    edges = np.floor(np.cumsum(share) / share.sum() * n + 0.5).astype(int)
    label = np.searchsorted(edges, np.arange(n), side="right").clip(0, pops - 1)
    anc = rng.uniform(0.1, 0.9, p)
    fst = 0.25
    f = rng.beta(anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst, size=(pops, p))
    codes = rng.binomial(2, f[label]).astype(np.int64)
    codes[rng.random((n, p)) < 0.05] = -1
    if p >= 31:
        codes[:, 3], codes[:, 17], codes[:, p - 2] = 0, 2, -1
    return codes


def relative_gap(lam, k):
    """min |lambda_i - lambda_j| / lambda_1 over the leading k + 1 eigenvalues (all of them if there are fewer)."""
    lead = np.sort(np.asarray(lam))[::-1][:k + 1]
    if lead.size < 2:
        return np.inf
    return float(np.min(-np.diff(lead)) / lead[0])


def gaps(lam_all, k):
    """gap_i, i < k: the distance from the i-th largest eigenvalue to the nearest other eigenvalue."""
    lam = np.sort(np.asarray(lam_all))[::-1]
    out = np.empty(k)
    for i in range(k):
        out[i] = np.min(np.abs(np.delete(lam, i) - lam[i])) if lam.size > 1 else np.inf
    return out


def residuals(phi, values, vectors):
    return np.linalg.norm(phi @ vectors - vectors * values[None, :], axis=0)


def residual_bound(phi, lam1, tol, n, b, e_fro=0.0):
    return tol * lam1 + e_fro + 8.0 * (n + b) * U * np.linalg.norm(phi)


def value_bound(rho, lam1, n):
    return rho + 8.0 * n * U * lam1


def vector_bound(rho, lam1, n, gap):
    return (2.0 * rho + 16.0 * n * U * lam1) / gap


def orth_bound(n, b):
    return 8.0 * (n + b) * U
