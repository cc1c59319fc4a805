"""The numpy statement of kinship_solve() (csrc/lmm.hip: mih_grm_solve) -- X = V^-1 B with V = tau_e I + tau_g Phi, Phi the
kinship matrix of tests/grm_spec.py -- and of the conjugate gradient the device runs.  It is the yardstick of the device path.

pcg(phi, B, tau_e, tau_g, tol, max_iter): the device's algorithm, step for step, every column by itself:
    d = diag V;  x = 0, r = b, z = r / d, p = z, rz = r'z;  the column is frozen at once if |r| <= tol |b| (a zero column)
    repeat  Vp = V p;  alpha = rz / p'Vp;  x += alpha p;  r -= alpha Vp;  z = r / d;  one iteration counted;
            frozen (converged) when |r|_2 <= tol |b|_2, evaluated as sqrt(r'r) <= tol sqrt(b'b);
            else beta = r'z / rz, rz = r'z, p = z + beta p
    until frozen or max_iter iterations;  0 / 0 in alpha and beta is 0
    the true residual |b - V x|_2 is formed explicitly at the end.
The device's sums run in another order, so the two agree within the bounds below and not bit for bit.

dense(phi, B, tau_e, tau_g): the reference, a Cholesky solve.

Bounds (u = 2^-53; E = grm_spec.bound, the entrywise distance between the device's Phi and the spec's; V_s the spec's V):
    residual_bound:  |b - V_s x|_2 <= reported true residual + (tau_g |E|_F + 8 (n + m) u |V_s|_F) |x|_2 -- the distance of the
                     two matrices and the rounding of the two residual evaluations
    gap_bound:       a converged column reports a true residual <= tol |b|_2 + gap_bound + eval_bound.  The recurrence residual
                     r_k and the true residual b - V x_k drift apart by the roundings of the two recurrences (Greenbaum 1997,
                     "Estimating the attainable accuracy of recursively computed residual methods"): with x_k = x_{k-1} +
                     alpha p + xi_k, |xi_k| <= u |x_k| (one fused multiply-add), and r_k = r_{k-1} - alpha fl(V p) + eta_k,
                     |eta_k| <= u |r_k| + |alpha| (n + 2) u |V| |p| (an n-term sum in any order, the product tau_e p and
                     the fused multiply-add of the epilogue), the gap g_k = b - V x_k - r_k obeys g_0 = 0 and
                     g_k = g_{k-1} - V xi_k - eta_k.  With Theta = max_j |x_j|_2, |alpha p_j| <= 2 Theta,
                     |r_j| <= |b| + |V| Theta and | |V| |_2 <= |V|_F this gives, to first order in u,
                         |g_k|_2 <= k u ((2 n + 6) |V|_F Theta + |b|_2)
                     -- Greenbaum's u * iterations * |V| * max |x_k| with the constant 2 n + 6.  Theta is taken as the largest
                     iterate of this file's pcg on the same input (the device's iterates differ from them by rounding) or the
                     returned solution, whichever is larger.  Measured beside it (test_lmm_spec_cpu.py prints them): the gap of
                     this file's own pcg at n = 513, m = 128 after 60 iterations at tol = 0 is at most 3.5e-15 |b| where the
                     bound allows 5.3e-10 |b|: the constant is a worst case over n-term sums, five orders above what is seen.
    eval_bound:      (n + 4) u (|V|_F |x|_2 + |b|_2), the rounding of the device's own evaluation of |b - V x|_2"""
import numpy as np

U = 2.0 ** -53
SOLVE_N = (1, 17, 127, 129, 257, 513)          # the matrix-core block, the tile, three tiles, the slab of the Gram partials
SOLVE_M = (1, 16, 17, 33, 65, 128)             # where <IB, NB> switches, and the most
SOLVE_P = 400
TAU = (0.7, 1.3)                               # (tau_e, tau_g) of the GPU tests
TOL = 1e-10


def vmat(phi, tau_e, tau_g):
    return tau_e * np.eye(phi.shape[0]) + tau_g * phi


def dense(phi, B, tau_e, tau_g):
    v = vmat(phi, tau_e, tau_g)
    low = np.linalg.cholesky(v)
    return np.linalg.solve(low.T, np.linalg.solve(low, B))


def pcg(phi, B, tau_e, tau_g, tol=TOL, max_iter=500):
    """(x, iters, converged, true residuals, the largest |x_k|_2 of every column)."""
    B = np.asarray(B, dtype=np.float64)
    one = B.ndim == 1
    B = B.reshape(B.shape[0], -1)
    n, m = B.shape
    v = vmat(phi, tau_e, tau_g)
    d = np.diag(v).copy()
    x, r = np.zeros((n, m)), B.copy()
    z = r / d[:, None]
    p = z.copy()
    rz = np.einsum("ij,ij->j", r, z)
    bnorm = np.sqrt(np.einsum("ij,ij->j", B, B))
    frozen = bnorm <= tol * bnorm                                   # (a NaN is never frozen)
    conv = frozen.copy()
    iters = np.zeros(m, dtype=np.int32)
    theta = np.zeros(m)
    for _ in range(max_iter):
        if frozen.all():
            break
        live = ~frozen
        vp = v @ p[:, live]
        pvp = np.einsum("ij,ij->j", p[:, live], vp)
        with np.errstate(invalid="ignore", divide="ignore"):
            alpha = np.where(pvp == 0.0, 0.0, rz[live] / pvp)
        x[:, live] += alpha * p[:, live]
        r[:, live] -= alpha * vp
        z[:, live] = r[:, live] / d[:, None]
        iters[live] += 1
        theta[live] = np.maximum(theta[live], np.linalg.norm(x[:, live], axis=0))
        rzn = np.einsum("ij,ij->j", r[:, live], z[:, live])
        done = np.sqrt(np.einsum("ij,ij->j", r[:, live], r[:, live])) <= tol * bnorm[live]
        with np.errstate(invalid="ignore", divide="ignore"):
            beta = np.where(done | (rz[live] == 0.0), 0.0, rzn / rz[live])
        rz[live] = rzn
        p[:, live] = z[:, live] + beta * p[:, live]
        idx = np.flatnonzero(live)
        frozen[idx[done]] = True
        conv[idx[done]] = True
    res = np.linalg.norm(B - v @ x, axis=0)
    if one:
        return x[:, 0], iters, conv, res, theta
    return x, iters, conv, res, theta


def residual_bound(reported, tau_g, e_fro, v_fro, n, m, xnorm):
    return reported + (tau_g * e_fro + 8.0 * (n + m) * U * v_fro) * xnorm


def gap_bound(iters, n, v_fro, theta, bnorm):
    return iters * U * ((2.0 * n + 6.0) * v_fro * theta + bnorm)


def eval_bound(n, v_fro, xnorm, bnorm):
    return (n + 4.0) * U * (v_fro * xnorm + bnorm)


def rhs(n, m, seed=0):
    """The right-hand sides of the tests: standard normal, seeded by the shape."""
    return np.random.default_rng(7919 * n + 31 * m + seed).standard_normal((n, m))


# ---- the REML null model (csrc/lmm.hip: mih_lmm_null) ---------------------------------------------------------------------------
"""reml(phi, y, Z, ...): y = Z alpha + g + e, g ~ N(0, tau_g Phi), e ~ N(0, tau_e I), by average-information REML as GMMAT and
SAIGE run it for a Gaussian trait, the traces by Hutchinson's estimate on fixed Rademacher probes.  Step for step what the
device does; solver="pcg" is the statement (this file's pcg at cg_tol), solver="dense" the reference (Cholesky solves);
exact=True replaces the two trace estimates by tr P and tr P Phi from the dense inverse.
    probes: u_k(i) = +1 if the top bit of splitmix64's output function at seed + golden (128 i + k + 1) is 0, else -1
    start:  e0 = y - Z (Z'Z)^-1 Z'y, s2 = e0'e0 / (n - c), dbar = mean Phi_ii, tau = (tau_e, tau_g) = (s2 / 2, s2 / (2 dbar))
    iteration:
      1. S = V^-1 [y, Z, U]
      2. H = sym(Z'S_Z), Sigma = H^-1, alpha = Sigma Z'S_y
      3. P [y, U] = S_{y,U} - S_Z Sigma (Z'S_{y,U})
      4. a = P y; Phi a; T = V^-1 [a, Phi a]; P a = T_a - S_Z Sigma Z'T_a, P Phi a likewise
      5. score = ((a'a - t_e) / 2, (a'Phi a - t_g) / 2), t_e = mean_k u_k'P u_k, t_g = mean_k (Phi u_k)'P u_k
      6. AI = [a, Phi a]'[P a, P Phi a] / 2, symmetrised
      7. tau' = tau + 2^-h AI^-1 score, the smallest h >= 0 with tau'_i >= tau_i / 10 for both i
         the boundary rule: tau'_g < 1e-8 s2 ends the fit with state 2, tau = (s2, 0) -- the OLS fit in closed form
      8. converged (state 1) when 2 max_i |tau'_i - tau_i| / (|tau'_i| + |tau_i|) <= tol_reml; the iterate is tau' either way
    finish: at the final tau steps 1-3 on [y, Z] give alpha and a = P y
    variance ratio (GRAMMAR-Gamma / SAIGE): for the columns g_j of G, rho_j = g_j'P g_j / |(I - Z (Z'Z)^-1 Z') g_j|^2 with
      P g_j = S_g - S_Z Sigma Z'S_g from one more batched solve; gamma = mean rho_j
    the scan: score_test(A = P y, w = None, Z) as it is, then, in this order, each on the arrays score_test returned:
      z' = z / sqrt(gamma), beta' = beta / gamma, se' = se / sqrt(gamma), -log10 p from z' by the host's finite-tail function
Choices the outline leaves open, made here: the convergence test looks at the step actually taken (after the halving); the
iteration count includes the iteration that hits the boundary; trace holds (t_e, t_g) of the last iteration; the number of CG
iterations of a batched solve is that of its slowest column."""
MASK = (1 << 64) - 1


def probes(seed, n, m):
    i, k = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(m, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(128) * i + k + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return np.where((z >> np.uint64(63)) == 0, 1.0, -1.0)


def ols(y, Z):
    """(e0, s2, (Z'Z)^-1)."""
    zinv = np.linalg.inv(Z.T @ Z)
    e0 = y - Z @ (zinv @ (Z.T @ y))
    return e0, float(e0 @ e0) / (Z.shape[0] - Z.shape[1]), zinv


def ai_step(tau, score, ai):
    ai = (ai + ai.T) / 2.0
    delta = np.linalg.solve(ai, score)
    for h in range(61):
        nxt = tau + 2.0 ** -h * delta
        if np.all(nxt >= 0.1 * tau):
            return nxt, h
    raise FloatingPointError("no step keeps the components")


def rel_change(a, b):
    return float(np.max(2.0 * np.abs(a - b) / (np.abs(a) + np.abs(b))))


class Fit:
    pass


def reml(phi, y, Z, nprobes=30, seed=0, G=None, tol_reml=1e-5, max_iter=50, cg_tol=1e-10, cg_max_iter=500, solver="pcg", exact=False, kappa=False):
    """kappa=True (dense solves only) also records the largest condition number of V along the trajectory, f.kappa."""
    n, c = Z.shape
    f = Fit()
    f.cg_iters, f.worst, f.kappa = 0, 0.0, 0.0

    def solve(B, tau):
        if solver == "dense":
            if kappa:
                lam = np.linalg.eigvalsh(vmat(phi, tau[0], tau[1]))
                f.kappa = max(f.kappa, float(lam[-1] / lam[0]))
            return dense(phi, B, tau[0], tau[1])
        x, it, conv, res, _ = pcg(phi, B, tau[0], tau[1], cg_tol, cg_max_iter)
        f.cg_iters += int(it.max())
        bn = np.linalg.norm(B, axis=0)
        f.worst = max(f.worst, float(np.max(np.where(bn > 0, res / np.where(bn > 0, bn, 1.0), 0.0))))
        return x

    def project(S):
        """(Sigma, S_Z, P applied to every column of [y, Z, ...])."""
        SZ = S[:, 1:1 + c]
        sigma = np.linalg.inv((Z.T @ SZ + (Z.T @ SZ).T) / 2.0)
        return sigma, SZ, S - SZ @ (sigma @ (Z.T @ S))

    e0, s2, zinv = ols(y, Z)
    dbar = float(np.mean(np.diag(phi)))
    U = probes(seed, n, nprobes)
    phiu = phi @ U
    tau = np.array([s2 / 2.0, s2 / (2.0 * dbar)])
    f.path, f.state, f.iters, f.trace = [tau.copy()], 0, 0, np.zeros(2)
    rhs0 = np.column_stack([y, Z, U])
    while f.iters < max_iter:
        S = solve(rhs0, tau)
        sigma, SZ, PS = project(S)
        a = PS[:, 0]
        if exact:
            vinv = np.linalg.inv(vmat(phi, tau[0], tau[1]))
            pm = vinv - vinv @ Z @ np.linalg.inv(Z.T @ vinv @ Z) @ Z.T @ vinv
            f.trace = np.array([np.trace(pm), np.trace(pm @ phi)])
        else:
            PU = PS[:, 1 + c:]
            f.trace = np.array([np.mean(np.einsum("ij,ij->j", U, PU)), np.mean(np.einsum("ij,ij->j", phiu, PU))])
        ab = np.column_stack([a, phi @ a])
        T = solve(ab, tau)
        PT = T - SZ @ (sigma @ (Z.T @ T))
        score = 0.5 * (np.array([a @ a, a @ ab[:, 1]]) - f.trace)
        nxt, _ = ai_step(tau, score, 0.5 * (ab.T @ PT))
        f.iters += 1
        if nxt[1] < 1e-8 * s2:
            f.state, tau = 2, np.array([s2, 0.0])
            f.path.append(tau.copy())
            break
        change = rel_change(nxt, tau)
        tau = nxt
        f.path.append(tau.copy())
        f.last_change = change
        if change <= tol_reml:
            f.state = 1
            break
    S = solve(rhs0[:, :1 + c], tau)
    sigma, SZ, PS = project(S)
    f.tau, f.alpha, f.py, f.dbar, f.s2 = tau, sigma @ (Z.T @ S[:, 0]), PS[:, 0], dbar, s2
    f.path = np.array(f.path)
    f.h2 = tau[1] * dbar / (tau[1] * dbar + tau[0])
    f.ratios, f.gamma = np.zeros(0), float("nan")
    if G is not None and G.shape[1]:
        SG = solve(G, tau)
        PG = SG - SZ @ (sigma @ (Z.T @ SG))
        gt = G - Z @ (zinv @ (Z.T @ G))
        f.ratios = np.einsum("ij,ij->j", G, PG) / np.einsum("ij,ij->j", gt, gt)
        f.gamma = float(np.mean(f.ratios))
    return f


def phenotype(xs, Z, alpha, sg2, se2, seed):
    """y = Z alpha + sigma_g X~ b / sqrt(p) + sigma_e eps with X~ the standardised matrix Phi = X~ X~' / p is built from, so that
    Cov(y) = sigma_g^2 Phi + sigma_e^2 I exactly."""
    rng = np.random.default_rng(seed)
    n, p = xs.shape
    return Z @ alpha + np.sqrt(sg2) * (xs @ rng.standard_normal(p)) / np.sqrt(p) + np.sqrt(se2) * rng.standard_normal(n)


def covariates(n, c, seed):
    rng = np.random.default_rng(seed + 17)
    return np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])


def rescale(z, beta, se, gamma):
    """The scan's host operations, in the stated order; -log10 p is then the host's finite-tail function of z'."""
    return z / np.sqrt(gamma), beta / gamma, se / np.sqrt(gamma)
