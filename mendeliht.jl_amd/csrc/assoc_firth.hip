// assoc_firth.hip -- the Firth-penalised effect size and likelihood-ratio p-value of the case-control association scan
// (mih_assoc_score_firth, driven from assoc.hip after the plain scan's finish).  tests/firth_spec.py states the definitions in
// numpy; firth_finish.h has the control of the root iteration and the host's finish of a column.
//
// The covariates' effects are held at the null fit as an offset (the approximate Firth test of REGENIE), which leaves a
// one-parameter logistic model in the covariate-adjusted genotype c_i whose log-likelihood is beta q - K(beta), K the cumulant
// generating function of the saddlepoint pass.  Jeffreys' penalty adds log K2(beta) / 2; the penalised score equation is
//     g(beta) = K1 - K3 / (2 K2) = q,      g' = D = K2 - (K4 K2 - K3^2) / (2 K2^2),
// K1 .. K4 the first four derivatives of K.  k_assoc_firth solves it per flagged column, one 256-thread workgroup per column for
// the whole solve, under the safeguard of the saddlepoint root (spa_iter_step) with the exact slope D.
//
// Layout: that of k_assoc_spa.  The selection, alpha and the slabs are the saddlepoint pass's own (assoc_flag_run), the slab of
// c_i is formed ONCE per column by the shared spa_slab_form, and an evaluation is one 8-byte load beside eta_i and mu_i, one exp
// and one division per row; it carries four sums where the saddlepoint's carries two.  A pass takes a thread's rows four at a
// time (kSpaAhead) and the last 0 .. 3 singly -- n <= 768 has only single rows, n >= 1024 both in every thread -- in the same
// order of additions; there is no other path that depends on n.  K and K2 at the root come from spa_pass<true> as it stands.
//
// Sums: every thread adds its rows tid, tid + 256, ... in ascending order, then the 256 partial sums go over the fixed LDS tree
// (spa_tree).  No atomics, contraction off.  The control values (SpaIter) live in registers: every lane reads the same four sums
// from LDS and makes the same step.  All sums of a column are made inside one workgroup and U, b, V are bit-reproducible, so the
// Firth outputs, the evaluation counts included, are bit for bit the same whatever slice_rows and the number of workgroups, and
// on repeated calls.
#include "assoc_slab.h"
#include "firth_finish.h"
#include <cmath>
#include <limits>
#include <vector>

namespace mih {

// the terms of one row: sigma - mu, s = sigma (1 - sigma), s omega (omega = 1 - 2 sigma) and s (1 - 6 s), times c, c^2, c^3, c^4
__device__ __forceinline__ void firth_term(double cc, double h, double mu, double t, double &a1, double &a2, double &a3, double &a4)
{
#pragma clang fp contract(off)
    const double x = h + cc * t, e = exp(-fabs(x)), r = 1.0 / (1.0 + e), er = e * r;
    const double s = er * r, d = (1.0 - e) * r, c2 = cc * cc;
    a1 = a1 + cc * ((x >= 0.0 ? r : er) - mu);
    a2 = a2 + c2 * s;
    a3 = a3 + (c2 * cc) * (s * (x >= 0.0 ? -d : d));
    a4 = a4 + (c2 * c2) * (s * (1.0 - 6.0 * s));
}

// One evaluation at argument t: this thread's shares of K1 .. K4, its rows in ascending order, kSpaAhead loads ahead.
__device__ __forceinline__ void firth_pass(const double *cs, const double *__restrict__ eta, const double *__restrict__ mu, int64_t n,
                                           double t, double &a1, double &a2, double &a3, double &a4)
{
    a1 = 0.0; a2 = 0.0; a3 = 0.0; a4 = 0.0;
    int64_t i = threadIdx.x;
    for (; i + 256 * (kSpaAhead - 1) < n; i += 256 * kSpaAhead) {
        double cc[kSpaAhead], h[kSpaAhead], mm[kSpaAhead];
        #pragma unroll
        for (int u = 0; u < kSpaAhead; ++u) { cc[u] = cs[i + 256 * u]; h[u] = eta[i + 256 * u]; mm[u] = mu[i + 256 * u]; }
        #pragma unroll
        for (int u = 0; u < kSpaAhead; ++u) firth_term(cc[u], h[u], mm[u], t, a1, a2, a3, a4);
    }
    for (; i < n; i += 256) firth_term(cs[i], eta[i], mu[i], t, a1, a2, a3, a4);
}

// The solve.  rec[6 f ..] = q, V, beta_hat, K(beta_hat), K2(beta_hat), I0 = K2 of the first evaluation; st[2 f ..] = status and
// evaluations (FirthRoot).  slab: gridDim.x x n doubles.
// Registers: left to itself the compiler gives the dense and dosage kinds 132 VGPRs (the 2-bit kind 123), three waves a SIMD
// where k_assoc_spa has four, and a pass is bound by the latency of its loads at that occupancy.  Asked for four waves a SIMD it
// fits 111 (dense, dosage) and 120 (2-bit) without scratch.
template <int KIND>      // 0: f64, 1: f32, 2: dosage, 3: 2-bit
__global__ void __launch_bounds__(256, 4)
k_assoc_firth(ColView m, int64_t n, int64_t p, int c, const int64_t *__restrict__ idx, int64_t nflag, const double *__restrict__ alpha,
              const double *__restrict__ Z, const double *__restrict__ eta, const double *__restrict__ mu, const double *__restrict__ sp0,
              const double *__restrict__ S, const double *__restrict__ V, double *__restrict__ slab, double *__restrict__ rec,
              int32_t *__restrict__ st)
{
#pragma clang fp contract(off)
    __shared__ double red[4][256];
    __shared__ double al[64];
    const int tid = threadIdx.x;
    double *cs = slab + (int64_t)blockIdx.x * n;
    for (int64_t f = blockIdx.x; f < nflag; f += gridDim.x) {
        const int64_t j = idx[f];
        __syncthreads();                                     // the last column's reads of al and red are over
        if (tid < c) al[tid] = alpha[f * c + tid];
        double a0, a1, a2;
        spa_slab_form<KIND>(m, n, j, c, al, Z, mu, cs, a0, a1, a2);
        red[0][tid] = a0;
        spa_tree(red, 1);
        const double m1 = red[0][0];
        const double q = S[j], v = V[j], tol = kSpaTolF * sqrt(v);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        double I0 = nan, bh = nan, K0 = nan, K2 = nan;
        SpaIter it;
        spa_iter_start(it);
        while (it.status == 0) {
            double k1, k2, k3, k4;
            firth_pass(cs, eta, mu, n, it.t, k1, k2, k3, k4);
            __syncthreads();                                 // every lane has read the sums of the evaluation before
            red[0][tid] = k1; red[1][tid] = k2; red[2][tid] = k3; red[3][tid] = k4;
            spa_tree(red, 4);
            if (it.evals == 0) I0 = red[1][0];
            firth_iter_step(it, red[0][0], red[1][0], red[2][0], red[3][0], q, tol);
        }
        if (it.status == 1) {
            bh = it.that;
            if (bh - bh == 0.0) {                            // finite: K and K2 at the root, the one pass with log1p
                double k0, k2;
                spa_pass<true>(cs, eta, sp0, n, bh, k0, k2);
                __syncthreads();
                red[0][tid] = k0; red[1][tid] = k2;
                spa_tree(red, 2);
                K0 = red[0][0] - bh * m1;
                K2 = red[1][0];
            }
        }
        if (tid == 0) {
            double *r = rec + 6 * f;
            r[0] = q; r[1] = v; r[2] = bh; r[3] = K0; r[4] = K2; r[5] = I0;
            st[2 * f] = it.status; st[2 * f + 1] = it.evals;
        }
    }
}

double assoc_firth_bytes(int64_t p)
{
    return (double)p * (48.0 + 8.0);                         // the roots' values and their status words, had every column been flagged
}

int assoc_firth_run(const AssocScan &sc, const AssocFlagged &fl, FirthOut &out)
{
    const mih_mat *h = sc.h;
    hipStream_t s = sc.s;
    const int64_t p = h->p, nflag = fl.nflag;
    out.beta.assign(sc.beta, sc.beta + p);
    out.se.assign(sc.se, sc.se + p);
    out.nlp.assign(sc.nlp, sc.nlp + p);
    out.state.assign((size_t)p, 0);
    out.evals.assign((size_t)p, 0);
    if (nflag == 0) return MIH_OK;

    std::vector<double> hrec;
    std::vector<int32_t> hst;
    MIH_TRY(assoc_solver_launch(sc, fl, "k_assoc_firth", 6, 2, [](auto K) { return k_assoc_firth<decltype(K)::value>; }, hrec, hst));

    int64_t total = 0;
    for (int64_t f = 0; f < nflag; ++f) {
        const int64_t j = fl.hidx[(size_t)f];
        const double *r = &hrec[(size_t)(6 * f)];
        const FirthRoot root = {r[2], r[3], r[4], r[5], (int)hst[(size_t)(2 * f)], (int)hst[(size_t)(2 * f + 1)]};
        out.state[(size_t)j] = (uint8_t)firth_column(root, r[0], r[1], sc.beta[j], sc.se[j], sc.nlp[j], &out.beta[(size_t)j], &out.se[(size_t)j],
                                                     &out.nlp[(size_t)j]);
        out.evals[(size_t)j] = root.evals;
        total += root.evals;
    }
    // a record without a kernel for the measurement hook: the columns tried and the evaluations they took
    PassRecord er;
    if (prof_begin(h, s, er)) {
        snprintf(er.kernel, sizeof(er.kernel), "assoc_firth_evals");
        er.residuals = (int)std::min<int64_t>(nflag, 2147483647); er.operands = (int)std::min<int64_t>(total, 2147483647);
        prof_end(h, s, er);
    }
    return MIH_OK;
}

void firth_publish(const FirthCall &call, const FirthOut &out)
{
    memcpy(call.beta, out.beta.data(), sizeof(double) * out.beta.size());
    memcpy(call.se, out.se.data(), sizeof(double) * out.se.size());
    memcpy(call.neglog10p, out.nlp.data(), sizeof(double) * out.nlp.size());
    memcpy(call.state, out.state.data(), out.state.size());
    if (call.evals) memcpy(call.evals, out.evals.data(), sizeof(int32_t) * out.evals.size());
}

}  // namespace mih
