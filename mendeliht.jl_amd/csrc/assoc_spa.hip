// assoc_spa.hip -- the saddlepoint-corrected p-value of the case-control association scan (mih_assoc_score_spa, driven from
// assoc.hip after the plain scan's finish).  tests/spa_spec.py states the definitions in numpy; spa_finish.h has the control of
// the root iteration and the host's finish of a column.
//
// The plain scan leaves U_j, b_j, V_j and z_j on the device.  k_assoc_spa_select compacts, in column order, the indices of the
// columns with a finite |z_j| >= cutoff (NaN marks the degenerate ones); k_assoc_spa_alpha forms alpha_j = Linv' (Linv b_j) for
// them; k_assoc_spa solves K'(t) = +|q| and K'(t) = -|q| per flagged column, one 256-thread workgroup per column for the whole
// solve.
//
// Layout.  c_i = x_ij - Z_i. alpha_j is formed ONCE per column into a slab of n doubles that belongs to the workgroup (the grid is
// capped at kSpaSlabs workgroups, each walks the flagged columns blockIdx.x, blockIdx.x + gridDim.x, ...).  Forming it anew in
// every evaluation would cost a decode and c + 1 loads and c multiply-adds per row, up to 64 of them, about a dozen times per
// column; from the slab an evaluation is one 8-byte load beside eta_i and mu_i, one exp and one division per row whatever c is.
// No path depends on the size of n: nothing is staged in LDS by n, the slab is global memory at every n.  A pass takes a thread's
// rows four at a time (kSpaAhead) and the last 0 .. 3 of them singly -- n <= 768 has only single rows, n >= 1024 both in every
// thread -- in the same order of additions.
//
// Sums: every thread adds its rows tid, tid + 256, ... in ascending order, then the 256 partial sums go over a fixed LDS tree
// (k = 128, 64, ... 1: red[tid] += red[tid + k]).  No atomics, contraction off.  All sums of a column are made inside one
// workgroup and U, b, V are bit-reproducible, so neglog10p_spa, state and t_hat are bit for bit the same whatever slice_rows
// and the number of workgroups, and on repeated calls.  The loop's control values (SpaIter) live in registers: every lane reads
// the same two sums from LDS and makes the same step.
//
// The slab's formation, the tree and the pass over the rows live in assoc_slab.h, one copy for this kernel and k_assoc_firth;
// the selection, alpha and the slabs (assoc_flag_run) serve both passes of a call that asks for both.
#include "assoc_slab.h"
#include "spa_finish.h"
#include <cmath>
#include <limits>
#include <vector>

namespace mih {

// per row: mu_i = sigma(eta_i) and softplus(eta_i), by the expressions of the evaluations (so that every term of K'(0) is 0)
__global__ void __launch_bounds__(256)
k_assoc_spa_rows(const double *__restrict__ eta, int64_t n, double *__restrict__ mu, double *__restrict__ sp0)
{
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    const double x = eta[i], e = exp(-fabs(x)), r = 1.0 / (1.0 + e);
    mu[i] = x >= 0.0 ? r : e * r;
    sp0[i] = fmax(x, 0.0) + log1p(e);
}

// idx[0 .. count): the columns with a finite |z| >= cutoff in ascending order; idx[p] = count.  One workgroup walks the columns
// 256 at a time: a ballot per wave, the four counts through LDS, the running total in a register of every lane.
__global__ void __launch_bounds__(256)
k_assoc_spa_select(const double *__restrict__ z, int64_t p, double cutoff, int64_t *__restrict__ idx)
{
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t base = 0;
    for (int64_t j0 = 0; j0 < p; j0 += 256) {
        const int64_t j = j0 + threadIdx.x;
        bool f = false;
        if (j < p) { const double a = fabs(z[j]); f = a >= cutoff && a < HUGE_VAL; }
        const unsigned long long m = __ballot(f);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int64_t off = base;
        for (int w = 0; w < wave; ++w) off += wcnt[w];
        if (f) idx[off + __popcll(m & ((1ull << lane) - 1ull))] = j;
        base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) idx[p] = base;
}

// alpha_f = Linv' (Linv b_j), j = idx[f], one thread per flagged column: u_k = sum_{l <= k} Linv[k][l] b_l (l ascending) into
// alpha[f c + k], then alpha_k = sum_{l >= k} Linv[l][k] u_l (l ascending) in place, k ascending (entry k is read by no later k).
__global__ void __launch_bounds__(256)
k_assoc_spa_alpha(const double *__restrict__ S, int64_t p, int c, const double *__restrict__ Linv, const int64_t *__restrict__ idx,
                  int64_t nflag, double *__restrict__ alpha)
{
#pragma clang fp contract(off)
    const int64_t f = blockIdx.x * 256ll + threadIdx.x;
    if (f >= nflag) return;
    const int64_t j = idx[f];
    double *a = alpha + f * c;
    for (int k = 0; k < c; ++k) {
        double u = 0.0;
        for (int l = 0; l <= k; ++l) u = u + Linv[k * c + l] * S[(int64_t)(1 + l) * p + j];
        a[k] = u;
    }
    for (int k = 0; k < c; ++k) {
        double v = 0.0;
        for (int l = k; l < c; ++l) v = v + Linv[l * c + k] * a[l];
        a[k] = v;
    }
}

// The solve.  rec[8 f ..] = q, V, then t_hat, K(t_hat), K''(t_hat) of tail 0 (target +|q|) and of tail 1 (-|q|); st[4 f ..] =
// status and evaluations of tail 0, of tail 1 (SpaTail).  slab: gridDim.x x n doubles.
template <int KIND>      // 0: f64, 1: f32, 2: dosage, 3: 2-bit
__global__ void __launch_bounds__(256)
k_assoc_spa(ColView m, int64_t n, int64_t p, int c, const int64_t *__restrict__ idx, int64_t nflag, const double *__restrict__ alpha,
            const double *__restrict__ Z, const double *__restrict__ eta, const double *__restrict__ mu, const double *__restrict__ sp0,
            const double *__restrict__ S, const double *__restrict__ V, double *__restrict__ slab, double *__restrict__ rec,
            int32_t *__restrict__ st)
{
#pragma clang fp contract(off)
    __shared__ double red[3][256];
    __shared__ double al[64];
    const int tid = threadIdx.x;
    double *cs = slab + (int64_t)blockIdx.x * n;
    for (int64_t f = blockIdx.x; f < nflag; f += gridDim.x) {
        const int64_t j = idx[f];
        __syncthreads();                                     // the last column's reads of al and red are over
        if (tid < c) al[tid] = alpha[f * c + tid];
        double a0, a1, a2;
        spa_slab_form<KIND>(m, n, j, c, al, Z, mu, cs, a0, a1, a2);
        red[0][tid] = a0; red[1][tid] = a1; red[2][tid] = a2;
        spa_tree(red, 3);
        const double m1 = red[0][0], smin = red[1][0] - m1, smax = red[2][0] - m1;
        const double q = S[j], v = V[j], aq = fabs(q), tol = kSpaTolF * sqrt(v);
        const int obs = q >= 0.0 ? 0 : 1;
        if (tid == 0) { rec[8 * f] = q; rec[8 * f + 1] = v; }
        for (int k = 0; k < 2; ++k) {
            const double s = k == 0 ? aq : -aq;
            const double nan = std::numeric_limits<double>::quiet_NaN();
            double that = nan, K0 = nan, K2 = nan;
            int status = 0, evals = 0;
            if (k == obs || (k == 0 ? s < smax : s > smin)) {
                SpaIter it;
                spa_iter_start(it);
                while (it.status == 0) {
                    double k1, k2;
                    spa_pass<false>(cs, eta, mu, n, it.t, k1, k2);
                    __syncthreads();                         // every lane has read the sums of the evaluation before
                    red[0][tid] = k1; red[1][tid] = k2;
                    spa_tree(red, 2);
                    spa_iter_step(it, red[0][0], red[1][0], s, tol);
                }
                status = it.status; evals = it.evals;
                if (status == 1) {
                    that = it.that;
                    if (that - that == 0.0) {                // finite: K and K'' at the root, the one pass with log1p
                        double k0, k2;
                        spa_pass<true>(cs, eta, sp0, n, that, k0, k2);
                        __syncthreads();
                        red[0][tid] = k0; red[1][tid] = k2;
                        spa_tree(red, 2);
                        K0 = red[0][0] - that * m1;
                        K2 = red[1][0];
                    }
                }
            }
            if (tid == 0) {
                rec[8 * f + 2 + 3 * k] = that; rec[8 * f + 3 + 3 * k] = K0; rec[8 * f + 4 + 3 * k] = K2;
                st[4 * f + 2 * k] = status; st[4 * f + 2 * k + 1] = evals;
            }
        }
    }
}

double assoc_flag_bytes(int64_t n, int64_t p, int c)
{
    const double dn = (double)n, dp = (double)p;
    return 8.0 * 3.0 * dn                                    // eta, mu, softplus(eta)
         + 8.0 * (dp + 1.0)                                  // the flagged columns' indices and their count
         + dp * (8.0 * c)                                    // alpha, had every column been flagged
         + 8.0 * dn * (double)std::min<int64_t>(p, kSpaSlabs);      // the slabs of c_i
}

double assoc_spa_bytes(int64_t n, int64_t p, int c)
{
    return assoc_flag_bytes(n, p, c) + (double)p * (64.0 + 16.0);   // the tails' values and their status words, had every column been flagged
}

int assoc_flag_run(const char *who, const AssocScan &sc, const double *eta_host, double cutoff, AssocFlagged &fl)
{
    hipStream_t s = sc.s;
    const int c = sc.c;
    const int64_t n = sc.h->n, p = sc.h->p;
    fl.nflag = 0; fl.grid = 0;
    MIH_TRY(fl.idx.alloc((size_t)p + 1));
    hipLaunchKernelGGL(k_assoc_spa_select, dim3(1), dim3(256), 0, s, sc.z, p, cutoff, fl.idx.p);
    MIH_TRY(launch_failed("k_assoc_spa_select"));
    int64_t nflag = 0;
    MIH_HIP(hipMemcpyAsync(&nflag, fl.idx.p + p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    if (nflag < 0 || nflag > p) { set_error("%s: the selection counted %lld of %lld columns", who, (long long)nflag, (long long)p); return MIH_HIP_ERROR; }
    if (nflag == 0) return MIH_OK;

    const int64_t grid = std::min(nflag, kSpaSlabs);
    MIH_TRY(fl.eta.alloc((size_t)n)); MIH_TRY(fl.mu.alloc((size_t)n)); MIH_TRY(fl.sp0.alloc((size_t)n));
    MIH_TRY(fl.alpha.alloc((size_t)(nflag * c))); MIH_TRY(fl.slab.alloc((size_t)(grid * n)));
    MIH_HIP(hipMemcpyAsync(fl.eta.p, eta_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_assoc_spa_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fl.eta.p, n, fl.mu.p, fl.sp0.p);
    MIH_TRY(launch_failed("k_assoc_spa_rows"));
    hipLaunchKernelGGL(k_assoc_spa_alpha, dim3((unsigned)((nflag + 255) / 256)), dim3(256), 0, s, sc.S, p, c, sc.Linv, fl.idx.p, nflag, fl.alpha.p);
    MIH_TRY(launch_failed("k_assoc_spa_alpha"));
    fl.hidx.resize((size_t)nflag);
    MIH_HIP(hipMemcpyAsync(fl.hidx.data(), fl.idx.p, sizeof(int64_t) * (size_t)nflag, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    for (int64_t f = 0; f < nflag; ++f)
        if (fl.hidx[(size_t)f] < 0 || fl.hidx[(size_t)f] >= p) { set_error("%s: flagged column %lld of %lld", who, (long long)fl.hidx[(size_t)f], (long long)p); return MIH_HIP_ERROR; }
    fl.nflag = nflag; fl.grid = grid;
    return MIH_OK;
}

int assoc_spa_run(const AssocScan &sc, const AssocFlagged &fl, SpaOut &out)
{
    const mih_mat *h = sc.h;
    hipStream_t s = sc.s;
    const int64_t p = h->p, nflag = fl.nflag;
    const double *nlp = sc.nlp;
    std::vector<double> &that = out.t_hat;
    out.nlp.assign(nlp, nlp + p);
    out.state.assign((size_t)p, 0);
    that.assign((size_t)(2 * p), std::numeric_limits<double>::quiet_NaN());
    if (nflag == 0) return MIH_OK;

    std::vector<double> hrec;
    std::vector<int32_t> hst;
    MIH_TRY(assoc_solver_launch(sc, fl, "k_assoc_spa", 8, 4, [](auto K) { return k_assoc_spa<decltype(K)::value>; }, hrec, hst));

    int64_t tails = 0, evals = 0;
    for (int64_t f = 0; f < nflag; ++f) {
        const int64_t j = fl.hidx[(size_t)f];
        const double *r = &hrec[(size_t)(8 * f)];
        const int32_t *w = &hst[(size_t)(4 * f)];
        SpaTail tl[2];
        for (int k = 0; k < 2; ++k) {
            tl[k] = SpaTail{r[2 + 3 * k], r[3 + 3 * k], r[4 + 3 * k], (int)w[2 * k], (int)w[2 * k + 1]};
            if (tl[k].status != 0) { ++tails; evals += tl[k].evals; }
            that[(size_t)(k * p + j)] = tl[k].status == 1 ? tl[k].t : std::numeric_limits<double>::quiet_NaN();
        }
        double val = 0.0;
        out.state[(size_t)j] = (uint8_t)spa_column(tl, r[0], r[1], nlp[j], &val);
        out.nlp[(size_t)j] = val;
    }
    // a record without a kernel for the measurement hook: the tails computed and the evaluations they took
    PassRecord er;
    if (prof_begin(h, s, er)) {
        snprintf(er.kernel, sizeof(er.kernel), "assoc_spa_evals");
        er.residuals = (int)std::min<int64_t>(tails, 2147483647); er.operands = (int)std::min<int64_t>(evals, 2147483647);
        prof_end(h, s, er);
    }
    return MIH_OK;
}

void spa_publish(const SpaCall &call, const SpaOut &out)
{
    memcpy(call.neglog10p_spa, out.nlp.data(), sizeof(double) * out.nlp.size());
    memcpy(call.state, out.state.data(), out.state.size());
    if (call.t_hat) memcpy(call.t_hat, out.t_hat.data(), sizeof(double) * out.t_hat.size());
}

}  // namespace mih
