// lmm.hip -- the mixed-model association scan's null model on the kinship matrix Phi of a genotype handle.  Two layers:
// mih_grm_solve, linear solves with V = tau_e I + tau_g Phi, X = V^-1 B for a block B of at most 128 columns; and mih_lmm_null,
// the variance-component model y = Z alpha + g + e, g ~ N(0, tau_g Phi), e ~ N(0, tau_e I) fitted by average-information REML
// on those solves (what SAIGE, fastGWA and GMMAT fit on related samples before they scan) -- without Phi leaving the device
// and without any n x n factorisation.  Everything n-sized is a product Phi B, a block Gram product or a thin rotation
// (grm_block.h) or one of the vector kernels here; the c x c and 2 x 2 algebra is the host's (lmm_host.h).
//
// Phi is built by grm_accumulate and mirrored into a full symmetric n_pad x n_pad matrix that stays in device memory for the
// call, as in pca.hip.  The solve is a conjugate gradient with the Jacobi preconditioner d = diag V, every column with scalars
// of its own (tests/lmm_spec.py states it in numpy):
//     x = 0, r = b, z = r / d, p = z, rz = r'z;  a column with |r| <= tol |b| is frozen -- a zero column at once
//     repeat  Vp = V p  (k_lmm_vmul);  alpha = rz / p'Vp;  x += alpha p;  r -= alpha Vp;  z = r / d;
//             frozen when |r| <= tol |b|;  else beta = r'z / rz, rz = r'z, p = z + beta p
//     until every column is frozen, or at max_iter;  then the true residual |b - V x| with one more product.
// The scalars alpha, beta, rz, the squared norms and the frozen flags never leave the device: k_lmm_alpha and k_lmm_beta compute
// them from partial sums over slabs of rows, added in ascending order, and the host reads one counter of live columns per
// check.  A frozen column is skipped by every later kernel, so how many iterations are queued between two checks changes no bit.
// No atomics; every sum of a column runs in an order that n_pad alone fixes: a column of the result does not depend on the
// other columns of the block, on panel_cols or on the call.
//
// Blocks are kept in the panel layout of grm.hip, B[c * n_pad + i]: bp = m rounded up to 16 columns, the columns beyond m and
// the rows beyond n all zeros -- b = 0 freezes the former at once, and V p keeps the latter (the pad rows of Phi are zeros).
#include "grm_block.h"
#include "lmm_host.h"
#include "normal_tail.h"
#include <algorithm>
#include <cmath>

namespace mih {

constexpr int kLmmSlabRows = 128;          // rows of a slab of the vector kernels: one workgroup of two waves, one row a thread
constexpr int kLmmScalWaves = 16;          // waves of the one workgroup that owns the scalars: wave w the columns w, w + 16, ...

// The sum of a wave's 64 values, the same in every lane: a butterfly, so the order is fixed.
__device__ __forceinline__ double lmm_wave_sum(double v)
{
    #pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// The sum of cnt partials by one wave: lane l adds l, l + 64, ... in ascending order, then the butterfly.
__device__ __forceinline__ double lmm_partial_sum(const double *__restrict__ part, int64_t cnt, int lane)
{
    double s = 0.0;
    for (int64_t k = lane; k < cnt; k += 64) s += part[k];
    return lmm_wave_sum(s);
}

// The two sums of a slab's 128 rows: each wave its butterfly, then wave 0 + wave 1.  Every thread of the workgroup must call.
__device__ __forceinline__ void lmm_slab_sums(double &a, double &b)
{
    __shared__ double s_a[2], s_b[2];
    a = lmm_wave_sum(a);
    b = lmm_wave_sum(b);
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    a = s_a[0] + s_a[1];
    b = s_b[0] + s_b[1];
}

// ---- d = diag V ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_lmm_diag(const double *__restrict__ Phi, int64_t n, int64_t n_pad, double tau_e, double tau_g, double *__restrict__ d)
{
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n_pad) d[i] = i < n ? fma(tau_g, Phi[i * n_pad + i], tau_e) : tau_e;
}

// ---- Y = V P ---------------------------------------------------------------------------------------------------------------------
// The walk of k_pca_spmm (grm_block_walk: the same order of every sum), then Y = tau_g (Phi P) + tau_e P, one fused
// multiply-add on the rounded tau_e P, and the partial sums of p'(Vp) that the walk has at hand: lane (r, q) holds, for every
// register, sample i0 + 16 ib + r of column 16 cb + q + 4 reg, so the 16 lanes of a quarter-wave add p_i y_i over the 16
// samples of a block by a butterfly.  pvp[c * nrb + i / 16] receives it: the granule is 16 rows whatever IB, so that the
// second stage (k_lmm_alpha) adds the same numbers in the same order for every <IB, NB>.
template <int IB, int NB>
__global__ void __launch_bounds__(64)
k_lmm_vmul(const double *__restrict__ Phi, const double *__restrict__ P, int64_t n_pad, int nb, double tau_e, double tau_g,
           double *__restrict__ Y, double *__restrict__ pvp)
{
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * (16 * IB), nrb = n_pad / 16;
    pca_v4d acc[IB][NB];
    grm_block_walk<IB, NB>(Phi, P, n_pad, nb, i0, acc);

    #pragma unroll
    for (int ib = 0; ib < IB; ++ib)
        #pragma unroll
        for (int cb = 0; cb < NB; ++cb)
            if (cb < nb)
                #pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int c = cb * 16 + q + 4 * reg;
                    const int64_t at = (int64_t)c * n_pad + i0 + ib * 16 + r;
                    const double pv = P[at];
                    const double y = fma(tau_g, acc[ib][cb][reg], tau_e * pv);
                    Y[at] = y;
                    double t = pv * y;
                    #pragma unroll
                    for (int w = 8; w > 0; w >>= 1) t += __shfl_xor(t, w, 16);
                    if (r == 0) pvp[(int64_t)c * nrb + i0 / 16 + ib] = t;
                }
}

// ---- the vector kernels: a workgroup = one slab of 128 rows of one column -------------------------------------------------------------
// x = 0, r = b, z = p = b / d; the partials of r'z and b'b
__global__ void __launch_bounds__(kLmmSlabRows)
k_lmm_init(const double *__restrict__ B, const double *__restrict__ d, int64_t n_pad, int64_t nslab, double *__restrict__ X,
           double *__restrict__ R, double *__restrict__ Z, double *__restrict__ P, double *__restrict__ part_rz, double *__restrict__ part_rr)
{
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kLmmSlabRows + threadIdx.x, at = (int64_t)c * n_pad + i;
    const double b = B[at], z = b / d[i];
    X[at] = 0.0; R[at] = b; Z[at] = z; P[at] = z;
    double rz = b * z, rr = b * b;
    lmm_slab_sums(rz, rr);
    if (threadIdx.x == 0) { part_rz[(int64_t)c * nslab + blockIdx.x] = rz; part_rr[(int64_t)c * nslab + blockIdx.x] = rr; }
}

// x += alpha p, r -= alpha Vp, z = r / d; the partials of r'z and r'r.  A frozen column is left as it is.
__global__ void __launch_bounds__(kLmmSlabRows)
k_lmm_update(const double *__restrict__ P, const double *__restrict__ VP, const double *__restrict__ d, const double *__restrict__ alpha,
             const int32_t *__restrict__ frozen, int64_t n_pad, int64_t nslab, double *__restrict__ X, double *__restrict__ R,
             double *__restrict__ Z, double *__restrict__ part_rz, double *__restrict__ part_rr)
{
    const int c = blockIdx.y;
    if (frozen[c]) return;                                                   // (the whole workgroup)
    const int64_t i = (int64_t)blockIdx.x * kLmmSlabRows + threadIdx.x, at = (int64_t)c * n_pad + i;
    const double a = alpha[c];
    X[at] = fma(a, P[at], X[at]);
    const double r = fma(-a, VP[at], R[at]), z = r / d[i];
    R[at] = r; Z[at] = z;
    double rz = r * z, rr = r * r;
    lmm_slab_sums(rz, rr);
    if (threadIdx.x == 0) { part_rz[(int64_t)c * nslab + blockIdx.x] = rz; part_rr[(int64_t)c * nslab + blockIdx.x] = rr; }
}

// p = z + beta p
__global__ void __launch_bounds__(kLmmSlabRows)
k_lmm_direction(const double *__restrict__ Z, const double *__restrict__ beta, const int32_t *__restrict__ frozen, int64_t n_pad,
                double *__restrict__ P)
{
    const int c = blockIdx.y;
    if (frozen[c]) return;
    const int64_t at = (int64_t)c * n_pad + (int64_t)blockIdx.x * kLmmSlabRows + threadIdx.x;
    P[at] = fma(beta[c], P[at], Z[at]);
}

// the partials of |b - Vx|^2
__global__ void __launch_bounds__(kLmmSlabRows)
k_lmm_residual(const double *__restrict__ B, const double *__restrict__ VX, int64_t n_pad, int64_t nslab, double *__restrict__ part_rr)
{
    const int c = blockIdx.y;
    const int64_t at = (int64_t)c * n_pad + (int64_t)blockIdx.x * kLmmSlabRows + threadIdx.x;
    const double t = B[at] - VX[at];
    double rr = t * t, unused = 0.0;
    lmm_slab_sums(rr, unused);
    if (threadIdx.x == 0) part_rr[(int64_t)c * nslab + blockIdx.x] = rr;
}

// ---- the scalars: one workgroup, wave w the columns w, w + 16, ... ----------------------------------------------------------------------
// The scalars of a call, all in device memory, bp of each.
struct LmmScal {
    double *rz, *bb, *alpha, *beta, *res;
    int32_t *frozen, *iters, *conv, *live;                                   // live: one counter, the columns < m not frozen
};

__device__ __forceinline__ void lmm_count_live(const LmmScal &sc, int m)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t live = 0;
        for (int c = 0; c < m; ++c) live += sc.frozen[c] ? 0 : 1;
        *sc.live = live;
    }
}

// stop: 0 the start (rz and |b|^2 from the partials of k_lmm_init, no iteration taken), 1 after an update.  A column is frozen
// when |r| <= tol |b|; the columns beyond m are frozen from the start.  0 / 0 (a direction without length, which only a
// residual of 0 gives) is 0.
__global__ void __launch_bounds__(64 * kLmmScalWaves)
k_lmm_beta(LmmScal sc, const double *__restrict__ part_rz, const double *__restrict__ part_rr, int64_t nslab, int m, int bp, double tol, int start)
{
    const int lane = threadIdx.x & 63;
    for (int c = threadIdx.x >> 6; c < bp; c += kLmmScalWaves) {
        if (!start && sc.frozen[c]) continue;                                // (the whole wave)
        const double rz = lmm_partial_sum(part_rz + (int64_t)c * nslab, nslab, lane);
        const double rr = lmm_partial_sum(part_rr + (int64_t)c * nslab, nslab, lane);
        if (lane == 0) {
            if (start) { sc.bb[c] = rr; sc.iters[c] = 0; sc.alpha[c] = 0.0; sc.res[c] = 0.0; }
            else sc.iters[c] += 1;
            const bool done = sqrt(rr) <= tol * sqrt(sc.bb[c]);
            const double old = start ? 0.0 : sc.rz[c];
            sc.beta[c] = done || old == 0.0 ? 0.0 : rz / old;
            sc.rz[c] = rz;
            if (start) { sc.frozen[c] = done || c >= m ? 1 : 0; sc.conv[c] = done ? 1 : 0; }
            else if (done) { sc.frozen[c] = 1; sc.conv[c] = 1; }
        }
    }
    lmm_count_live(sc, m);
}

// alpha = rz / p'Vp from the partials of k_lmm_vmul
__global__ void __launch_bounds__(64 * kLmmScalWaves)
k_lmm_alpha(LmmScal sc, const double *__restrict__ pvp, int64_t nrb, int bp)
{
    const int lane = threadIdx.x & 63;
    for (int c = threadIdx.x >> 6; c < bp; c += kLmmScalWaves) {
        if (sc.frozen[c]) continue;
        const double s = lmm_partial_sum(pvp + (int64_t)c * nrb, nrb, lane);
        if (lane == 0) sc.alpha[c] = s == 0.0 ? 0.0 : sc.rz[c] / s;
    }
}

// res = |b - Vx| from the partials of k_lmm_residual
__global__ void __launch_bounds__(64 * kLmmScalWaves)
k_lmm_resnorm(LmmScal sc, const double *__restrict__ part_rr, int64_t nslab, int bp)
{
    const int lane = threadIdx.x & 63;
    for (int c = threadIdx.x >> 6; c < bp; c += kLmmScalWaves) {
        const double s = lmm_partial_sum(part_rr + (int64_t)c * nslab, nslab, lane);
        if (lane == 0) sc.res[c] = sqrt(s);
    }
}

// ---- the probes of the trace estimates ----------------------------------------------------------------------------------------------
// U[k * n_pad + i] = +1 or -1 by the top bit (0: +1) of the output function of splitmix64 at seed + golden (128 i + k + 1), the
// hash of k_pca_start: an entry depends on (seed, i, k) alone.  Rows >= n are zeros.
__global__ void __launch_bounds__(256)
k_lmm_probes(double *__restrict__ Uc, int64_t n, int64_t n_pad, uint64_t seed)
{
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n_pad) return;
    double v = 0.0;
    if (i < n) {
        uint64_t z = seed + 0x9E3779B97F4A7C15ull * (128ull * (uint64_t)i + (uint64_t)k + 1ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        v = (z >> 63) ? -1.0 : 1.0;
    }
    Uc[(int64_t)k * n_pad + i] = v;
}

// The blocks and scalars of one call, and the solve over them.
struct LmmRun {
    const mih_mat *h = nullptr;
    hipStream_t s = nullptr;
    const double *phi = nullptr;
    int64_t n = 0, n_pad = 0, nslab = 0, nrb = 0;
    int bp = 0;                                                              // the width the blocks were allocated with
    DevBuf<double> blk[6], d, pvp, part_rz, part_rr, scal;                   // blk: x, r, z, p, Vp, B
    DevBuf<int32_t> flags;
    LmmScal sc{};

    void shape(const mih_mat *hh, int m)
    {
        n = hh->n;
        n_pad = hh->kind == 0 ? hh->n_pad : round_up(hh->n, kGrmTile);
        bp = (int)round_up(m, 16);
        nslab = n_pad / kLmmSlabRows;
        nrb = n_pad / 16;
    }
    // what alloc() takes, for the memory rule
    double bytes() const { return 8.0 * (6.0 * (double)n_pad * bp + (double)n_pad + (double)bp * ((double)nrb + 2.0 * (double)nslab + 5.0)) + 4.0 * (3.0 * bp + 1.0); }

    int alloc()
    {
        for (auto &b : blk) MIH_TRY(b.alloc((size_t)n_pad * bp));
        MIH_TRY(d.alloc((size_t)n_pad));
        MIH_TRY(pvp.alloc((size_t)bp * nrb));
        MIH_TRY(part_rz.alloc((size_t)bp * nslab));
        MIH_TRY(part_rr.alloc((size_t)bp * nslab));
        MIH_TRY(scal.alloc((size_t)5 * bp));
        MIH_TRY(flags.alloc((size_t)3 * bp + 1));
        sc.rz = scal.p; sc.bb = scal.p + bp; sc.alpha = scal.p + 2 * bp; sc.beta = scal.p + 3 * bp; sc.res = scal.p + 4 * bp;
        sc.frozen = flags.p; sc.iters = flags.p + bp; sc.conv = flags.p + 2 * bp; sc.live = flags.p + 3 * bp;
        return MIH_OK;
    }

    double *X() { return blk[0].p; }
    double *B() { return blk[5].p; }

    // Y = V P over the nbl leading blocks of 16 columns; the partials of p'Vp go to pvp
    int vmul(const double *P, double *Y, int nbl, double tau_e, double tau_g)
    {
        PassRecord rec;
        const bool timed = prof_begin(h, s, rec);
        if (nbl <= 2) hipLaunchKernelGGL((k_lmm_vmul<4, 2>), dim3((unsigned)(n_pad / 64)), dim3(64), 0, s, phi, P, n_pad, nbl, tau_e, tau_g, Y, pvp.p);
        else if (nbl <= 4) hipLaunchKernelGGL((k_lmm_vmul<2, 4>), dim3((unsigned)(n_pad / 32)), dim3(64), 0, s, phi, P, n_pad, nbl, tau_e, tau_g, Y, pvp.p);
        else hipLaunchKernelGGL((k_lmm_vmul<1, 8>), dim3((unsigned)(n_pad / 16)), dim3(64), 0, s, phi, P, n_pad, nbl, tau_e, tau_g, Y, pvp.p);
        if (timed) { snprintf(rec.kernel, sizeof(rec.kernel), "k_lmm_vmul"); rec.residuals = 16 * nbl; prof_end(h, s, rec); }
        return launch_failed("k_lmm_vmul");
    }

    // X = V^-1 B for the m leading columns of B (m <= bp; the columns from m to the next multiple of 16 must be zeros).  On
    // return X holds the solutions and the scalars the iterations, the flags and the true residuals.
    int solve(int m, double tau_e, double tau_g, double tol, int max_iter)
    {
        const int w = (int)round_up(m, 16), nbl = w / 16;
        double *x = blk[0].p, *r = blk[1].p, *z = blk[2].p, *p = blk[3].p, *vp = blk[4].p, *b = blk[5].p;
        const dim3 slabs((unsigned)nslab, (unsigned)w), one(1), scalars(64 * kLmmScalWaves);
        hipLaunchKernelGGL(k_lmm_diag, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, phi, n, n_pad, tau_e, tau_g, d.p);
        MIH_TRY(launch_failed("k_lmm_diag"));
        hipLaunchKernelGGL(k_lmm_init, slabs, dim3(kLmmSlabRows), 0, s, (const double *)b, (const double *)d.p, n_pad, nslab, x, r, z, p, part_rz.p, part_rr.p);
        MIH_TRY(launch_failed("k_lmm_init"));
        hipLaunchKernelGGL(k_lmm_beta, one, scalars, 0, s, sc, (const double *)part_rz.p, (const double *)part_rr.p, nslab, m, w, tol, 1);
        MIH_TRY(launch_failed("k_lmm_beta"));
        // between two looks at the counter a small problem queues several iterations (a look costs more than they do), a large
        // one a single one (an iteration too many costs a pass over Phi); either way the bits are the same
        const int queue = n_pad >= 8192 ? 1 : 8;
        int32_t live = 0;
        for (int it = 0;;) {
            MIH_HIP(hipMemcpyAsync(&live, sc.live, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            MIH_HIP(hipStreamSynchronize(s));
            if (live == 0 || it >= max_iter) break;
            for (int k = 0; k < queue && it < max_iter; ++k, ++it) {
                MIH_TRY(vmul(p, vp, nbl, tau_e, tau_g));
                hipLaunchKernelGGL(k_lmm_alpha, one, scalars, 0, s, sc, (const double *)pvp.p, nrb, w);
                MIH_TRY(launch_failed("k_lmm_alpha"));
                hipLaunchKernelGGL(k_lmm_update, slabs, dim3(kLmmSlabRows), 0, s, (const double *)p, (const double *)vp, (const double *)d.p,
                                   (const double *)sc.alpha, (const int32_t *)sc.frozen, n_pad, nslab, x, r, z, part_rz.p, part_rr.p);
                MIH_TRY(launch_failed("k_lmm_update"));
                hipLaunchKernelGGL(k_lmm_beta, one, scalars, 0, s, sc, (const double *)part_rz.p, (const double *)part_rr.p, nslab, m, w, tol, 0);
                MIH_TRY(launch_failed("k_lmm_beta"));
                hipLaunchKernelGGL(k_lmm_direction, slabs, dim3(kLmmSlabRows), 0, s, (const double *)z, (const double *)sc.beta,
                                   (const int32_t *)sc.frozen, n_pad, p);
                MIH_TRY(launch_failed("k_lmm_direction"));
            }
        }
        // the true residual: one more product
        MIH_TRY(vmul(x, vp, nbl, tau_e, tau_g));
        hipLaunchKernelGGL(k_lmm_residual, slabs, dim3(kLmmSlabRows), 0, s, (const double *)b, (const double *)vp, n_pad, nslab, part_rr.p);
        MIH_TRY(launch_failed("k_lmm_residual"));
        hipLaunchKernelGGL(k_lmm_resnorm, one, scalars, 0, s, sc, (const double *)part_rr.p, nslab, w);
        return launch_failed("k_lmm_resnorm");
    }
};

}  // namespace mih

using namespace mih;

extern "C" {

int mih_grm_solve(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double tau_e, double tau_g, const double *B,
                  int32_t m, double tol, int32_t max_iter, double *X, int32_t *iters, int32_t *converged, double *residuals)
{
    const char *who = "mih_grm_solve";
    if (m < 1 || m > kPcaMaxBlock) { set_error("%s: m must be between 1 and %d, got %d", who, kPcaMaxBlock, (int)m); return MIH_BAD_ARG; }
    if (!std::isfinite(tau_e) || !(tau_e > 0.0)) { set_error("%s: tau_e must be finite and positive, got %g", who, tau_e); return MIH_BAD_ARG; }
    if (!std::isfinite(tau_g) || tau_g < 0.0) { set_error("%s: tau_g must be finite and not negative, got %g", who, tau_g); return MIH_BAD_ARG; }
    if (!std::isfinite(tol) || tol < 0.0) { set_error("%s: tol must be finite and not negative, got %g", who, tol); return MIH_BAD_ARG; }
    if (max_iter < 1) { set_error("%s: max_iter must be at least 1, got %d", who, (int)max_iter); return MIH_BAD_ARG; }

    LmmRun L;
    if (h) L.shape(h, m);
    GrmRun g;
    MIH_TRY(grm_accumulate(who, h, col_keep, method, panel_cols, L.bytes(), B && X && iters && converged && residuals, g));
    hipStream_t s = h->stream;
    MIH_TRY(grm_mirror(g, s));
    L.h = h; L.s = s; L.phi = g.acc.p;
    MIH_TRY(L.alloc());

    const int64_t n = L.n, n_pad = L.n_pad;
    const int bp = L.bp;
    MIH_HIP(hipMemsetAsync(L.B(), 0, sizeof(double) * (size_t)n_pad * bp, s));
    MIH_HIP(hipMemcpy2DAsync(L.B(), sizeof(double) * (size_t)n_pad, B, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)m,
                             hipMemcpyHostToDevice, s));
    MIH_TRY(L.solve(m, tau_e, tau_g, tol, max_iter));

    std::vector<double> x((size_t)n * m), res((size_t)bp);
    std::vector<int32_t> fl((size_t)3 * bp);
    MIH_HIP(hipMemcpy2DAsync(x.data(), sizeof(double) * (size_t)n, L.X(), sizeof(double) * (size_t)n_pad, sizeof(double) * (size_t)n, (size_t)m,
                             hipMemcpyDeviceToHost, s));
    MIH_HIP(hipMemcpyAsync(res.data(), L.sc.res, sizeof(double) * (size_t)bp, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipMemcpyAsync(fl.data(), L.flags.p, sizeof(int32_t) * (size_t)3 * bp, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    std::copy(x.begin(), x.end(), X);
    for (int c = 0; c < m; ++c) {
        iters[c] = fl[(size_t)bp + c];
        converged[c] = fl[(size_t)2 * bp + c];
        residuals[c] = res[(size_t)c];
    }
    return MIH_OK;
}

// The REML null model y = Z alpha + g + e, g ~ N(0, tau_g Phi), e ~ N(0, tau_e I), by average information with Hutchinson
// traces (tests/lmm_spec.py states every step in numpy).  Block columns: [y, Z (c), U (probes)].
int mih_lmm_null(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, const double *y, const double *Z, int32_t c,
                 int32_t probes, uint64_t seed, const double *G, int32_t R, double tol_reml, int32_t max_iter, double cg_tol, int32_t cg_max_iter,
                 double *tau, double *alpha, double *Py, double *gamma, double *ratios, double *trace, double *dbar_out, double *tau_path,
                 int32_t *iters, int32_t *state, int64_t *cg_iters, double *worst_residual)
{
    const char *who = "mih_lmm_null";
    if (c < 1 || probes < 1 || probes > 64 || 1 + c + probes > kPcaMaxBlock) {
        set_error("%s: needs c >= 1 covariates and 1 <= probes <= 64 with 1 + c + probes <= %d, got c = %d, probes = %d", who, kPcaMaxBlock, (int)c, (int)probes);
        return MIH_BAD_ARG;
    }
    if (R < 0 || R > kPcaMaxBlock || (R > 0 && !G)) { set_error("%s: R must be between 0 and %d with G given, got %d", who, kPcaMaxBlock, (int)R); return MIH_BAD_ARG; }
    if (!std::isfinite(tol_reml) || tol_reml < 0.0 || !std::isfinite(cg_tol) || cg_tol < 0.0) {
        set_error("%s: tol_reml and cg_tol must be finite and not negative, got %g and %g", who, tol_reml, cg_tol);
        return MIH_BAD_ARG;
    }
    if (max_iter < 1 || cg_max_iter < 1) { set_error("%s: max_iter and cg_max_iter must be at least 1, got %d and %d", who, (int)max_iter, (int)cg_max_iter); return MIH_BAD_ARG; }

    // the host's part of the start: the OLS residual e0 and s2 = e0'e0 / (n - c); Z must have full column rank
    const int w1 = 1 + c + probes, wz = 1 + c;
    std::vector<double> ztz((size_t)c * c), zinv((size_t)c * c), e0;
    double s2 = 0.0;
    if (h && y && Z && (R == 0 || G)) {
        const int64_t n = h->n;
        if (n <= c) { set_error("%s: %lld samples are too few for %d covariates", who, (long long)n, (int)c); return MIH_BAD_ARG; }
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(y[i])) { set_error("%s: y[%lld] is not finite", who, (long long)i); return MIH_BAD_ARG; }
        for (int64_t i = 0; i < n * c; ++i)
            if (!std::isfinite(Z[i])) { set_error("%s: Z has an entry that is not finite", who); return MIH_BAD_ARG; }
        for (int64_t i = 0; i < n * R; ++i)
            if (!std::isfinite(G[i])) { set_error("%s: G has an entry that is not finite", who); return MIH_BAD_ARG; }
        std::vector<double> zty((size_t)c, 0.0), b((size_t)c, 0.0);
        for (int a = 0; a < c; ++a) {
            for (int k = 0; k <= a; ++k) {
                double t = 0.0;
                for (int64_t i = 0; i < n; ++i) t += Z[(size_t)a * n + i] * Z[(size_t)k * n + i];
                ztz[(size_t)a * c + k] = ztz[(size_t)k * c + a] = t;
            }
            for (int64_t i = 0; i < n; ++i) zty[(size_t)a] += Z[(size_t)a * n + i] * y[i];
        }
        const int rank = lmm_spd_inverse(c, ztz.data(), zinv.data());
        if (rank < c) { set_error("%s: Z is rank-deficient: numerical rank %d of %d columns", who, rank, (int)c); return MIH_BAD_ARG; }
        for (int a = 0; a < c; ++a)
            for (int k = 0; k < c; ++k) b[(size_t)a] += zinv[(size_t)a * c + k] * zty[(size_t)k];
        e0.assign(y, y + n);
        for (int a = 0; a < c; ++a)
            for (int64_t i = 0; i < n; ++i) e0[(size_t)i] -= Z[(size_t)a * n + i] * b[(size_t)a];
        for (int64_t i = 0; i < n; ++i) s2 += e0[(size_t)i] * e0[(size_t)i];
        s2 /= (double)(n - c);
        if (!(s2 > 0.0)) { set_error("%s: y is a linear combination of the columns of Z: nothing to model", who); return MIH_BAD_ARG; }
    }

    LmmRun L;
    BlockOps ops;
    if (h) L.shape(h, std::max(w1, (int)R));
    const double extra = L.bytes() + 8.0 * (5.0 * (double)L.n_pad * L.bp + ((double)BlockOps::slabs(L.n_pad) + 3.0) * L.bp * L.bp);
    GrmRun g;
    MIH_TRY(grm_accumulate(who, h, col_keep, method, panel_cols, extra,
                           y && Z && tau && alpha && Py && gamma && (R == 0 || ratios) && trace && dbar_out && tau_path && iters && state && cg_iters && worst_residual, g));
    hipStream_t s = h->stream;
    MIH_TRY(grm_mirror(g, s));
    L.h = h; L.s = s; L.phi = g.acc.p;
    MIH_TRY(L.alloc());
    const int64_t n = L.n, n_pad = L.n_pad;
    const int bp = L.bp;
    MIH_TRY(ops.alloc(s, n_pad, bp));
    DevBuf<double> keep[5];
    for (auto &b : keep) MIH_TRY(b.alloc((size_t)n_pad * bp));
    double *rhs0 = keep[0].p, *phir = keep[1].p, *sblk = keep[2].p, *ps = keep[3].p, *pt = keep[4].p;
    const size_t colb = sizeof(double) * (size_t)n_pad;
    auto nbl = [](int w) { return (w + 15) / 16; };

    // d-bar = mean Phi_ii
    hipLaunchKernelGGL(k_lmm_diag, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, L.phi, n, n_pad, 0.0, 1.0, L.d.p);
    MIH_TRY(launch_failed("k_lmm_diag"));
    std::vector<double> diag((size_t)n);
    MIH_HIP(hipMemcpyAsync(diag.data(), L.d.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    double dbar = 0.0;
    for (int64_t i = 0; i < n; ++i) dbar += diag[(size_t)i];
    dbar /= (double)n;
    if (!std::isfinite(dbar) || !(dbar > 0.0)) { set_error("%s: the mean diagonal of the kinship matrix is %g: no genetic component to fit", who, dbar); return MIH_BAD_ARG; }

    // [y, Z, U] and Phi [y, Z, U], once
    MIH_HIP(hipMemsetAsync(rhs0, 0, colb * bp, s));
    MIH_HIP(hipMemcpy2DAsync(rhs0, colb, y, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, 1, hipMemcpyHostToDevice, s));
    MIH_HIP(hipMemcpy2DAsync(rhs0 + n_pad, colb, Z, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)c, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lmm_probes, dim3((unsigned)((n_pad + 255) / 256), (unsigned)probes), dim3(256), 0, s, rhs0 + (int64_t)wz * n_pad, n, n_pad, seed);
    MIH_TRY(launch_failed("k_lmm_probes"));
    MIH_TRY(L.vmul(rhs0, phir, nbl(w1), 0.0, 1.0));

    int64_t cg_total = 0;
    double worst = 0.0;
    std::vector<double> hres((size_t)bp), hbb((size_t)bp);
    std::vector<int32_t> hit((size_t)bp);
    // X = V^-1 (the w leading columns of src; nullptr: the right-hand sides are in place), and the tally of its iterations and
    // residuals
    auto solve = [&](const double *src, int w, const double *t) -> int {
        const int wp = (int)round_up(w, 16);
        if (src) MIH_HIP(hipMemcpyAsync(L.B(), src, colb * wp, hipMemcpyDeviceToDevice, s));
        MIH_TRY(L.solve(w, t[0], t[1], cg_tol, cg_max_iter));
        MIH_HIP(hipMemcpyAsync(hres.data(), L.sc.res, sizeof(double) * (size_t)w, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipMemcpyAsync(hbb.data(), L.sc.bb, sizeof(double) * (size_t)w, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipMemcpyAsync(hit.data(), L.sc.iters, sizeof(int32_t) * (size_t)w, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));
        int32_t most = 0;
        for (int k = 0; k < w; ++k) {
            most = std::max(most, hit[(size_t)k]);
            const double rel = hbb[(size_t)k] > 0.0 ? hres[(size_t)k] / std::sqrt(hbb[(size_t)k]) : 0.0;
            if (rel > worst || std::isnan(rel)) worst = rel;                 // (once a NaN, it stays)
        }
        cg_total += most;
        return MIH_OK;
    };
    // after a solve of [y, Z, ...] (w columns): S kept in sblk, Sigma = sym(Z'S_Z)^-1, alpha = Sigma Z'S_y, and
    // ps = S - S_Z Sigma (Z'S), all w columns
    std::vector<double> F, Sigma((size_t)c * c), SZ, hM, ha((size_t)c);
    auto project = [&](int w) -> int {
        const int wp = (int)round_up(w, 16);
        MIH_HIP(hipMemcpyAsync(sblk, L.X(), colb * wp, hipMemcpyDeviceToDevice, s));
        MIH_TRY(ops.gram(rhs0, L.X(), nbl(w), false, F));
        std::vector<double> H((size_t)c * c);
        for (int a = 0; a < c; ++a)
            for (int k = 0; k < c; ++k) H[(size_t)a * c + k] = 0.5 * (F[(size_t)(1 + a) * bp + 1 + k] + F[(size_t)(1 + k) * bp + 1 + a]);
        if (lmm_spd_inverse(c, H.data(), Sigma.data()) < c) { set_error("%s: Z'V^-1 Z is numerically singular", who); return MIH_BAD_ARG; }
        SZ.assign((size_t)c * w, 0.0);
        for (int a = 0; a < c; ++a)
            for (int col = 0; col < w; ++col) {
                double t = 0.0;
                for (int k = 0; k < c; ++k) t += Sigma[(size_t)a * c + k] * F[(size_t)(1 + k) * bp + col];
                SZ[(size_t)a * w + col] = t;
            }
        for (int a = 0; a < c; ++a) ha[(size_t)a] = SZ[(size_t)a * w];
        hM.assign((size_t)w * w, 0.0);
        for (int a = 0; a < w; ++a) hM[(size_t)a * w + a] = 1.0;
        for (int a = 0; a < c; ++a)
            for (int col = 0; col < w; ++col) hM[(size_t)(1 + a) * w + col] -= SZ[(size_t)a * w + col];
        return ops.rotate(L.X(), w, nullptr, 0, w, wp, hM, ps);
    };
    // pt = X - S_Z Sigma (Z'X) for the w leading columns of the solution X of another right-hand side
    auto project_other = [&](int w) -> int {
        const int wp = (int)round_up(w, 16);
        MIH_TRY(ops.gram(rhs0, L.X(), std::max(nbl(wz), nbl(w)), false, F));
        hM.assign((size_t)(w + wz) * w, 0.0);
        for (int a = 0; a < w; ++a) hM[(size_t)a * w + a] = 1.0;
        for (int a = 0; a < c; ++a)
            for (int col = 0; col < w; ++col) {
                double t = 0.0;
                for (int k = 0; k < c; ++k) t += Sigma[(size_t)a * c + k] * F[(size_t)(1 + k) * bp + col];
                hM[(size_t)(w + 1 + a) * w + col] = -t;
            }
        return ops.rotate(L.X(), w, sblk, wz, w, wp, hM, pt);
    };

    double t[2] = {s2 / 2.0, s2 / (2.0 * dbar)}, tr[2] = {0.0, 0.0};
    std::vector<double> path;
    path.push_back(t[0]); path.push_back(t[1]);
    int it = 0, st = 0;
    while (it < max_iter) {
        MIH_TRY(solve(rhs0, w1, t));
        MIH_TRY(project(w1));
        // the traces: t_e = mean u'Pu, t_g = mean (Phi u)'Pu, the probes in ascending order
        std::vector<double> D1, D2;
        MIH_TRY(ops.gram(rhs0, ps, nbl(w1), true, D1));
        MIH_TRY(ops.gram(phir, ps, nbl(w1), true, D2));
        tr[0] = tr[1] = 0.0;
        for (int k = wz; k < w1; ++k) { tr[0] += D1[(size_t)k * bp + k]; tr[1] += D2[(size_t)k * bp + k]; }
        tr[0] /= (double)probes; tr[1] /= (double)probes;
        // [a, Phi a] with a = Py, their solve and projection
        double *b2 = L.B(), *scratch = L.blk[4].p;
        MIH_HIP(hipMemsetAsync(b2, 0, colb * 16, s));
        MIH_HIP(hipMemcpyAsync(b2, ps, colb, hipMemcpyDeviceToDevice, s));
        MIH_TRY(L.vmul(b2, scratch, 1, 0.0, 1.0));
        MIH_HIP(hipMemcpyAsync(b2 + n_pad, scratch, colb, hipMemcpyDeviceToDevice, s));
        MIH_TRY(solve(nullptr, 2, t));
        MIH_TRY(project_other(2));
        std::vector<double> A1, A2;
        MIH_TRY(ops.gram(L.B(), L.B(), 1, false, A1));                                            // a'a, a'Phi a
        MIH_TRY(ops.gram(L.B(), pt, 1, false, A2));                                               // [a, Phi a]'[Pa, P Phi a]
        const double score[2] = {0.5 * (A1[0] - tr[0]), 0.5 * (A1[1] - tr[1])};
        const double AI[4] = {0.5 * A2[0], 0.5 * A2[1], 0.5 * A2[(size_t)bp], 0.5 * A2[(size_t)bp + 1]};
        double next[2];
        if (lmm_ai_step(t, score, AI, next) < 0) { set_error("%s: the average-information matrix of iteration %d has no finite inverse", who, it + 1); return MIH_BAD_ARG; }
        ++it;
        if (next[1] < 1e-8 * s2) {                                   // the boundary: the OLS fit in closed form
            st = 2; t[0] = s2; t[1] = 0.0;
            path.push_back(t[0]); path.push_back(t[1]);
            break;
        }
        const double change = lmm_rel_change(next, t);
        t[0] = next[0]; t[1] = next[1];
        path.push_back(t[0]); path.push_back(t[1]);
        if (change <= tol_reml) { st = 1; break; }
    }

    // the finish at the final tau: alpha and a = Py; then the variance ratios of the marker columns
    MIH_TRY(solve(rhs0, wz, t));
    MIH_TRY(project(wz));
    std::vector<double> hpy((size_t)n), rho((size_t)R);
    MIH_HIP(hipMemcpyAsync(hpy.data(), ps, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (R > 0) {
        const int rp = (int)round_up(R, 16);
        MIH_HIP(hipMemsetAsync(phir, 0, colb * rp, s));
        MIH_HIP(hipMemcpy2DAsync(phir, colb, G, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)R, hipMemcpyHostToDevice, s));
        MIH_TRY(solve(phir, R, t));
        MIH_TRY(project_other(R));
        std::vector<double> D;
        MIH_TRY(ops.gram(L.B(), pt, nbl(R), true, D));
        for (int j = 0; j < R; ++j) {                                // g~ = (I - Z (Z'Z)^-1 Z') g on the host: n R c operations
            const double *gj = G + (size_t)j * n;
            std::vector<double> ztg((size_t)c, 0.0), b((size_t)c, 0.0);
            for (int a = 0; a < c; ++a)
                for (int64_t i = 0; i < n; ++i) ztg[(size_t)a] += Z[(size_t)a * n + i] * gj[i];
            for (int a = 0; a < c; ++a)
                for (int k = 0; k < c; ++k) b[(size_t)a] += zinv[(size_t)a * c + k] * ztg[(size_t)k];
            double ss = 0.0;
            for (int64_t i = 0; i < n; ++i) {
                double v = gj[i];
                for (int a = 0; a < c; ++a) v -= Z[(size_t)a * n + i] * b[(size_t)a];
                ss += v * v;
            }
            rho[(size_t)j] = D[(size_t)j * bp + j] / ss;
        }
    }
    MIH_HIP(hipStreamSynchronize(s));

    double gm = 0.0;
    for (int j = 0; j < R; ++j) gm += rho[(size_t)j];
    *gamma = R > 0 ? gm / (double)R : std::nan("");
    std::copy(rho.begin(), rho.end(), ratios ? ratios : rho.data());
    tau[0] = t[0]; tau[1] = t[1];
    std::copy(ha.begin(), ha.end(), alpha);
    std::copy(hpy.begin(), hpy.end(), Py);
    trace[0] = tr[0]; trace[1] = tr[1];
    *dbar_out = dbar;
    std::copy(path.begin(), path.end(), tau_path);
    *iters = it; *state = st; *cg_iters = cg_total; *worst_residual = worst;
    return MIH_OK;
}

// -log10 p of z statistics by the tail function of the scans (normal_tail.h): what a caller that rescales z afterwards, as the
// mixed-model scan does with its variance ratio, recomputes the p-values with.  Host code.
int mih_neglog10p(const double *z, int64_t count, double *out)
{
    if (count < 0 || (count > 0 && (!z || !out))) { set_error("mih_neglog10p: null argument or a negative count"); return MIH_BAD_ARG; }
    for (int64_t i = 0; i < count; ++i) out[i] = neglog10p_of_z(z[i]);
    return MIH_OK;
}

}  // extern "C"
