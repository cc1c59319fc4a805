// pca.hip -- the k leading eigenpairs of the kinship matrix of a genotype handle (mih_grm_eig): the principal components that
// manuscript/UKBB_metabolomic/data_process.jl:103-110 hands to the fit as covariates, after grm and the related-pair screen of
// grm.hip -- without Phi leaving the device.  The components of the standardised genotype matrix are the leading eigenvectors
// of exactly that Phi (what PLINK and GCTA compute).
//
// Phi is built by grm_accumulate and mirrored into a full symmetric n_pad x n_pad matrix that stays in device memory for the
// call; a blocked subspace iteration extracts the pairs (tests/pca_spec.py states it in numpy):
//     Q (n_pad x b_l, a hashed start) <- orth(orth(Q));
//     repeat  Y = Phi Q;  T = sym(Q'Y) = S Theta S' on the host;  rho_i = |Y s_i - theta_i Q s_i|, i < k;
//             stop when max rho <= tol theta_1 or at max_iter;  else Q <- orth(orth(Y))
//     orth(Y): G = Y'Y = W D W' on the host, directions with d_i <= 2^-52 d_1 dropped for good, Q = Y W D^(-1/2)
//     U = Q S[:, :k], the sign rule, home.
// Everything n-sized is a kernel here, all f64, no atomics, every sum in an order the shapes alone fix: the same arguments give
// the same bits.  The b_l x b_l algebra (b_l <= 128) is the host's: sym_eig.h.
//
// Blocks are kept in the panel layout of grm.hip, B[c * n_pad + i], column c, sample i: bp = b_l rounded up to 16 columns, the
// columns beyond the live ones and the rows beyond n all zeros -- every kernel that writes a block writes them.
#include "grm_block.h"
#include "sym_eig.h"
#include <algorithm>
#include <cmath>

namespace mih {

constexpr int kPcaMaxK = 64;

// ---- the start block -------------------------------------------------------------------------------------------------------------
// Q[c * n_pad + i] = ((z >> 12) + 1/2) 2^-51 - 1 in (-1, 1), z the output function of splitmix64 at seed + golden (128 i + c + 1):
// a counter-based hash, so an entry depends on (seed, i, c) alone.  Rows >= n and columns >= bl are zeros.
__global__ void __launch_bounds__(256)
k_pca_start(double *__restrict__ Q, int64_t n, int64_t n_pad, int bl, uint64_t seed)
{
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= n_pad) return;
    double v = 0.0;
    if (i < n && c < bl) {
        uint64_t z = seed + 0x9E3779B97F4A7C15ull * (128ull * (uint64_t)i + (uint64_t)c + 1ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        v = ((double)(z >> 12) + 0.5) * 0x1p-51 - 1.0;
    }
    Q[(int64_t)c * n_pad + i] = v;
}

// ---- Y = Phi Q -------------------------------------------------------------------------------------------------------------------
// The walk over j on the f64 matrix cores is grm_block_walk (grm_block.h states the layout and the order of the sums), which
// lmm.hip shares.  No LDS, no barrier: one wave per workgroup, so that the n_pad / (16 IB) waves spread over the CUs evenly.
// Phi is read once per product; Q (L2-resident) NB / IB times as many bytes.  A quarter-wave stores 16 consecutive samples of
// one column.
template <int IB, int NB>
__global__ void __launch_bounds__(64)
k_pca_spmm(const double *__restrict__ Phi, const double *__restrict__ Q, int64_t n_pad, int nb, double *__restrict__ Y)
{
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * (16 * IB);
    pca_v4d acc[IB][NB];
    grm_block_walk<IB, NB>(Phi, Q, n_pad, nb, i0, acc);

    #pragma unroll
    for (int ib = 0; ib < IB; ++ib)
        #pragma unroll
        for (int cb = 0; cb < NB; ++cb)
            if (cb < nb)
                #pragma unroll
                for (int reg = 0; reg < 4; ++reg) Y[(int64_t)(cb * 16 + q + 4 * reg) * n_pad + i0 + ib * 16 + r] = acc[ib][cb][reg];
}

// ---- sign and norm ---------------------------------------------------------------------------------------------------------------
// One workgroup per column of U: the entry of largest magnitude (the lowest index on a tie) and the sum of squares, thread t
// over the samples t, t + 256, ... and then a tree over the 256 threads -- an order the shapes fix; then every entry divided by
// the norm, negated if that entry was negative.
__global__ void __launch_bounds__(256)
k_pca_sign_norm(double *__restrict__ Uc, int64_t n, int64_t n_pad)
{
    __shared__ double s_abs[256], s_val[256], s_sq[256];
    __shared__ int64_t s_idx[256];
    double *u = Uc + (int64_t)blockIdx.x * n_pad;
    const int t = threadIdx.x;
    double ab = -1.0, val = 0.0, sq = 0.0;
    int64_t ib = 0;
    for (int64_t i = t; i < n; i += 256) {
        const double x = u[i];
        sq = fma(x, x, sq);
        if (sign_rule_better(fabs(x), i, ab, ib)) { ab = fabs(x); ib = i; val = x; }
    }
    s_abs[t] = ab; s_val[t] = val; s_sq[t] = sq; s_idx[t] = ib;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            s_sq[t] += s_sq[t + w];
            if (sign_rule_better(s_abs[t + w], s_idx[t + w], s_abs[t], s_idx[t])) { s_abs[t] = s_abs[t + w]; s_idx[t] = s_idx[t + w]; s_val[t] = s_val[t + w]; }
        }
        __syncthreads();
    }
    const double norm = sqrt(s_sq[0]);
    if (!(norm > 0.0)) return;
    const bool flip = s_val[0] < 0.0;
    for (int64_t i = t; i < n; i += 256) {
        const double x = u[i] / norm;
        u[i] = flip ? -x : x;
    }
}

// The blocks and scratch of one call, and the steps of the iteration over them.
struct PcaRun {
    const mih_mat *h = nullptr;
    hipStream_t s = nullptr;
    const double *phi = nullptr;
    int64_t n = 0, n_pad = 0, nslab = 0;
    int bl = 0, bp = 0, r = 0;                                    // the logical block, its padded width, the live directions
    DevBuf<double> blk[3];
    BlockOps ops;                                                 // the Gram products and rotations (grm_block.h)
    std::vector<double> hG, hW, hd, hM;

    int nb() const { return (r + 15) / 16; }

    // hG (r x r, row-major) = sym(A'B) of the live columns; diag: only the diagonal is meaningful
    int gram(const double *A, const double *B, int cols, bool diag)
    {
        std::vector<double> full;
        MIH_TRY(ops.gram(A, B, (cols + 15) / 16, diag, full));
        hG.assign((size_t)cols * cols, 0.0);
        for (int a = 0; a < cols; ++a)
            for (int c = 0; c < cols; ++c) hG[(size_t)a * cols + c] = 0.5 * (full[(size_t)a * bp + c] + full[(size_t)c * bp + a]);
        return MIH_OK;
    }

    // Out = In1 M1 (+ In2 M2), all bp columns of Out written: hM holds M1 (r1 x kout) then M2 (r2 x kout), row-major with the
    // stride kout
    int rotate(const double *In1, int r1, const double *In2, int r2, int kout, double *Out) { return ops.rotate(In1, r1, In2, r2, kout, bp, hM, Out); }

    // Out = orth(In): the live directions r shrink to the numerical rank of In
    int orth(const double *In, double *Out)
    {
        if (r < 1) return MIH_OK;
        MIH_TRY(gram(In, In, r, false));
        hd.assign((size_t)r, 0.0);
        hW.assign((size_t)r * r, 0.0);
        sym_eig_jacobi(r, hG.data(), hd.data(), hW.data());
        const int keep = sym_eig_rank(r, hd.data());
        hM.assign((size_t)r * std::max(keep, 1), 0.0);
        for (int a = 0; a < r; ++a)
            for (int c = 0; c < keep; ++c) hM[(size_t)a * keep + c] = hW[(size_t)a * r + c] / std::sqrt(hd[(size_t)c]);
        MIH_TRY(rotate(In, r, nullptr, 0, keep, Out));
        r = keep;
        return MIH_OK;
    }

    int product(const double *Q, double *Y)
    {
        PassRecord rec;
        const bool timed = prof_begin(h, s, rec);
        const int nbl = nb();
        if (nbl <= 2) hipLaunchKernelGGL((k_pca_spmm<4, 2>), dim3((unsigned)(n_pad / 64)), dim3(64), 0, s, phi, Q, n_pad, nbl, Y);
        else if (nbl <= 4) hipLaunchKernelGGL((k_pca_spmm<2, 4>), dim3((unsigned)(n_pad / 32)), dim3(64), 0, s, phi, Q, n_pad, nbl, Y);
        else hipLaunchKernelGGL((k_pca_spmm<1, 8>), dim3((unsigned)(n_pad / 16)), dim3(64), 0, s, phi, Q, n_pad, nbl, Y);
        if (timed) { snprintf(rec.kernel, sizeof(rec.kernel), "k_pca_spmm"); rec.residuals = r; prof_end(h, s, rec); }
        return launch_failed("k_pca_spmm");
    }
};

}  // namespace mih

using namespace mih;

extern "C" {

int mih_grm_eig(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, int32_t k, int32_t block, double tol,
                int32_t max_iter, uint64_t seed, double *values, double *vectors, double *residuals, int32_t *iters, int32_t *converged)
{
    const char *who = "mih_grm_eig";
    if (k < 1 || k > kPcaMaxK || (h && (int64_t)k > h->n)) {
        set_error("%s: k must be between 1 and min(n, %d), got %d", who, kPcaMaxK, (int)k);
        return MIH_BAD_ARG;
    }
    if (block != 0 && (block < k || block > kPcaMaxBlock)) {
        set_error("%s: block must be 0 (the library's rule) or between k = %d and %d, got %d", who, (int)k, kPcaMaxBlock, (int)block);
        return MIH_BAD_ARG;
    }
    if (!std::isfinite(tol) || tol < 0.0) { set_error("%s: tol must be finite and not negative, got %g", who, tol); return MIH_BAD_ARG; }
    if (max_iter < 1) { set_error("%s: max_iter must be at least 1, got %d", who, (int)max_iter); return MIH_BAD_ARG; }

    PcaRun p;
    const int b = block ? block : (int)round_up(std::max(2 * k, k + 8), 16);
    if (h) {
        p.n = h->n;
        p.n_pad = h->kind == 0 ? h->n_pad : round_up(h->n, kGrmTile);
        p.bl = (int)std::min<int64_t>(b, p.n);
        p.bp = (int)round_up(p.bl, 16);
        p.nslab = BlockOps::slabs(p.n_pad);
    }
    const double extra = 8.0 * (3.0 * (double)p.n_pad * p.bp + ((double)p.nslab + 3.0) * p.bp * p.bp);
    GrmRun g;
    MIH_TRY(grm_accumulate(who, h, col_keep, method, panel_cols, extra, values && vectors && residuals && iters && converged, g));
    hipStream_t s = h->stream;
    MIH_TRY(grm_mirror(g, s));

    p.h = h; p.s = s; p.phi = g.acc.p;
    const int64_t n = p.n, n_pad = p.n_pad;
    const int bp = p.bp;
    for (auto &blk : p.blk) MIH_TRY(blk.alloc((size_t)n_pad * bp));
    MIH_TRY(p.ops.alloc(s, n_pad, bp));
    double *Q = p.blk[0].p, *Y = p.blk[1].p, *Z = p.blk[2].p;

    hipLaunchKernelGGL(k_pca_start, dim3((unsigned)((n_pad + 255) / 256), (unsigned)bp), dim3(256), 0, s, Q, n, n_pad, p.bl, seed);
    MIH_TRY(launch_failed("k_pca_start"));
    p.r = p.bl;
    MIH_TRY(p.orth(Q, Z));
    MIH_TRY(p.orth(Z, Q));

    std::vector<double> theta, S, res((size_t)k, 0.0), Sk;
    int it = 0;
    bool done = false;
    for (;;) {
        if (p.r < k) {
            set_error("%s: the matrix has numerical rank %d, below k = %d", who, p.r, (int)k);
            return MIH_BAD_ARG;
        }
        const int r = p.r;
        MIH_TRY(p.product(Q, Y));
        MIH_TRY(p.gram(Q, Y, r, false));
        theta.assign((size_t)r, 0.0);
        S.assign((size_t)r * r, 0.0);
        sym_eig_jacobi(r, p.hG.data(), theta.data(), S.data());
        // R = Y S_k - Q (S_k Theta_k), then the norms of its columns
        p.hM.assign((size_t)2 * r * k, 0.0);
        for (int a = 0; a < r; ++a)
            for (int c = 0; c < k; ++c) {
                p.hM[(size_t)a * k + c] = S[(size_t)a * r + c];
                p.hM[(size_t)(r + a) * k + c] = -(S[(size_t)a * r + c] * theta[(size_t)c]);
            }
        MIH_TRY(p.rotate(Y, r, Q, r, k, Z));
        MIH_TRY(p.gram(Z, Z, k, true));
        double worst = 0.0;
        for (int c = 0; c < k; ++c) {
            res[(size_t)c] = std::sqrt(p.hG[(size_t)c * k + c]);
            if (!(res[(size_t)c] <= worst)) worst = res[(size_t)c];          // (a NaN is the worst)
        }
        ++it;
        done = worst <= tol * theta[0];
        if (done || it >= max_iter) break;
        MIH_TRY(p.orth(Y, Z));
        MIH_TRY(p.orth(Z, Q));
    }

    // U = Q S_k, the sign rule, rows < n home
    const int r = p.r;
    p.hM.assign((size_t)r * k, 0.0);
    for (int a = 0; a < r; ++a)
        for (int c = 0; c < k; ++c) p.hM[(size_t)a * k + c] = S[(size_t)a * r + c];
    MIH_TRY(p.rotate(Q, r, nullptr, 0, k, Z));
    hipLaunchKernelGGL(k_pca_sign_norm, dim3((unsigned)k), dim3(256), 0, s, Z, n, n_pad);
    MIH_TRY(launch_failed("k_pca_sign_norm"));
    std::vector<double> U((size_t)n * k);
    MIH_HIP(hipMemcpy2DAsync(U.data(), sizeof(double) * (size_t)n, Z, sizeof(double) * (size_t)n_pad, sizeof(double) * (size_t)n, (size_t)k,
                             hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    std::copy(U.begin(), U.end(), vectors);
    for (int c = 0; c < k; ++c) { values[c] = theta[(size_t)c]; residuals[c] = res[(size_t)c]; }
    *iters = it;
    *converged = done ? 1 : 0;
    return MIH_OK;
}

}  // extern "C"
