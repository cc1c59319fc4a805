// grm_block.h -- what pca.hip and lmm.hip share: the walk of a product Phi Q of the resident kinship matrix with a block of at
// most 128 columns on the f64 matrix cores, the block Gram products A'B, the thin rotations, and their launches (BlockOps).
// The blocks are kept in the panel layout of grm.hip, B[c * n_pad + i], column c, sample i, the columns rounded up to 16, the
// columns beyond the live ones and the rows beyond n all zeros.  The kernels that are no templates are static: each of the
// two translation units has its own copy.
#pragma once
#include "grm.h"
#include <vector>

namespace mih {

constexpr int kPcaMaxBlock = 128;
constexpr int kPcaGramRows = 512;          // rows of a slab of the Gram kernels: one wave, 16 steps of 32 rows
constexpr int kPcaRotCols = 8;             // output columns per thread of the thin rotation

typedef double pca_v4d __attribute__((ext_vector_type(4)));

// v_mfma_f64_16x16x4_f64 computes D[m][n] += sum_k A[m][k] B[k][n]; lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and
// D[(l >> 4) + 4 reg][l & 15] (grm.hip).  Here m is a column c of the block, n a sample i and k a sample j of the contraction:
//     A[c][j] = Q[c * n_pad + j],   B[j][i] = Phi[j][i] = Phi[i][j] (symmetric bit for bit: read along row i),
//     D[c][i] = (Phi Q)[c * n_pad + i]: a quarter-wave holds 16 consecutive samples of one column.
// A wave owns IB blocks of 16 samples i, from i0, and all NB blocks of 16 columns, and walks j over the whole of n_pad in steps
// of 32: lane (r = l & 15, q = l >> 4) reads the 8 consecutive doubles j0 + 8 q .. + 7 of row i0 + r of Phi and of column
// c0 + r of Q -- 64 contiguous bytes each, a quarter-wave's 256 -- and feeds them to 8 instructions, s = 0..7, whose k-slot q
// carries j = j0 + 8 q + s.  Which j rides in which slot is the same for A and B, so the product is the plain one, and the
// order of the sum of an entry is fixed by n_pad alone: it depends on neither IB nor NB, nor on the other columns of the block.
// The next step's fragments are loaded before the current step's arithmetic.  nb <= NB blocks of columns are live; the rest is
// not read, and its accumulators stay zero.  On return acc[ib][cb][reg] = (Phi Q)[(cb * 16 + q + 4 reg) * n_pad + i0 + ib * 16 + r].
template <int IB, int NB>
__device__ __forceinline__ void
grm_block_walk(const double *__restrict__ Phi, const double *__restrict__ Q, int64_t n_pad, int nb, int64_t i0, pca_v4d (&acc)[IB][NB])
{
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const double *pb = Phi + (i0 + r) * n_pad + 8 * q;
    const double *pa = Q + (int64_t)r * n_pad + 8 * q;

    #pragma unroll
    for (int ib = 0; ib < IB; ++ib)
        #pragma unroll
        for (int cb = 0; cb < NB; ++cb) acc[ib][cb] = pca_v4d{0.0, 0.0, 0.0, 0.0};

    pca_v4d fb[2][IB][2], fa[2][NB][2];
    auto load = [&](int buf, int64_t j0) {
        #pragma unroll
        for (int ib = 0; ib < IB; ++ib) {
            const pca_v4d *p = reinterpret_cast<const pca_v4d *>(pb + (int64_t)ib * 16 * n_pad + j0);
            fb[buf][ib][0] = p[0];
            fb[buf][ib][1] = p[1];
        }
        #pragma unroll
        for (int cb = 0; cb < NB; ++cb)
            if (cb < nb) {
                const pca_v4d *p = reinterpret_cast<const pca_v4d *>(pa + (int64_t)cb * 16 * n_pad + j0);
                fa[buf][cb][0] = p[0];
                fa[buf][cb][1] = p[1];
            }
    };
    auto mult = [&](int buf) {
        #pragma unroll
        for (int s = 0; s < 8; ++s)
            #pragma unroll
            for (int ib = 0; ib < IB; ++ib)
                #pragma unroll
                for (int cb = 0; cb < NB; ++cb)
                    if (cb < nb)
                        acc[ib][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[buf][cb][s >> 2][s & 3], fb[buf][ib][s >> 2][s & 3], acc[ib][cb], 0, 0, 0);
    };

    load(0, 0);
    for (int64_t j0 = 0; j0 < n_pad; j0 += 64) {               // n_pad is a multiple of 128: two steps per trip, the buffers by name
        load(1, j0 + 32);
        mult(0);
        if (j0 + 64 < n_pad) load(0, j0 + 64);
        mult(1);
    }
}

// ---- the block Gram products A'B -------------------------------------------------------------------------------------------------
// part[slab][a][c] = sum over the slab's rows i of A[a * n_pad + i] B[c * n_pad + i], a and c below 16 nb; slab = kPcaGramRows
// rows, cut at n_pad.  One wave per (slab, block of 16 a), every block of 16 c: m = a, n = c, k = i, both fragments read like
// the A side of k_pca_spmm.  diag: only the block c = a is computed (the residual norms are a diagonal), the others are
// neither computed nor read by k_pca_gram_sum.  The slabs are summed in ascending order by k_pca_gram_sum, one thread per entry:
// G is bp x bp row-major, G[a * bp + c].
static __global__ void __launch_bounds__(64)
k_pca_gram(const double *__restrict__ A, const double *__restrict__ B, int64_t n_pad, int nb, int bp, int diag, double *__restrict__ part)
{
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4, ab = blockIdx.y;
    const int64_t lo = (int64_t)blockIdx.x * kPcaGramRows, hi = min(lo + (int64_t)kPcaGramRows, n_pad);
    const double *pa = A + (int64_t)(ab * 16 + r) * n_pad + 8 * q;
    const double *pb = B + (int64_t)r * n_pad + 8 * q;
    pca_v4d acc[kPcaMaxBlock / 16];
    #pragma unroll
    for (int cb = 0; cb < kPcaMaxBlock / 16; ++cb) acc[cb] = pca_v4d{0.0, 0.0, 0.0, 0.0};
    for (int64_t i = lo; i < hi; i += 32) {
        const pca_v4d *p = reinterpret_cast<const pca_v4d *>(pa + i);
        const pca_v4d a0 = p[0], a1 = p[1];
        #pragma unroll
        for (int cb = 0; cb < kPcaMaxBlock / 16; ++cb)
            if (cb < nb && (!diag || cb == ab)) {
                const pca_v4d *pq = reinterpret_cast<const pca_v4d *>(pb + (int64_t)cb * 16 * n_pad + i);
                const pca_v4d b0 = pq[0], b1 = pq[1];
                #pragma unroll
                for (int s = 0; s < 4; ++s) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], b0[s], acc[cb], 0, 0, 0);
                #pragma unroll
                for (int s = 0; s < 4; ++s) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], b1[s], acc[cb], 0, 0, 0);
            }
    }
    double *out = part + (int64_t)blockIdx.x * bp * bp;
    #pragma unroll
    for (int cb = 0; cb < kPcaMaxBlock / 16; ++cb)
        if (cb < nb && (!diag || cb == ab))
            #pragma unroll
            for (int reg = 0; reg < 4; ++reg) out[(int64_t)(ab * 16 + q + 4 * reg) * bp + cb * 16 + r] = acc[cb][reg];
}

static __global__ void __launch_bounds__(256)
k_pca_gram_sum(const double *__restrict__ part, int64_t nslab, int nb, int bp, int diag, double *__restrict__ G)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= bp * bp) return;
    const int a = e / bp, c = e % bp;
    double sum = 0.0;
    if (a < 16 * nb && c < 16 * nb && (!diag || a / 16 == c / 16))
        for (int64_t s = 0; s < nslab; ++s) sum += part[s * bp * bp + e];
    G[e] = sum;
}

// ---- the thin rotation -----------------------------------------------------------------------------------------------------------
// Out[:, c] = sum_{a < r1} In1[:, a] M1[a * ldm + c] (+ sum_{a < r2} In2[:, a] M2[a * ldm + c]) for c < kout, zeros for
// kout <= c < kwrite; a ascending, In1 before In2, one fused multiply-add each.  Thread = one sample and kPcaRotCols columns;
// the entries of M are the same for a whole wave (scalar loads).  Out is neither In1 nor In2.
static __global__ void __launch_bounds__(256)
k_pca_rotate(const double *__restrict__ In1, const double *__restrict__ M1, int r1, const double *__restrict__ In2,
             const double *__restrict__ M2, int r2, int ldm, int64_t n_pad, int kout, int kwrite, double *__restrict__ Out)
{
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    const int c0 = blockIdx.y * kPcaRotCols;
    if (i >= n_pad) return;
    double acc[kPcaRotCols];
    #pragma unroll
    for (int t = 0; t < kPcaRotCols; ++t) acc[t] = 0.0;
    if (c0 < kout) {
        for (int a = 0; a < r1; ++a) {
            const double x = In1[(int64_t)a * n_pad + i];
            #pragma unroll
            for (int t = 0; t < kPcaRotCols; ++t) acc[t] = fma(x, M1[a * ldm + c0 + t], acc[t]);
        }
        for (int a = 0; a < r2; ++a) {
            const double x = In2[(int64_t)a * n_pad + i];
            #pragma unroll
            for (int t = 0; t < kPcaRotCols; ++t) acc[t] = fma(x, M2[a * ldm + c0 + t], acc[t]);
        }
    }
    #pragma unroll
    for (int t = 0; t < kPcaRotCols; ++t)
        if (c0 + t < kwrite) Out[(int64_t)(c0 + t) * n_pad + i] = c0 + t < kout ? acc[t] : 0.0;
}

// The scratch of the block Gram products and thin rotations of one call, and their launches.
struct BlockOps {
    hipStream_t s = nullptr;
    int64_t n_pad = 0, nslab = 0;
    int bp = 0;
    DevBuf<double> part, G, M;                                    // M: two bp x bp matrices

    static int64_t slabs(int64_t n_pad) { return (n_pad + kPcaGramRows - 1) / kPcaGramRows; }
    int alloc(hipStream_t stream, int64_t np, int width)
    {
        s = stream; n_pad = np; bp = width; nslab = slabs(np);
        MIH_TRY(part.alloc((size_t)nslab * bp * bp));
        MIH_TRY(G.alloc((size_t)bp * bp));
        return M.alloc((size_t)2 * bp * bp);
    }

    // full (bp x bp, row-major) = A'B over the leading nbl blocks of 16 columns of both; diag: only the diagonal blocks
    int gram(const double *A, const double *B, int nbl, bool diag, std::vector<double> &full)
    {
        hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)nslab, (unsigned)nbl), dim3(64), 0, s, A, B, n_pad, nbl, bp, diag ? 1 : 0, part.p);
        MIH_TRY(launch_failed("k_pca_gram"));
        hipLaunchKernelGGL(k_pca_gram_sum, dim3((unsigned)((bp * bp + 255) / 256)), dim3(256), 0, s, part.p, nslab, nbl, bp, diag ? 1 : 0, G.p);
        MIH_TRY(launch_failed("k_pca_gram_sum"));
        full.resize((size_t)bp * bp);
        MIH_HIP(hipMemcpyAsync(full.data(), G.p, sizeof(double) * full.size(), hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));
        return MIH_OK;
    }

    // Out = In1 M1 (+ In2 M2), kwrite columns of Out written (zeros from kout on): hM holds M1 (r1 x kout) then M2 (r2 x kout),
    // row-major with the stride kout
    int rotate(const double *In1, int r1, const double *In2, int r2, int kout, int kwrite, const std::vector<double> &hM, double *Out)
    {
        const int ldm = bp;
        std::vector<double> m((size_t)2 * bp * bp, 0.0);
        for (int a = 0; a < r1; ++a)
            for (int c = 0; c < kout; ++c) m[(size_t)a * ldm + c] = hM[(size_t)a * kout + c];
        for (int a = 0; a < r2; ++a)
            for (int c = 0; c < kout; ++c) m[(size_t)bp * bp + (size_t)a * ldm + c] = hM[(size_t)(r1 + a) * kout + c];
        MIH_HIP(hipMemcpyAsync(M.p, m.data(), sizeof(double) * m.size(), hipMemcpyHostToDevice, s));
        MIH_HIP(hipStreamSynchronize(s));                         // m leaves scope
        hipLaunchKernelGGL(k_pca_rotate, dim3((unsigned)((n_pad + 255) / 256), (unsigned)((kwrite + kPcaRotCols - 1) / kPcaRotCols)), dim3(256), 0, s, In1,
                           (const double *)M.p, r1, In2, (const double *)(M.p + (size_t)bp * bp), r2, ldm, n_pad, kout, kwrite, Out);
        return launch_failed("k_pca_rotate");
    }
};

}  // namespace mih
