// grm.hip -- the genetic relationship matrix of the samples of a genotype handle and the screen for related pairs
// (mih_grm, mih_grm_pairs): what SnpArrays.grm(x; method = :GRM / :Robust, minmaf) and the removal of every pair with
// Phi > 0.125 do between SnpArrays.filter and the principal components in manuscript/UKBB_metabolomic/data_process.jl:80-103
// (manuscript/NFBC_sim/NFBC_data_qc.jl:18-33 has GEMMA compute the same matrix) -- without the matrix leaving the device.
//
// The one product of the library that contracts over the SNP axis with an n x n result, so nothing of the X'r / X beta tile
// layout (M = SNP, K = sample) serves it: kept columns are decoded, a panel at a time, into f64 with the samples contiguous
// (K-major for a product over SNPs), and a symmetric rank-W update on the f64 matrix pipe adds the panel to an n_pad x n_pad
// accumulator of which only the lower-triangular 128 x 128 tiles exist.  Every Phi_ik is one chain of fused multiply-adds over
// the kept columns in ascending order, whatever the panel width: no atomics on the accumulator, no split over the columns.
#include "grm.h"
#include <algorithm>
#include <cmath>

namespace mih {

constexpr int kGrmKB = 8;                  // panel columns per LDS stage (two steps of the 16 x 16 x 4 instruction)
constexpr int kGrmLd = kGrmTile + 16;      // LDS row stride in doubles: the four panel columns a fragment load touches fall
                                           // into different halves of the 64 banks (144 mod 32 = 16)
constexpr int64_t kGrmPanelCols = 4096;    // the library's panel width: the accumulator's read-modify-write is 128 / 4096 = 3 %
                                           // of the operand traffic of a tile
constexpr int kGrmPairParts = 4;           // row ranges (waves) per strip of 64 columns in the pair scan

typedef double grm_v4d __attribute__((ext_vector_type(4)));

// workgroup b of a launch over the lower-triangular tile pairs: (ti, tk) with tk <= ti and b = ti (ti + 1) / 2 + tk
__device__ __forceinline__ void tri_decode(int64_t b, int64_t &ti, int64_t &tk)
{
    ti = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > b) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= b) ++ti;
    tk = b - ti * (ti + 1) / 2;
}

// ---- panel preparation -----------------------------------------------------------------------------------------------------------
// P[c * n_pad + i], c < Wp (a multiple of 4), i < n_pad: panel column c is kept column cols[c] for c < W, zeros for the pad
// columns and the pad rows.  Thread = one sample, so a wave stores 512 contiguous bytes; the 2-bit source is a sixteenth of
// that and four dwords serve a wave, so nothing is staged.
// 2-bit handles: the entry is (code - mu) [* sinv], the three values a column can take; a column without a finite mu (every
// genotype missing) is all zeros.  A missing entry is code 0 in the tiles: k_grm_panel_missing, queued behind, zeroes it.
__global__ void __launch_bounds__(256)
k_grm_panel_snp(const uint32_t *__restrict__ X, int64_t nbp, int64_t n, int64_t n_pad, int64_t nrb, const int64_t *__restrict__ cols,
                int64_t W, const double *__restrict__ mu, const double *__restrict__ sinv, int scaled, double *__restrict__ P)
{
    const int64_t c = blockIdx.x / nrb, i = (blockIdx.x % nrb) * 256 + threadIdx.x;
    if (i >= n_pad) return;
    double v = 0.0;
    if (c < W && i < n) {
        const int64_t j = cols[c];
        const double m = mu[j];
        if (isfinite(m)) {
            const uint32_t code = (X[xword(nbp, j, i >> 4)] >> (2 * (int)(i & 15))) & 3u;
            v = (double)code - m;
            if (scaled) v *= sinv[j];
        }
    }
    P[c * n_pad + i] = v;
}

// one wave per panel column over the column's missing list
__global__ void __launch_bounds__(64)
k_grm_panel_missing(const int64_t *__restrict__ miss_ptr, const int32_t *__restrict__ miss_row, const int64_t *__restrict__ cols,
                    int64_t n_pad, double *__restrict__ P)
{
    const int64_t c = blockIdx.x, j = cols[c];
    for (int64_t t = miss_ptr[j] + threadIdx.x, e = miss_ptr[j + 1]; t < e; t += 64) P[c * n_pad + miss_row[t]] = 0.0;
}

// 16-bit dosage handles: the entry of the standardized matrix (GRM), or the centred numerator (Robust: the divisor carries
// denom^2); missing entries are 0 in both
__global__ void __launch_bounds__(256)
k_grm_panel_dosage(DosageView dv, int64_t n, int64_t n_pad, int64_t nrb, const int64_t *__restrict__ cols, int64_t W, int scaled,
                   double *__restrict__ P)
{
    const int64_t c = blockIdx.x / nrb, i = (blockIdx.x % nrb) * 256 + threadIdx.x;
    if (i >= n_pad) return;
    double v = 0.0;
    if (c < W && i < n) {
        const int64_t j = cols[c];
        v = scaled ? dosage_x(dv, j, i) : dosage_c(dv.X[j * dv.ld + i], dv.mun[j]);
    }
    P[c * n_pad + i] = v;
}

// ---- symmetric rank-W update -----------------------------------------------------------------------------------------------------
// Acc[I + r, K + c] += sum_k P[k, I + r] P[k, K + c] for the tile pair (I, K) of the workgroup, K <= I; first: the tile starts
// from zero instead (the accumulator is never cleared, and tiles above the diagonal are never touched).  Both operand tiles
// of kGrmKB panel columns go through LDS, double-buffered, the next stage's global loads in flight during the current stage's
// arithmetic.  v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], one double each, and the results
// D[(l >> 4) + 4 reg][l & 15], reg = 0..3 -- the C/D map of this instruction alone.  A wave owns 4 x 4 such blocks.
// Wp is a multiple of 4; panel columns of a stage beyond Wp are neither loaded nor multiplied.  n_pad is a multiple of the
// tile, so every lane's rows exist.  Two workgroups per CU (176 registers, 36 KB of LDS): one computes while the other waits
// at its barrier.
__global__ void __launch_bounds__(256, 2)
k_grm_update(const double *__restrict__ P, int64_t n_pad, int64_t Wp, double *__restrict__ Acc, int first)
{
    __shared__ double sA[2][kGrmKB * kGrmLd], sB[2][kGrmKB * kGrmLd];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    int64_t ti, tk;
    tri_decode(blockIdx.x, ti, tk);
    const int64_t I = ti * kGrmTile, K = tk * kGrmTile;

    grm_v4d acc[4][4];
    double *C = Acc + (I + wr * 64 + (lane >> 4)) * n_pad + K + wc * 64 + (lane & 15);
    #pragma unroll
    for (int bi = 0; bi < 4; ++bi)
        #pragma unroll
        for (int bj = 0; bj < 4; ++bj)
            #pragma unroll
            for (int r = 0; r < 4; ++r) acc[bi][bj][r] = first ? 0.0 : C[(int64_t)(bi * 16 + 4 * r) * n_pad + bj * 16];

    // staging: element it * 256 + tid of the kGrmKB x 128 stage, panel column 2 it + (tid >> 7), sample tid & 127
    const int sk = tid >> 7, sr = tid & 127;
    double ra[4], rb[4];
    auto gload = [&](int64_t k0) {
        #pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int64_t k = k0 + 2 * it + sk;
            const bool in = k < Wp;
            ra[it] = in ? P[k * n_pad + I + sr] : 0.0;
            rb[it] = in ? P[k * n_pad + K + sr] : 0.0;
        }
    };
    auto sstore = [&](int buf) {
        #pragma unroll
        for (int it = 0; it < 4; ++it) {
            sA[buf][(2 * it + sk) * kGrmLd + sr] = ra[it];
            sB[buf][(2 * it + sk) * kGrmLd + sr] = rb[it];
        }
    };
    const int fa = (lane >> 4) * kGrmLd + wr * 64 + (lane & 15), fb = (lane >> 4) * kGrmLd + wc * 64 + (lane & 15);

    gload(0);
    sstore(0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = 0; k0 < Wp; k0 += kGrmKB, buf ^= 1) {
        const bool more = k0 + kGrmKB < Wp;
        if (more) gload(k0 + kGrmKB);
        const int steps = Wp - k0 >= kGrmKB ? kGrmKB / 4 : (int)((Wp - k0) / 4);
        for (int ks = 0; ks < steps; ++ks) {
            double a[4], b[4];
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = sA[buf][ks * 4 * kGrmLd + fa + q * 16];
                b[q] = sB[buf][ks * 4 * kGrmLd + fb + q * 16];
            }
            #pragma unroll
            for (int bi = 0; bi < 4; ++bi)
                #pragma unroll
                for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], b[bj], acc[bi][bj], 0, 0, 0);
        }
        if (more) sstore(buf ^ 1);
        __syncthreads();
    }

    #pragma unroll
    for (int bi = 0; bi < 4; ++bi)
        #pragma unroll
        for (int bj = 0; bj < 4; ++bj)
            #pragma unroll
            for (int r = 0; r < 4; ++r) C[(int64_t)(bi * 16 + 4 * r) * n_pad + bj * 16] = acc[bi][bj][r];
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------
// The whole matrix, in place: every entry of the lower triangle (diagonal included) divided by the divisor, every entry above
// it the copy of its mirror image -- inside a diagonal tile too, where the update has left numbers of its own above the
// diagonal: they are not read.  One workgroup per lower-triangular pair of 32 x 32 tiles, transposed through LDS.
__global__ void __launch_bounds__(256)
k_grm_mirror(double *__restrict__ Acc, int64_t n_pad, double div)
{
    __shared__ double t[32][33];
    int64_t ti, tk;
    tri_decode(blockIdx.x, ti, tk);
    const int64_t I = ti * 32, K = tk * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) t[r][tx] = Acc[(I + r) * n_pad + K + tx] / div;
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        if (ti == tk) {
            Acc[(I + r) * n_pad + I + tx] = r >= tx ? t[r][tx] : t[tx][r];
        } else {
            Acc[(I + r) * n_pad + K + tx] = t[r][tx];
            Acc[(K + r) * n_pad + I + tx] = t[tx][r];
        }
    }
}

__global__ void k_grm_diag(const double *__restrict__ Acc, int64_t n, int64_t n_pad, double div, double *__restrict__ diag)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) diag[i] = Acc[i * n_pad + i] / div;
}

// The pairs (i, k), i < k, with Phi_ik = Acc[k, i] / div > thr (strictly; a NaN is no pair), in the order (i, k).  A workgroup
// takes the strip of 64 columns i of the lower triangle, lane = column, and wave q the rows k of the q-th quarter of the
// samples, in ascending order: a wave reads 512 contiguous bytes per row.  off == nullptr: the pairs of (column i, quarter q)
// are counted into cnt[4 i + q].  Otherwise off[4 i + q] is where they start in the list -- the exclusive prefix sum of those
// counts, which is the order (i, k) -- and those that start below cap are written.  So the list needs no sort, a list that is
// cut at cap holds the first cap pairs, and a second call finds the same.
__global__ void __launch_bounds__(256)
k_grm_pairs(const double *__restrict__ Acc, int64_t n, int64_t n_pad, double div, double thr, const int64_t *__restrict__ off,
            int32_t *__restrict__ cnt, int64_t cap, int64_t *__restrict__ row_i, int64_t *__restrict__ row_k, double *__restrict__ phi)
{
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t i0 = blockIdx.x * 64ll, i = i0 + lane;
    const int64_t R = (n + kGrmPairParts - 1) / kGrmPairParts;
    const int64_t lo = max((int64_t)q * R, i0 + 1), hi = min(n, (int64_t)(q + 1) * R);
    const bool live = i < n;
    const int64_t base = off && live ? off[kGrmPairParts * i + q] : 0;
    int32_t c = 0;
    for (int64_t k = lo; k < hi; ++k) {
        if (!live || k <= i) continue;
        const double v = Acc[k * n_pad + i] / div;
        if (v > thr) {
            if (off && base + c < cap) { row_i[base + c] = i; row_k[base + c] = k; phi[base + c] = v; }
            ++c;
        }
    }
    if (!off && live) cnt[kGrmPairParts * i + q] = c;
}

int launch_failed(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MIH_OK;
    set_error("%s could not be launched: %s", what, hipGetErrorString(e));
    return MIH_HIP_ERROR;
}

int grm_accumulate(const char *who, const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double extra_bytes,
                   bool have_out, GrmRun &g)
{
    if (!h) { set_error("%s: null matrix handle", who); return MIH_BAD_ARG; }
    if (h->kind != 0 && !h->Du) { set_error("%s needs a 2-bit (SnpLinAlg) or a 16-bit dosage handle, not a dense matrix", who); return MIH_BAD_ARG; }
    if (method != 0 && method != 1) { set_error("%s: method must be 0 (GRM) or 1 (Robust), got %d", who, method); return MIH_BAD_ARG; }
    const int64_t n = h->n, p = h->p;
    std::vector<int64_t> kept;
    for (int64_t j = 0; j < p; ++j)
        if (!col_keep || col_keep[j]) kept.push_back(j);
    const int64_t m = (int64_t)kept.size();
    if (m == 0) { set_error("%s: the selection of columns is empty", who); return MIH_BAD_ARG; }
    const int64_t n_pad = h->kind == 0 ? h->n_pad : round_up(n, kGrmTile);
    int64_t W = panel_cols <= 0 ? kGrmPanelCols : round_up(panel_cols, 4);
    W = std::min(W, round_up(m, 4));
    const int64_t nt = n_pad / kGrmTile, nrb = (n_pad + 255) / 256;
    if ((double)nt * (double)(nt + 1) / 2.0 >= 2147483648.0 || (double)W * (double)nrb >= 2147483648.0) {
        set_error("%s: %lld samples in panels of %lld columns are too many tiles for one launch", who, (long long)n, (long long)W);
        return MIH_BAD_DIM;
    }

    // the memory rule: everything the call will hold, against what the device has free, before anything is allocated
    MIH_HIP(hipSetDevice(h->device));
    const double need = 8.0 * (double)n_pad * (double)n_pad + 8.0 * (double)n_pad * (double)W + 8.0 * (double)m + extra_bytes;
    size_t free_b = 0, total_b = 0;
    MIH_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > (double)free_b) {
        set_error("%s: the accumulator of %lld samples, a panel of %lld columns and the lists need %.0f bytes of device memory, %.0f bytes are free",
                  who, (long long)n, (long long)W, need, (double)free_b);
        return MIH_OOM;
    }
    if (!have_out) { set_error("%s: null argument", who); return MIH_BAD_ARG; }

    hipStream_t s = h->stream;
    std::vector<double> mu((size_t)p);
    MIH_HIP(hipMemcpyAsync(mu.data(), h->mu, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    if (method == 0) {
        g.div = 2.0 * (double)m;
    } else {                                                     // in ascending order of the columns, as the spec sums it
        double sum = 0.0;
        for (int64_t j : kept)
            if (std::isfinite(mu[(size_t)j])) sum += mu[(size_t)j] * (1.0 - mu[(size_t)j] / 2.0);
        g.div = 2.0 * sum;
        if (h->kind != 0) g.div *= (double)h->denom * (double)h->denom;       // the panel holds centred numerators
    }
    g.n = n; g.n_pad = n_pad; g.m = m;
    MIH_TRY(g.acc.alloc((size_t)n_pad * (size_t)n_pad));
    MIH_TRY(g.panel.alloc((size_t)n_pad * (size_t)W));
    MIH_TRY(g.cols.alloc((size_t)m));
    MIH_HIP(hipMemcpyAsync(g.cols.p, kept.data(), sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, s));

    for (int64_t a = 0; a < m; a += W) {
        const int64_t w = std::min(W, m - a), wp = round_up(w, 4);
        if (h->kind == 0) {
            hipLaunchKernelGGL(k_grm_panel_snp, dim3((unsigned)(wp * nrb)), dim3(256), 0, s, h->X, h->nbp, n, n_pad, nrb, g.cols.p + a, w, h->mu,
                               h->sinv, method == 0 ? 1 : 0, g.panel.p);
            if (h->total_missing > 0)
                hipLaunchKernelGGL(k_grm_panel_missing, dim3((unsigned)w), dim3(64), 0, s, h->miss_ptr, h->miss_row, g.cols.p + a, n_pad, g.panel.p);
        } else {
            hipLaunchKernelGGL(k_grm_panel_dosage, dim3((unsigned)(wp * nrb)), dim3(256), 0, s, dosage_view(h), n, n_pad, nrb, g.cols.p + a, w,
                               method == 0 ? 1 : 0, g.panel.p);
        }
        MIH_TRY(launch_failed("the panel kernel"));
        PassRecord rec;
        const bool timed = prof_begin(h, s, rec);
        hipLaunchKernelGGL(k_grm_update, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, g.panel.p, n_pad, wp, g.acc.p, a == 0 ? 1 : 0);
        if (timed) { snprintf(rec.kernel, sizeof(rec.kernel), "k_grm_update"); rec.residuals = (int)w; prof_end(h, s, rec); }
        MIH_TRY(launch_failed("k_grm_update"));
    }
    return MIH_OK;
}

int grm_mirror(GrmRun &g, hipStream_t s)
{
    const int64_t nt = g.n_pad / 32;
    hipLaunchKernelGGL(k_grm_mirror, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, g.acc.p, g.n_pad, g.div);
    return launch_failed("k_grm_mirror");
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_grm(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double *phi)
{
    GrmRun g;
    MIH_TRY(grm_accumulate("mih_grm", h, col_keep, method, panel_cols, 0.0, phi != nullptr, g));
    hipStream_t s = h->stream;
    MIH_TRY(grm_mirror(g, s));
    MIH_HIP(hipMemcpy2DAsync(phi, sizeof(double) * (size_t)g.n, g.acc.p, sizeof(double) * (size_t)g.n_pad, sizeof(double) * (size_t)g.n,
                             (size_t)g.n, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    return MIH_OK;
}

int mih_grm_pairs(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double threshold, int64_t cap,
                  int64_t *row_i, int64_t *row_k, double *phi, int64_t *count, double *diag)
{
    if (cap < 0) { set_error("mih_grm_pairs: cap must not be negative, got %lld", (long long)cap); return MIH_BAD_ARG; }
    if (std::isnan(threshold)) { set_error("mih_grm_pairs: the threshold is NaN"); return MIH_BAD_ARG; }
    const double n_d = h ? (double)h->n : 0.0;
    const double list = std::min((double)cap, n_d * (n_d - 1.0) / 2.0) * 24.0 + n_d * (kGrmPairParts * 12.0 + 8.0);
    GrmRun g;
    MIH_TRY(grm_accumulate("mih_grm_pairs", h, col_keep, method, panel_cols, list, count && (cap == 0 || (row_i && row_k && phi)), g));
    hipStream_t s = h->stream;
    const int64_t n = g.n;
    const unsigned strips = (unsigned)((n + 63) / 64);
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> off, li, lk;
    DevBuf<double> lphi, dg;
    MIH_TRY(cnt.alloc((size_t)(kGrmPairParts * n)));
    hipLaunchKernelGGL(k_grm_pairs, dim3(strips), dim3(256), 0, s, g.acc.p, n, g.n_pad, g.div, threshold, (const int64_t *)nullptr, cnt.p,
                       (int64_t)0, (int64_t *)nullptr, (int64_t *)nullptr, (double *)nullptr);
    MIH_TRY(launch_failed("k_grm_pairs"));
    if (diag) {
        MIH_TRY(dg.alloc((size_t)n));
        hipLaunchKernelGGL(k_grm_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g.acc.p, n, g.n_pad, g.div, dg.p);
        MIH_HIP(hipMemcpyAsync(diag, dg.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    }
    std::vector<int32_t> hcnt((size_t)(kGrmPairParts * n));
    MIH_HIP(hipMemcpyAsync(hcnt.data(), cnt.p, sizeof(int32_t) * hcnt.size(), hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    std::vector<int64_t> hoff(hcnt.size());
    int64_t total = 0;
    for (size_t t = 0; t < hcnt.size(); ++t) { hoff[t] = total; total += hcnt[t]; }
    const int64_t take = std::min(cap, total);
    if (take > 0) {
        MIH_TRY(off.alloc(hoff.size()));
        MIH_TRY(li.alloc((size_t)take));
        MIH_TRY(lk.alloc((size_t)take));
        MIH_TRY(lphi.alloc((size_t)take));
        MIH_HIP(hipMemcpyAsync(off.p, hoff.data(), sizeof(int64_t) * hoff.size(), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_grm_pairs, dim3(strips), dim3(256), 0, s, g.acc.p, n, g.n_pad, g.div, threshold, off.p, (int32_t *)nullptr, take,
                           li.p, lk.p, lphi.p);
        MIH_TRY(launch_failed("k_grm_pairs"));
        MIH_HIP(hipMemcpyAsync(row_i, li.p, sizeof(int64_t) * (size_t)take, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipMemcpyAsync(row_k, lk.p, sizeof(int64_t) * (size_t)take, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipMemcpyAsync(phi, lphi.p, sizeof(double) * (size_t)take, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));
    }
    *count = total;
    return MIH_OK;
}

}  // extern "C"
