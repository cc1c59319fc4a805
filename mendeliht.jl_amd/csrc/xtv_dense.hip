// xtv_dense.hip -- out = X' r over a dense f64 / f32 design matrix and over the 16-bit dosage image
#include "common.h"

namespace mih {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- dense design matrix: out_j = sum_i D[i,j] r_i (one wave per column) ---------------
__device__ __forceinline__ double wave_sum(double v)
{
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

typedef double f64x2 __attribute__((ext_vector_type(2)));
// One wave per column.  The matrix is read exactly once: nontemporal 16 B/lane loads, four of them in
// flight per lane (64 lanes x 64 B = 4 KB per wave-iteration), two accumulators per load slot; the
// fixed lane -> row mapping and the fixed final tree keep the sum bit-reproducible.
__global__ void __launch_bounds__(256)
k_xtv_dense(const double *__restrict__ D, int64_t n, int64_t p, const double *__restrict__ r,
            double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    int64_t j = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (j >= p) return;
    const double *col = D + j * n;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if ((n & 1) == 0 && (((uintptr_t)col) & 15) == 0) {
        const f64x2 *cx = reinterpret_cast<const f64x2 *>(col);
        const f64x2 *rx = reinterpret_cast<const f64x2 *>(r);
        const int64_t n2 = n >> 1;
        int64_t i = lane;
        for (; i + 192 < n2; i += 256) {
            f64x2 x0 = __builtin_nontemporal_load(cx + i), x1 = __builtin_nontemporal_load(cx + i + 64);
            f64x2 x2 = __builtin_nontemporal_load(cx + i + 128), x3 = __builtin_nontemporal_load(cx + i + 192);
            f64x2 v0 = rx[i], v1 = rx[i + 64], v2 = rx[i + 128], v3 = rx[i + 192];
            a[0] = fma(x0.x, v0.x, a[0]); a[1] = fma(x0.y, v0.y, a[1]);
            a[2] = fma(x1.x, v1.x, a[2]); a[3] = fma(x1.y, v1.y, a[3]);
            a[4] = fma(x2.x, v2.x, a[4]); a[5] = fma(x2.y, v2.y, a[5]);
            a[6] = fma(x3.x, v3.x, a[6]); a[7] = fma(x3.y, v3.y, a[7]);
        }
        for (; i < n2; i += 64) {
            f64x2 x0 = __builtin_nontemporal_load(cx + i), v0 = rx[i];
            a[0] = fma(x0.x, v0.x, a[0]); a[1] = fma(x0.y, v0.y, a[1]);
        }
    } else {
        for (int64_t k = lane; k < n; k += 64) a[0] = fma(col[k], r[k], a[0]);
    }
    double s = wave_sum(((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])));
    if (lane == 0) out[j] = s;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// Float32 storage of the dense matrix: the same loop with 16-B loads of four floats, products and sums in f64
__global__ void __launch_bounds__(256)
k_xtv_dense_f32(const float *__restrict__ D, int64_t n, int64_t p, const double *__restrict__ r, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    int64_t j = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (j >= p) return;
    const float *col = D + j * n;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if ((n & 3) == 0 && (((uintptr_t)col) & 15) == 0) {
        const f32x4 *cx = reinterpret_cast<const f32x4 *>(col);
        const f64x2 *rx = reinterpret_cast<const f64x2 *>(r);
        const int64_t n4 = n >> 2;
        int64_t i = lane;
        for (; i + 64 < n4; i += 128) {
            f32x4 x0 = __builtin_nontemporal_load(cx + i), x1 = __builtin_nontemporal_load(cx + i + 64);
            f64x2 v0 = rx[2 * i], v1 = rx[2 * i + 1], v2 = rx[2 * (i + 64)], v3 = rx[2 * (i + 64) + 1];
            a[0] = fma((double)x0.x, v0.x, a[0]); a[1] = fma((double)x0.y, v0.y, a[1]);
            a[2] = fma((double)x0.z, v1.x, a[2]); a[3] = fma((double)x0.w, v1.y, a[3]);
            a[4] = fma((double)x1.x, v2.x, a[4]); a[5] = fma((double)x1.y, v2.y, a[5]);
            a[6] = fma((double)x1.z, v3.x, a[6]); a[7] = fma((double)x1.w, v3.y, a[7]);
        }
        for (; i < n4; i += 64) {
            f32x4 x0 = __builtin_nontemporal_load(cx + i);
            f64x2 v0 = rx[2 * i], v1 = rx[2 * i + 1];
            a[0] = fma((double)x0.x, v0.x, a[0]); a[1] = fma((double)x0.y, v0.y, a[1]);
            a[2] = fma((double)x0.z, v1.x, a[2]); a[3] = fma((double)x0.w, v1.y, a[3]);
        }
    } else {
        for (int64_t k = lane; k < n; k += 64) a[0] = fma((double)col[k], r[k], a[0]);
    }
    double s = wave_sum(((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])));
    if (lane == 0) out[j] = s;
}

// The dense kernel of choice: the four waves of a block own four adjacent columns and walk them in steps of 256
// 16-B loads per column; the residual chunk of a step is staged ONCE per block in LDS (double buffered, one barrier
// per step) instead of being re-read from L2 by every wave, and the loads of step t+1 are issued before the FMAs of
// step t.  50 000 x 100 000 f64: 5.66 ms = 7.07 TB/s against 6.19 ms for k_xtv_dense (tools/dense_probe.hip).
// NRHS residual vectors (n apart in r, p apart in out) ride the same pass over D; per (column, residual) the
// arithmetic and its order are those of the NRHS = 1 kernel, so fused and single passes give the same bits.
// Fixed lane -> row mapping, fixed final tree: bit-reproducible.  Needs n % (16 / sizeof(T)) == 0 and a 16-B aligned D.
template <typename T, int NRHS>
__global__ void __launch_bounds__(256)
k_xtv_dense_lds(const T *__restrict__ D, int64_t n, int64_t p, const double *__restrict__ r, double *__restrict__ out)
{
    constexpr int E = 16 / (int)sizeof(T);         // matrix elements per 16-B load: 2 (f64) or 4 (f32)
    constexpr int RC = 128 * E;                    // f64x2 residual pairs per step (256 loads x E rows)
    constexpr int RK = RC / 256;                   // staged pairs per thread, step and residual
    typedef T vecT __attribute__((ext_vector_type(E)));
    __shared__ f64x2 rt[2][NRHS][RC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t jj = blockIdx.x * 4ll + wave, j = jj < p ? jj : p - 1;      // idle waves redo the last column
    const vecT *cx = reinterpret_cast<const vecT *>(D + j * n);
    const int64_t nv = n / E, nr2 = n >> 1, steps = (nv + 255) / 256;
    const vecT vzero = {};
    const f64x2 rzero = {0.0, 0.0};
    double a[NRHS][4][E];
    #pragma unroll
    for (int v = 0; v < NRHS; ++v)
        #pragma unroll
        for (int u = 0; u < 4; ++u)
            #pragma unroll
            for (int e = 0; e < E; ++e) a[v][u][e] = 0.0;
    #pragma unroll
    for (int v = 0; v < NRHS; ++v) {
        const f64x2 *rx = reinterpret_cast<const f64x2 *>(r + (int64_t)v * n);
        #pragma unroll
        for (int k = 0; k < RK; ++k) { const int t = threadIdx.x + 256 * k; rt[0][v][t] = t < nr2 ? rx[t] : rzero; }
    }
    __syncthreads();
    vecT x[4], xn[4];
    #pragma unroll
    for (int u = 0; u < 4; ++u) { const int64_t i = lane + 64 * u; x[u] = i < nv ? __builtin_nontemporal_load(cx + i) : vzero; }
    for (int64_t st = 0; st < steps; ++st) {
        const int buf = (int)(st & 1);
        f64x2 rn[NRHS][RK];
        #pragma unroll
        for (int v = 0; v < NRHS; ++v) {
            const f64x2 *rx = reinterpret_cast<const f64x2 *>(r + (int64_t)v * n);
            #pragma unroll
            for (int k = 0; k < RK; ++k) { const int64_t t = (st + 1) * RC + threadIdx.x + 256 * k; rn[v][k] = t < nr2 ? rx[t] : rzero; }
        }
        #pragma unroll
        for (int u = 0; u < 4; ++u) { const int64_t i = (st + 1) * 256 + lane + 64 * u; xn[u] = i < nv ? __builtin_nontemporal_load(cx + i) : vzero; }
        #pragma unroll
        for (int v = 0; v < NRHS; ++v) {
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                #pragma unroll
                for (int h = 0; h < E / 2; ++h) {
                    const f64x2 rv = rt[buf][v][(E / 2) * (lane + 64 * u) + h];
                    a[v][u][2 * h] = fma((double)x[u][2 * h], rv.x, a[v][u][2 * h]);
                    a[v][u][2 * h + 1] = fma((double)x[u][2 * h + 1], rv.y, a[v][u][2 * h + 1]);
                }
            }
        }
        #pragma unroll
        for (int v = 0; v < NRHS; ++v)
            #pragma unroll
            for (int k = 0; k < RK; ++k) rt[buf ^ 1][v][threadIdx.x + 256 * k] = rn[v][k];
        __syncthreads();
        #pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = xn[u];
    }
    #pragma unroll
    for (int v = 0; v < NRHS; ++v) {
        double su[4];
        #pragma unroll
        for (int u = 0; u < 4; ++u) {
            su[u] = a[v][u][0] + a[v][u][1];
            if (E == 4) su[u] = su[u] + (a[v][u][2] + a[v][u][3]);
        }
        const double sum = wave_sum((su[0] + su[1]) + (su[2] + su[3]));
        if (lane == 0 && jj < p) out[(int64_t)v * p + j] = sum;
    }
}

template <typename T>
static void launch_dense_lds(const T *D, const mih_mat *h, const double *r_dev, int m, double *out_dev, hipStream_t s)
{
    const dim3 grid((unsigned)((h->p + 3) / 4)), block(256);
    int v = 0;
    if constexpr (sizeof(T) == 8)          // eight f64 residual chunks fill the 64 KB of static LDS
        for (; v + 8 <= m; v += 8)
            hipLaunchKernelGGL((k_xtv_dense_lds<T, 8>), grid, block, 0, s, D, h->n, h->p, r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
    for (; v + 4 <= m; v += 4)
        hipLaunchKernelGGL((k_xtv_dense_lds<T, 4>), grid, block, 0, s, D, h->n, h->p, r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
    if (m - v >= 2) {
        hipLaunchKernelGGL((k_xtv_dense_lds<T, 2>), grid, block, 0, s, D, h->n, h->p, r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
        v += 2;
    }
    if (m - v == 1)
        hipLaunchKernelGGL((k_xtv_dense_lds<T, 1>), grid, block, 0, s, D, h->n, h->p, r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
}

// The 16-bit dosage image (mih_dosage_create): out_j = sc_j * sum_i c_ij r_i with c_ij = num_ij - mun_j (0 where missing,
// pad rows included), the centring done per entry in numerator units before the product -- folding the mean out as
// sc_j (sum num r - mun_j sum r) cancels badly for a mean near 2.  Eight waves per block, two columns per wave (16 columns
// per block); a step is two 16-B loads (8 rows each) per lane and column, 1024 rows.  The residual chunk of a step is
// staged once per block in LDS, double buffered, as 16-B pairs in the order the lanes read them (pair 4 L + h of the
// step at h * 128 + L, L = lane + 64 u: conflict-free ds_read_b128; the coalesced global read of pair tid pays a
// 4-way conflict on the one write per step instead), and one read serves both columns of a wave.
// LDS: 2 * NRHS * 512 * 16 B = 16 KiB per residual, so NRHS <= 4 (64 KiB).  Per (column, residual) the chains and the
// final tree are those of NRHS = 1: fused and single passes give the same bits; any n (the pad rows are missing).
constexpr int kDsgWaves = 8, kDsgCols = 2, kDsgU = 2;
constexpr int kDsgPairs = kDsgU * 64 * 4;                 // f64x2 residual pairs per step
template <int NRHS>
__global__ void __launch_bounds__(512)
k_xtv_dosage_lds(DosageView dv, int64_t n, int64_t p, const double *__restrict__ r, double *__restrict__ out)
{
    constexpr int CW = kDsgWaves * kDsgCols;
    __shared__ f64x2 rt[2][NRHS][kDsgPairs];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t jj[kDsgCols], j[kDsgCols];
    const u32x4 *cx[kDsgCols];
    double mun[kDsgCols];
    #pragma unroll
    for (int c = 0; c < kDsgCols; ++c) {
        jj[c] = blockIdx.x * (int64_t)CW + wave * kDsgCols + c;
        j[c] = jj[c] < p ? jj[c] : p - 1;                   // idle columns redo the last one
        cx[c] = reinterpret_cast<const u32x4 *>(dv.X + j[c] * dv.ld);
        mun[c] = dv.mun[j[c]];
    }
    const int64_t nv = dv.ld / 8, steps = (nv + 64 * kDsgU - 1) / (64 * kDsgU);
    const u32x4 vmiss = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    // this thread stages pair tid of each step (rows 2 tid, 2 tid + 1) at LDS slot (tid & 3) * 128 + (tid >> 2)
    const int64_t trow = 2 * (int64_t)threadIdx.x;
    const int slot = (threadIdx.x & 3) * (kDsgPairs / 4) + (threadIdx.x >> 2);
    auto stage = [&](int64_t st, int v) -> f64x2 {
        const int64_t i = st * 2 * kDsgPairs + trow;
        const double *rv = r + (int64_t)v * n;
        f64x2 q; q.x = i < n ? rv[i] : 0.0; q.y = i + 1 < n ? rv[i + 1] : 0.0;
        return q;
    };
    double a[NRHS][kDsgCols][4];
    #pragma unroll
    for (int v = 0; v < NRHS; ++v)
        #pragma unroll
        for (int c = 0; c < kDsgCols; ++c)
            #pragma unroll
            for (int e = 0; e < 4; ++e) a[v][c][e] = 0.0;
    #pragma unroll
    for (int v = 0; v < NRHS; ++v) rt[0][v][slot] = stage(0, v);
    __syncthreads();
    u32x4 x[kDsgCols][kDsgU], xn[kDsgCols][kDsgU];
    #pragma unroll
    for (int c = 0; c < kDsgCols; ++c)
        #pragma unroll
        for (int u = 0; u < kDsgU; ++u) { const int64_t i = lane + 64 * u; x[c][u] = i < nv ? __builtin_nontemporal_load(cx[c] + i) : vmiss; }
    for (int64_t st = 0; st < steps; ++st) {
        const int buf = (int)(st & 1);
        f64x2 rn[NRHS];
        #pragma unroll
        for (int v = 0; v < NRHS; ++v) rn[v] = stage(st + 1, v);
        #pragma unroll
        for (int c = 0; c < kDsgCols; ++c)
            #pragma unroll
            for (int u = 0; u < kDsgU; ++u) {
                const int64_t i = (st + 1) * 64 * kDsgU + lane + 64 * u;
                xn[c][u] = i < nv ? __builtin_nontemporal_load(cx[c] + i) : vmiss;
            }
        #pragma unroll
        for (int u = 0; u < kDsgU; ++u) {
            double cv[kDsgCols][8];
            #pragma unroll
            for (int c = 0; c < kDsgCols; ++c) {
                const uint32_t w[4] = {x[c][u].x, x[c][u].y, x[c][u].z, x[c][u].w};
                #pragma unroll
                for (int k = 0; k < 4; ++k) {
                    cv[c][2 * k] = dosage_c(w[k] & 0xFFFFu, mun[c]);
                    cv[c][2 * k + 1] = dosage_c(w[k] >> 16, mun[c]);
                }
            }
            #pragma unroll
            for (int v = 0; v < NRHS; ++v)
                #pragma unroll
                for (int hh = 0; hh < 4; ++hh) {
                    const f64x2 rv = rt[buf][v][hh * (kDsgPairs / 4) + lane + 64 * u];
                    #pragma unroll
                    for (int c = 0; c < kDsgCols; ++c) {
                        a[v][c][2 * (hh & 1)] = fma(cv[c][2 * hh], rv.x, a[v][c][2 * (hh & 1)]);
                        a[v][c][2 * (hh & 1) + 1] = fma(cv[c][2 * hh + 1], rv.y, a[v][c][2 * (hh & 1) + 1]);
                    }
                }
        }
        #pragma unroll
        for (int v = 0; v < NRHS; ++v) rt[buf ^ 1][v][slot] = rn[v];
        __syncthreads();
        #pragma unroll
        for (int c = 0; c < kDsgCols; ++c)
            #pragma unroll
            for (int u = 0; u < kDsgU; ++u) x[c][u] = xn[c][u];
    }
    #pragma unroll
    for (int v = 0; v < NRHS; ++v)
        #pragma unroll
        for (int c = 0; c < kDsgCols; ++c) {
            const double sum = wave_sum((a[v][c][0] + a[v][c][1]) + (a[v][c][2] + a[v][c][3]));
            if (lane == 0 && jj[c] < p) out[(int64_t)v * p + j[c]] = sum * dv.sc[j[c]];
        }
}

static void launch_dosage_lds(const mih_mat *h, const double *r_dev, int m, double *out_dev, hipStream_t s)
{
    const dim3 grid((unsigned)((h->p + kDsgWaves * kDsgCols - 1) / (kDsgWaves * kDsgCols))), block(64 * kDsgWaves);
    const DosageView dv = dosage_view(h);
    int v = 0;
    for (; v + 4 <= m; v += 4)
        hipLaunchKernelGGL((k_xtv_dosage_lds<4>), grid, block, 0, s, dv, h->n, h->p, r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
    if (m - v >= 2) {
        hipLaunchKernelGGL((k_xtv_dosage_lds<2>), grid, block, 0, s, dv, h->n, h->p, r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
        v += 2;
    }
    if (m - v == 1)
        hipLaunchKernelGGL((k_xtv_dosage_lds<1>), grid, block, 0, s, dv, h->n, h->p, r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
}

int xtv_dense_device(const mih_mat *h, const XtvWork &w, const double *r_dev, int m, double *out_dev, hipStream_t s)
{
    const bool f32 = h->Df != nullptr;
    const bool lds_ok = w.tune.variant < 0 && (((uintptr_t)(f32 ? (const void *)h->Df : (const void *)h->D)) & 15) == 0 && h->n % (f32 ? 4 : 2) == 0;
    PassRecord rec;
    const bool prof = prof_begin(h, s, rec);
    if (h->Du) launch_dosage_lds(h, r_dev, m, out_dev, s);                 // (any n, any alignment: no fallback kernel)
    else if (lds_ok) {
        if (f32) launch_dense_lds<float>(h->Df, h, r_dev, m, out_dev, s);
        else launch_dense_lds<double>(h->D, h, r_dev, m, out_dev, s);
    } else {
        for (int v = 0; v < m; ++v) {
            if (f32) hipLaunchKernelGGL(k_xtv_dense_f32, dim3((unsigned)((h->p + 3) / 4)), dim3(256), 0, s, h->Df, h->n, h->p,
                                        r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
            else hipLaunchKernelGGL(k_xtv_dense, dim3((unsigned)((h->p + 3) / 4)), dim3(256), 0, s, h->D, h->n, h->p,
                                    r_dev + (int64_t)v * h->n, out_dev + (int64_t)v * h->p);
        }
    }
    if (prof) {
        rec.residuals = m; rec.operands = m; rec.stream_tag = w.stream_tag;
        if (h->Du) snprintf(rec.kernel, sizeof(rec.kernel), "k_xtv_dosage_lds<u16>");
        else snprintf(rec.kernel, sizeof(rec.kernel), "%s<%s>", lds_ok ? "k_xtv_dense_lds" : "k_xtv_dense", f32 ? "f32" : "f64");
        prof_end(h, s, rec);
    }
    MIH_HIP(hipGetLastError());
    return MIH_OK;
}

}  // namespace mih
