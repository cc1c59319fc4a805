// assoc_slab.h -- the device code that the per-column solvers of the case-control scan share (k_assoc_spa in assoc_spa.hip,
// k_assoc_firth in assoc_firth.hip): the slab of covariate-adjusted genotypes c_i = x_ij - Z_i. alpha_j that a workgroup forms
// ONCE per flagged column (decode by handle kind, the missing list, Z alpha, M1 and the ends of the range), the fixed LDS tree of
// the 256 partial sums, and the pass over the rows that gives K and K'' at a root.  One copy, inlined into both kernels.
#pragma once
#include "assoc.h"

namespace mih {

// The pieces of the per-kind column decode that every kernel working on decoded columns shares (the slabs below, the set Gram
// of assoc_sets.hip).  2-bit: the four values of a column as k_xtv_finalize multiplies them (k_ib_solve's expressions) -- codes
// 0, 1, 2 and a row of the column's missing list (the list holds a column's rows in ascending order, as the constructors write it).
struct SnpVals { double x0, x1, x2, xm; };
__device__ __forceinline__ SnpVals snp_vals(const ColView &m, int64_t j)
{
#pragma clang fp contract(off)
    const double s = m.scale ? m.sinv[j] : 1.0, cm = m.center ? m.mu[j] : 0.0;
    SnpVals v;
    v.x0 = (0.0 - cm) * s; v.x1 = (1.0 - cm) * s; v.x2 = (2.0 - cm) * s; v.xm = ((m.impute ? m.mu[j] : 0.0) - cm) * s;
    return v;
}
// dense f64 (KIND 0), dense f32 (1) and 16-bit dosage (2): the entry mih_xtv multiplies
template <int KIND>
__device__ __forceinline__ double slab_dense_x(const ColView &m, int64_t n, int64_t j, int64_t i)
{
    return KIND == 0 ? m.D[j * n + i] : KIND == 1 ? (double)m.Df[j * n + i] : dosage_x(m.dv, j, i);
}

// red[v][0] becomes the sum of red[v][0 .. 256), v < nv, over the fixed tree k = 128, 64, ... 1: red[tid] += red[tid + k]
__device__ __forceinline__ void spa_tree(double (*red)[256], int nv)
{
#pragma clang fp contract(off)
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k)
            for (int v = 0; v < nv; ++v) red[v][threadIdx.x] = red[v][threadIdx.x] + red[v][threadIdx.x + k];
        __syncthreads();
    }
}

// One pass over the rows of a column at argument t, the thread's rows tid, tid + 256, ... in ascending order:
//   ROOT = false:  a = sum c_i (sigma(x_i) - aux_i),  aux = mu            b = sum c_i^2 sigma(x_i) (1 - sigma(x_i))
//   ROOT = true:   a = sum (softplus(x_i) - aux_i),   aux = softplus(eta)  b likewise
// x_i = eta_i + c_i t.  The loads of kSpaAhead rows are issued before the first of them is used (a pass is bound by the latency
// of its loads otherwise: one row per thread in flight); the terms are added in row order all the same, so the sums do not
// depend on it.
constexpr int kSpaAhead = 4;

template <bool ROOT>
__device__ __forceinline__ void spa_term(double cc, double h, double aux, double t, double &a, double &b)
{
#pragma clang fp contract(off)
    const double x = h + cc * t, e = exp(-fabs(x)), r = 1.0 / (1.0 + e), er = e * r;
    if (ROOT) a = a + ((fmax(x, 0.0) + log1p(e)) - aux);
    else a = a + cc * ((x >= 0.0 ? r : er) - aux);
    b = b + (cc * cc) * (er * r);
}

template <bool ROOT>
__device__ __forceinline__ void spa_pass(const double *cs, const double *__restrict__ eta, const double *__restrict__ aux,
                                         int64_t n, double t, double &a, double &b)
{
    a = 0.0; b = 0.0;
    int64_t i = threadIdx.x;
    for (; i + 256 * (kSpaAhead - 1) < n; i += 256 * kSpaAhead) {
        double cc[kSpaAhead], h[kSpaAhead], ax[kSpaAhead];
        #pragma unroll
        for (int u = 0; u < kSpaAhead; ++u) { cc[u] = cs[i + 256 * u]; h[u] = eta[i + 256 * u]; ax[u] = aux[i + 256 * u]; }
        #pragma unroll
        for (int u = 0; u < kSpaAhead; ++u) spa_term<ROOT>(cc[u], h[u], ax[u], t, a, b);
    }
    for (; i < n; i += 256) spa_term<ROOT>(cs[i], eta[i], aux[i], t, a, b);
}

// The slab of column j: cs[i] = c_i for every row, and this thread's shares of M1 = sum c_i mu_i (a0), sum min(c_i, 0) (a1) and
// sum max(c_i, 0) (a2) over its rows tid, tid + 256, ...  al: the column's alpha in LDS, written by the caller before the call
// (the barriers in here order it).  KIND 0: f64, 1: f32, 2: dosage, 3: 2-bit.
template <int KIND>
__device__ __forceinline__ void spa_slab_form(const ColView &m, int64_t n, int64_t j, int c, const double *al, const double *__restrict__ Z,
                                              const double *__restrict__ mu, double *cs, double &a0, double &a1, double &a2)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    if (KIND == 3) {                                     // the stored codes first, then the column's missing rows over them
        const SnpVals sv = snp_vals(m, j);
        const double x0 = sv.x0, x1 = sv.x1, x2 = sv.x2, xm = sv.xm;
        for (int64_t i = tid; i < n; i += 256) {
            const uint32_t g = (m.X[xword(m.nbp, j, i >> 4)] >> (2 * (int)(i & 15))) & 3u;
            cs[i] = g == 0u ? x0 : g == 1u ? x1 : x2;
        }
        __syncthreads();
        for (int64_t e = m.miss_ptr[j] + tid, e1 = m.miss_ptr[j + 1]; e < e1; e += 256) {
            const int64_t row = m.miss_row[e];
            if (row >= 0 && row < n) cs[row] = xm;
        }
    }
    __syncthreads();
    // c_i, M1 = sum c_i mu_i and the two ends of the range
    a0 = 0.0; a1 = 0.0; a2 = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
        const double x = KIND == 3 ? cs[i] : slab_dense_x<KIND>(m, n, j, i);
        double za = 0.0;
        for (int k = 0; k < c; ++k) za = za + Z[(int64_t)k * n + i] * al[k];
        const double cc = x - za;
        cs[i] = cc;
        a0 = a0 + cc * mu[i];
        a1 = a1 + fmin(cc, 0.0);
        a2 = a2 + fmax(cc, 0.0);
    }
}

}  // namespace mih
