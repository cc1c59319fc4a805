// xb.hip -- OUT = X B for a dense B (p x t) through the row image of X (mih_snp_transpose): X B = (X')' B, so the X'r pass over
// the 2-bit matrix of the transposed genotypes, with the columns of B as its "residuals", is the dense forward product.  It is the
// mirror image of xv.hip's header and of xtv_finalize_col: there mu and 1/sigma sit on the output axis and are applied behind the
// pass; here they sit on the contracted axis, so they move into B in front of it.  With a_jt = (scale ? sinv_j : 1) B_jt
//   out_it = sum_j code_ij a_jt               the pass over the row image: raw codes, missing = 0 (XtvWork::raw)
//          + sum_{j in miss(i)} mu_j a_jt      impute: the per-sample lists of the row image, ascending j, one f64 chain
//          - sum_j mu_j a_jt                   center: c_t, one fixed-order sum per column of B, the same for every sample
// in this order.  Everything but the pass is one rounding per operation in f64 with contraction off; c_t is a fixed tree (below),
// so a column of OUT depends on its column of B, the two matrices and the format, and on nothing else.
#include "common.h"
#include <algorithm>

namespace mih {

constexpr int kXbChunk = 1024;             // entries of a column of B per workgroup of k_xb_coef: four per thread, then a tree over 256

// the fixed tree over the 256 threads' values (every level adds neighbours at a fixed distance): the sum in red[0]
__device__ __forceinline__ void xb_tree(double *red)
{
    for (int d = 128; d > 0; d >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < d) red[threadIdx.x] = __dadd_rn(red[threadIdx.x], red[threadIdx.x + d]);
    }
    __syncthreads();
}

// grid (chunks of kXbChunk SNPs, t): a = (scale ? sinv : 1) B into A, mu a into MA (MA != nullptr: the call centres or imputes),
// and the chunk's sum of mu a into part[chunk + nchunk * column]: thread k adds entries k, k + 256, k + 512, k + 768 of the chunk
// in this order, then the tree.
__global__ void __launch_bounds__(256)
k_xb_coef(const double *__restrict__ B, int64_t p, const double *__restrict__ mu, const double *__restrict__ sinv, int scale,
          double *__restrict__ A, double *__restrict__ MA, double *__restrict__ part)
{
    __shared__ double red[256];
    const int64_t col = blockIdx.y, j0 = (int64_t)blockIdx.x * kXbChunk;
    double acc = 0.0;
    for (int k = 0; k < kXbChunk / 256; ++k) {
        const int64_t j = j0 + k * 256 + threadIdx.x;
        if (j >= p) break;
        const double a = scale ? __dmul_rn(sinv[j], B[col * p + j]) : B[col * p + j];
        A[col * p + j] = a;
        if (MA) {
            const double ma = __dmul_rn(mu[j], a);
            MA[col * p + j] = ma;
            acc = __dadd_rn(acc, ma);
        }
    }
    if (!MA) return;                                             // (the same for every thread)
    red[threadIdx.x] = acc;
    xb_tree(red);
    if (threadIdx.x == 0) part[col * gridDim.x + blockIdx.x] = red[0];
}

// one workgroup per column of B: c_t from the chunks' sums -- thread k adds chunks k, k + 256, ... in this order, then the tree
__global__ void __launch_bounds__(256)
k_xb_const(const double *__restrict__ part, int64_t nchunk, double *__restrict__ c)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < nchunk; b += 256) acc = __dadd_rn(acc, part[blockIdx.x * nchunk + b]);
    red[threadIdx.x] = acc;
    xb_tree(red);
    if (threadIdx.x == 0) c[blockIdx.x] = red[0];
}

// One thread per sample and all t columns: the pass's raw dot, plus the imputation chain over the sample's missing SNPs (the row
// image's list, ascending), minus the column's constant.  A column the pass answered with NaN stays NaN.
__global__ void __launch_bounds__(256)
k_xb_finish(double *__restrict__ out, int64_t n, int64_t p, int t, const int64_t *__restrict__ miss_ptr, const int32_t *__restrict__ miss_row,
            const double *__restrict__ MA, const double *__restrict__ c, int center, int impute)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t a = 0, b = 0;
    if (impute) { a = miss_ptr[i]; b = miss_ptr[i + 1]; }
    for (int u = 0; u < t; ++u) {
        double v = out[(int64_t)u * n + i];
        if (b > a) {
            double ms = 0.0;
            for (int64_t k = a; k < b; ++k) ms = __dadd_rn(ms, MA[(int64_t)u * p + miss_row[k]]);
            v = __dadd_rn(v, ms);
        }
        if (center) v = __dadd_rn(v, -c[u]);
        out[(int64_t)u * n + i] = v;
    }
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_xb_dense(const mih_mat *h, const mih_mat *rows, const double *B, int32_t t, int center, int scale, int impute, int digits,
                 double *OUT)
{
    if (!h || !rows || !B || !OUT) { set_error("null argument"); return MIH_BAD_ARG; }
    if (h->kind != 0 || rows->kind != 0) {
        set_error("mih_xb_dense needs a 2-bit (SnpLinAlg) handle and its row image; the products of dense and dosage handles are not offered");
        return MIH_BAD_ARG;
    }
    if (rows->n != h->p || rows->p != h->n || rows->device != h->device || rows->total_missing != h->total_missing) {
        set_error("mih_xb_dense: `rows` (%lld x %lld, %lld missing, device %d) is not the transposed image of the %lld x %lld matrix "
                  "(%lld missing, device %d)", (long long)rows->n, (long long)rows->p, (long long)rows->total_missing, rows->device,
                  (long long)h->n, (long long)h->p, (long long)h->total_missing, h->device);
        return MIH_BAD_ARG;
    }
    if (t < 1) { set_error("mih_xb_dense: t = %d columns", (int)t); return MIH_BAD_ARG; }
    for (int f : {center, scale, impute})
        if (f < -1 || f > 1) { set_error("center, scale and impute must be 0, 1 or -1 (the handle's)"); return MIH_BAD_ARG; }
    if (center < 0) center = h->center;
    if (scale < 0) scale = h->scale;
    if (impute < 0) impute = h->impute;
    impute = impute && h->total_missing > 0;
    const int64_t n = h->n, p = h->p;
    MIH_HIP(hipSetDevice(h->device));
    MIH_HIP(hipStreamSynchronize(h->stream));
    hipStream_t s = rows->stream;
    XtvWork w;
    w.raw = true;
    MIH_TRY(xtv_work_init(rows, w, t, xtv_tune(digits)));
    const bool corr = center || impute;
    const int64_t nchunk = (p + kXbChunk - 1) / kXbChunk;
    DevBuf<double> b, a, ma, part, c, out;
    MIH_TRY(b.alloc((size_t)t * p));
    MIH_TRY(a.alloc((size_t)t * p));
    if (corr) {
        MIH_TRY(ma.alloc((size_t)t * p));
        MIH_TRY(part.alloc((size_t)t * nchunk));
        MIH_TRY(c.alloc((size_t)t));
    }
    MIH_TRY(out.alloc((size_t)t * n));
    MIH_HIP(hipMemcpyAsync(b.p, B, sizeof(double) * (size_t)t * p, hipMemcpyHostToDevice, s));
    for (int32_t u0 = 0; u0 < t; u0 += 65535) {                  // (grid.y stays below 65536)
        const int32_t nu = std::min<int32_t>(65535, t - u0);
        hipLaunchKernelGGL(k_xb_coef, dim3((unsigned)nchunk, (unsigned)nu), dim3(256), 0, s, b.p + (int64_t)u0 * p, p, h->mu, h->sinv, scale,
                           a.p + (int64_t)u0 * p, corr ? ma.p + (int64_t)u0 * p : nullptr, corr ? part.p + (int64_t)u0 * nchunk : nullptr);
    }
    if (corr) hipLaunchKernelGGL(k_xb_const, dim3((unsigned)t), dim3(256), 0, s, part.p, nchunk, c.p);
    MIH_TRY(xtv_device(rows, w, a.p, t, out.p, s));
    if (corr)
        hipLaunchKernelGGL(k_xb_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out.p, n, p, (int)t, rows->miss_ptr, rows->miss_row,
                           ma.p, c.p, center, impute);
    MIH_HIP(hipMemcpyAsync(OUT, out.p, sizeof(double) * (size_t)t * n, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    xtv_count_peels(rows, w, s);
    return MIH_OK;
}

}  // extern "C"
