// dosage.hip -- the 16-bit dosage design matrix (mih_dosage_create*): imputed VCF DS / BGEN dosages and hard calls on a grid of
// num / denom, stored as u16 numerators (4x less HBM than the reference's Matrix{Float64}).  Ingest, the column statistics of
// standardize_genotypes! (src/wrapper.jl:406-423), the seeded synthetic generator and the export of numerators.  The matrix
// is a dense one (kind 1) to every fit; the sites that read its storage standardize per entry (common.h: dosage_x,
// xtv_dense.hip: k_xtv_dosage_lds).
#include "common.h"
#include <cmath>

namespace mih {

// One block per column: count and sum the non-missing numerators (integers: the order does not matter), count the entries
// outside [0, 2 denom], and set mu_j, 1/sigma_j (dosage units) and their numerator-unit forms.  sigma_j = sqrt(mu (1 - mu/2))
// as SnpLinAlg; a column with sigma_j = 0 is centred but not scaled; an all-missing column is all zeros (mu_j = 0).
__global__ void __launch_bounds__(256)
k_dosage_stats(const uint16_t *__restrict__ X, int64_t ld, int32_t denom, double *__restrict__ mu, double *__restrict__ sinv,
               double *__restrict__ mun, double *__restrict__ sc, unsigned long long *__restrict__ bad)
{
    __shared__ unsigned long long s_sum[256], s_cnt[256], s_bad[256];
    const int64_t j = blockIdx.x;
    const uint4 *cx = reinterpret_cast<const uint4 *>(X + j * ld);
    const uint32_t top = 2u * (uint32_t)denom;
    unsigned long long sum = 0, cnt = 0, nbad = 0;
    for (int64_t i = threadIdx.x; i < ld / 8; i += 256) {
        const uint4 q = cx[i];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        #pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t v = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
            if (v != 0xFFFFu) {
                if (v > top) ++nbad;
                else { sum += v; ++cnt; }
            }
        }
    }
    s_sum[threadIdx.x] = sum; s_cnt[threadIdx.x] = cnt; s_bad[threadIdx.x] = nbad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + w]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + w];
            s_bad[threadIdx.x] += s_bad[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double S = (double)s_sum[0], N = (double)s_cnt[0];
        const double m = N > 0.0 ? S / (N * (double)denom) : 0.0;        // N * denom < 2^53: one rounding
        const double s = sqrt(m * (1.0 - m / 2.0));
        mu[j] = m;
        sinv[j] = s > 0.0 ? 1.0 / s : 1.0;
        mun[j] = N > 0.0 ? S / N : 0.0;
        sc[j] = sinv[j] / (double)denom;
        if (s_bad[0]) atomicAdd(bad, s_bad[0]);
    }
}

__device__ __forceinline__ uint32_t dsg_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// Synthetic dosages: hard calls Binomial(2, rho_j), rho_j ~ U(0, 0.5) (data/README.md), moved by up to +-0.1 on the grid
// and clamped to [0, 2]; missing with probability missing_rate.  Keyed by (seed, column, row): the same matrix for any launch
// shape.  One thread writes 8 rows (one 16-B store); the pad rows are missing.
__global__ void __launch_bounds__(256)
k_dosage_synth(uint16_t *__restrict__ X, int64_t ld, int64_t n, int64_t p, uint64_t seed, int32_t denom, uint32_t miss_thr)
{
    const int64_t nv = ld / 8, total = nv * p;
    const uint32_t s0 = dsg_mix((uint32_t)seed ^ 0x3C6EF372u) ^ dsg_mix((uint32_t)(seed >> 32) + 0x1B873593u);
    const int32_t blur = denom / 10;                       // |delta| <= 0.1 on the grid
    for (int64_t q = blockIdx.x * 256ll + threadIdx.x; q < total; q += 256ll * gridDim.x) {
        const int64_t j = q / nv, i0 = (q - j * nv) * 8;
        const uint32_t key = dsg_mix(s0 ^ dsg_mix((uint32_t)j) ^ dsg_mix((uint32_t)(j >> 32) + 0x85EBCA6Bu));
        const uint32_t thr = (uint32_t)(((dsg_mix(key ^ 0xB5297A4Du) >> 8) + 0.5) / 16777216.0 * 0.5 * 65536.0);   // rho_j in 1/65536
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        #pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t i = i0 + k;
            uint32_t v = 0xFFFFu;
            if (i < n) {
                const uint32_t e = dsg_mix(key ^ dsg_mix((uint32_t)i ^ 0x68E31DA4u) ^ (uint32_t)(i >> 32));
                const uint32_t f = dsg_mix(e ^ 0x1B56C4E9u), g = dsg_mix(f ^ 0x2C1B3C6Du);
                const int32_t calls = (int32_t)((e & 0xFFFFu) < thr) + (int32_t)((e >> 16) < thr);
                const int32_t d = blur > 0 ? (int32_t)(f % (uint32_t)(2 * blur + 1)) - blur : 0;
                int32_t num = calls * denom + d;
                num = num < 0 ? 0 : (num > 2 * denom ? 2 * denom : num);
                v = g < miss_thr ? 0xFFFFu : (uint32_t)num;
            }
            w[k >> 1] |= v << (16 * (k & 1));
        }
        reinterpret_cast<uint4 *>(X + j * ld)[i0 / 8] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// allocate the storage and statistics of an n x p dosage matrix (kind 1, no centring flags: the storage standardizes)
int dosage_alloc(mih_mat *h, int64_t n, int64_t p, int32_t denom, int device)
{
    h->kind = 1; h->device = device; h->n = n; h->p = p; h->center = h->scale = h->impute = 0;
    h->denom = denom;
    h->du_ld = (n + 7) / 8 * 8;
    if (device_malloc((void **)&h->Du, sizeof(uint16_t) * (size_t)h->du_ld * (size_t)p) != hipSuccess) {
        set_error("hipMalloc for the dosage matrix (%lld x %lld u16) failed", (long long)n, (long long)p); (void)hipGetLastError(); return MIH_OOM;
    }
    for (double **a : {&h->mu, &h->sinv, &h->du_mun, &h->du_sc})
        if (device_malloc((void **)a, sizeof(double) * (size_t)p) != hipSuccess) { set_error("hipMalloc failed"); (void)hipGetLastError(); return MIH_OOM; }
    if (hipStreamCreate(&h->stream) != hipSuccess) return MIH_HIP_ERROR;
    return MIH_OK;
}

// column statistics; MIH_BAD_ARG if a numerator other than 0xFFFF exceeds 2 denom
int dosage_stats(mih_mat *h)
{
    DevBuf<unsigned long long> bad;
    MIH_TRY(bad.alloc(1));
    MIH_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_dosage_stats, dim3((unsigned)h->p), dim3(256), 0, h->stream, h->Du, h->du_ld, h->denom, h->mu, h->sinv,
                       h->du_mun, h->du_sc, bad.p);
    unsigned long long nbad = 0;
    MIH_HIP(hipMemcpyAsync(&nbad, bad.p, sizeof(nbad), hipMemcpyDeviceToHost, h->stream));
    MIH_HIP(hipStreamSynchronize(h->stream));
    if (nbad) { set_error("%llu dosage numerators exceed 2 * denom = %d (0xFFFF marks a missing entry)", nbad, 2 * h->denom); return MIH_BAD_ARG; }
    return MIH_OK;
}

// Column j of the numerators times m_j = gcol[j] / g (the BGEN reader's fix-up onto the common grid) or times mult (regrid):
// a value v / denom becomes (v m) / (denom m), exactly; 0xFFFF stays missing.  One block per column, 8 rows per thread.
__global__ void __launch_bounds__(256)
k_dosage_scale(uint16_t *__restrict__ X, int64_t ld, const uint32_t *__restrict__ gcol, uint32_t g, uint32_t mult)
{
    const int64_t j = blockIdx.x;
    const uint32_t m = gcol ? gcol[j] / g : mult;
    if (m == 1u) return;
    uint4 *cx = reinterpret_cast<uint4 *>(X + j * ld);
    for (int64_t i = threadIdx.x; i < ld / 8; i += 256) {
        const uint4 q = cx[i];
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = w[k] & 0xFFFFu, hi = w[k] >> 16;
            w[k] = (lo == 0xFFFFu ? lo : lo * m) | ((hi == 0xFFFFu ? hi : hi * m) << 16);
        }
        cx[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

void dosage_rescale(mih_mat *h, const uint32_t *gcol, uint32_t g, uint32_t mult)
{
    hipLaunchKernelGGL(k_dosage_scale, dim3((unsigned)h->p), dim3(256), 0, h->stream, h->Du, h->du_ld, gcol, g, mult);
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_dosage_create(const uint16_t *num, int64_t n, int64_t p, int64_t col_stride, int32_t denom, int device, mih_mat **out)
{
    if (!num || !out) { set_error("null argument"); return MIH_BAD_ARG; }
    if (n <= 0 || p <= 0 || col_stride < n) { set_error("bad dimensions"); return MIH_BAD_DIM; }
    if (denom < 1 || denom > 32767) { set_error("denom must be in [1, 32767], got %d", denom); return MIH_BAD_ARG; }
    MIH_TRY(select_device(device));
    mih_mat *h = new mih_mat();
    auto fail = [&](int code) { mih_mat_destroy(h); return code; };
    int rc = dosage_alloc(h, n, p, denom, device);
    if (rc) return fail(rc);
    const size_t ld_b = sizeof(uint16_t) * (size_t)h->du_ld;
    if (h->du_ld > n && hipMemset2DAsync(h->Du + n, ld_b, 0xFF, sizeof(uint16_t) * (size_t)(h->du_ld - n), (size_t)p, h->stream) != hipSuccess)
        return fail(MIH_HIP_ERROR);
    if (hipMemcpy2DAsync(h->Du, ld_b, num, sizeof(uint16_t) * (size_t)col_stride, sizeof(uint16_t) * (size_t)n, (size_t)p,
                         hipMemcpyHostToDevice, h->stream) != hipSuccess) { set_error("dosage upload failed"); return fail(MIH_HIP_ERROR); }
    if ((rc = dosage_stats(h))) return fail(rc);
    *out = h;
    return MIH_OK;
}

int mih_dosage_create_synthetic(int64_t n, int64_t p, uint64_t seed, int32_t denom, double missing_rate, int device, mih_mat **out)
{
    if (!out) { set_error("null argument"); return MIH_BAD_ARG; }
    if (n <= 0 || p <= 0) { set_error("bad dimensions"); return MIH_BAD_DIM; }
    if (denom < 1 || denom > 32767) { set_error("denom must be in [1, 32767], got %d", denom); return MIH_BAD_ARG; }
    if (!(missing_rate >= 0.0 && missing_rate < 1.0)) { set_error("missing_rate must be in [0,1)"); return MIH_BAD_ARG; }
    MIH_TRY(select_device(device));
    mih_mat *h = new mih_mat();
    auto fail = [&](int code) { mih_mat_destroy(h); return code; };
    int rc = dosage_alloc(h, n, p, denom, device);
    if (rc) return fail(rc);
    const uint32_t miss_thr = (uint32_t)(missing_rate * 4294967296.0);
    hipLaunchKernelGGL(k_dosage_synth, dim3(8192), dim3(256), 0, h->stream, h->Du, h->du_ld, n, p, seed, denom, miss_thr);
    if ((rc = dosage_stats(h))) return fail(rc);
    *out = h;
    return MIH_OK;
}

int mih_dosage_regrid(mih_mat *h, int32_t denom)
{
    if (!h || !h->Du) { set_error("not a dosage handle"); return MIH_BAD_ARG; }
    if (denom < 1 || denom > 32767 || denom % h->denom != 0) {
        set_error("denom must be a multiple of the handle's denominator %d and at most 32767, got %d", h->denom, denom); return MIH_BAD_ARG;
    }
    if (denom == h->denom) return MIH_OK;
    MIH_HIP(hipSetDevice(h->device));
    dosage_rescale(h, nullptr, 1u, (uint32_t)(denom / h->denom));
    h->denom = denom;
    return dosage_stats(h);
}

int mih_dosage_export(const mih_mat *h, int64_t col0, int64_t ncols, uint16_t *out)
{
    if (!h || !h->Du || !out) { set_error("not a dosage handle"); return MIH_BAD_ARG; }
    if (col0 < 0 || ncols < 0 || col0 + ncols > h->p) { set_error("columns [%lld, %lld) out of range", (long long)col0, (long long)(col0 + ncols)); return MIH_BAD_DIM; }
    if (ncols == 0) return MIH_OK;
    MIH_HIP(hipSetDevice(h->device));
    MIH_HIP(hipMemcpy2D(out, sizeof(uint16_t) * (size_t)h->n, h->Du + col0 * h->du_ld, sizeof(uint16_t) * (size_t)h->du_ld,
                        sizeof(uint16_t) * (size_t)h->n, (size_t)ncols, hipMemcpyDeviceToHost));
    return MIH_OK;
}

}  // extern "C"
