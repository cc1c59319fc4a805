// transpose.hip -- a 2-bit matrix of the transposed genotypes, made on the device (mih_snp_transpose): SNPs as rows, samples as
// columns, in the same tile-major layout, with its own mu and 1/sigma (per sample) and its own ascending missing lists.  The stored
// tile is the MFMA A fragment with K = the row axis, so nothing in an image can be contracted over its columns (DESIGN.md §11,
// §13); the X'r pass over THIS image is the dense forward product X B of the original (xb.hip).
#include "common.h"
#include "transpose_bits.h"
#include <algorithm>

namespace mih {

constexpr int kTrBlocks = 16;              // 128-SNP blocks one wave walks, its samples' counts in registers meanwhile
constexpr int kTrGroup = 68;               // dwords of LDS per group of 16 lane records: 64 and four of padding (below)

// The lane records of the result.  Work item: the 128 x 128 block (B, bp) -- source tiles (4 B + c, bp), c = 0 .. 3 (a tile with
// 4 B + c >= s_ncg does not exist and counts as zeros), become result tiles (4 bp + r, B), r = 0 .. 3.  A workgroup is one wave;
// it keeps bp and walks kTrBlocks values of B.  Per block:
//   1. four coalesced 1 KB loads, a 16-byte record per lane, into LDS;
//   2. lane (c, h, q = 2 e + u, u') takes the 16 x 16 matrix of 2-bit fields held by dword q of the records 32 h + 16 u' + s'
//      (s' = 0 .. 15) of source tile c -- SNPs 32 c + 16 u' + s' by samples 64 e + 32 h + 16 u + s of the block -- and transposes
//      it in registers (transpose_bits.h).  Row s of the result is dword q' = 2 (c >> 1) + u' of record 32 (c & 1) + 16 u + s of
//      result tile r = 2 e + h: sample 32 r + 16 u + s, SNPs 64 (c >> 1) + 32 (c & 1) + 16 u' + (0 .. 15).  Back to LDS;
//   3. four coalesced 1 KB stores, a 16-byte record per lane.
// LDS holds a group of 16 records in kTrGroup dwords: the 64 lanes of step 2 read and write dword (group g, record s', q) at
// 68 g + 4 s' + q, sixteen groups and four q -- 64 different banks.  Every record of every result tile is written (pad SNPs and
// pad samples are zeros in the source, so zeros here).  The source holds its missing entries as code 0 and so does the result
// until k_transpose_missing marks them.  n1 and n2 of every sample are counted into cnt[3 i + {0, 1}] (integer atomics, one per
// sample, counter and workgroup).
__global__ void __launch_bounds__(64)
k_transpose_tiles(const uint4 *__restrict__ S, int64_t s_ncg, int64_t s_nbp, int64_t s_n, uint4 *__restrict__ X, int64_t ncg, int64_t nbp,
                  int64_t nchunk, int32_t *__restrict__ cnt)
{
    __shared__ uint4 in4[16 * kTrGroup / 4], out4[16 * kTrGroup / 4];
    uint32_t *in = reinterpret_cast<uint32_t *>(in4), *out = reinterpret_cast<uint32_t *>(out4);
    const int lane = threadIdx.x;
    const int64_t bp = blockIdx.x / nchunk, B0 = (blockIdx.x % nchunk) * kTrBlocks;
    const int c = lane >> 4, h = (lane >> 3) & 1, q = (lane >> 1) & 3, up = lane & 1;
    const int g_in = c * 4 + 2 * h + up;                              // the group of 16 source records this lane transposes
    const int g_out = (2 * (q >> 1) + h) * 4 + 2 * (c & 1) + (q & 1), q_out = 2 * (c >> 1) + up;
    int32_t c1[4] = {0, 0, 0, 0}, c2[4] = {0, 0, 0, 0};
    for (int64_t B = B0; B < B0 + kTrBlocks && B < nbp; ++B) {       // (the same trips for every lane)
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t cg = 4 * B + k;
            const uint4 v = cg < s_ncg ? S[(cg * s_nbp + bp) * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
            in4[((k * 4 + (lane >> 4)) * kTrGroup + 4 * (lane & 15)) >> 2] = v;
        }
        __syncthreads();
        uint32_t x[16];
        #pragma unroll
        for (int s = 0; s < 16; ++s) x[s] = in[g_in * kTrGroup + 4 * s + q];
        transpose16x16_2bit(x);
        #pragma unroll
        for (int s = 0; s < 16; ++s) out[g_out * kTrGroup + 4 * s + q_out] = x[s];
        __syncthreads();
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t cg = 4 * bp + r;
            if (cg >= ncg) continue;
            const uint4 v = out4[((r * 4 + (lane >> 4)) * kTrGroup + 4 * (lane & 15)) >> 2];
            X[(cg * nbp + B) * 64 + lane] = v;
            c1[r] += __popc(v.x & 0x55555555u) + __popc(v.y & 0x55555555u) + __popc(v.z & 0x55555555u) + __popc(v.w & 0x55555555u);
            c2[r] += __popc(v.x & 0xAAAAAAAAu) + __popc(v.y & 0xAAAAAAAAu) + __popc(v.z & 0xAAAAAAAAu) + __popc(v.w & 0xAAAAAAAAu);
        }
        // (the next trip writes `in` behind this trip's second barrier and `out` behind its own first: two barriers a trip are enough)
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) {                                     // the two halves of a sample's records meet in lane m
        const int32_t a1 = c1[r] + __shfl_xor(c1[r], 32, 64), a2 = c2[r] + __shfl_xor(c2[r], 32, 64);
        const int64_t i = bp * 128 + r * 32 + (lane & 31);
        if (lane < 32 && i < s_n) {
            if (a1) atomicAdd(&cnt[3 * i], a1);
            if (a2) atomicAdd(&cnt[3 * i + 1], a2);
        }
    }
}

// One wave per source column (SNP) j over its missing list: entry (sample i, SNP j) of the result gets the temporary code 3, which
// finish_tiles lists per sample in ascending SNP order and turns back into code 0 -- the route of a freshly transcoded matrix.
// An or of a constant per entry: the result does not depend on the order.
__global__ void __launch_bounds__(64)
k_transpose_missing(const int64_t *__restrict__ s_ptr, const int32_t *__restrict__ s_row, int64_t j0, uint32_t *__restrict__ X, int64_t nbp)
{
    const int64_t j = j0 + blockIdx.x;
    const int64_t a = s_ptr[j], b = s_ptr[j + 1];
    const uint32_t bits = 3u << (2 * (int)(j & 15));
    for (int64_t t = a + threadIdx.x; t < b; t += 64) atomicOr(&X[xword(nbp, (int64_t)s_row[t], j >> 4)], bits);
}

// the per-sample missing counts of k_missing_counts into the counters finish_tiles reads
__global__ void k_place_missing(const int32_t *__restrict__ row_missing, int64_t n, int32_t *__restrict__ cnt)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) cnt[3 * i + 2] = row_missing[i];
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_snp_transpose(const mih_mat *src, int center, int scale, int impute, int dtype, int64_t reserve_bytes, mih_mat **out)
{
    if (!out) { set_error("null argument"); return MIH_BAD_ARG; }
    *out = nullptr;
    if (!src || src->kind != 0) { set_error("mih_snp_transpose needs a 2-bit (SnpLinAlg) handle"); return MIH_BAD_ARG; }
    if (dtype != 64 && dtype != 32) { set_error("dtype must be 64 (SnpLinAlg{Float64}) or 32 (SnpLinAlg{Float32})"); return MIH_BAD_ARG; }
    const int64_t n = src->p, p = src->n;                          // of the result
    if (n >= (1ll << 31)) { set_error("the transposed matrix would have %lld rows: n must be < 2^31", (long long)n); return MIH_BAD_DIM; }
    MIH_HIP(hipSetDevice(src->device));
    const int64_t ncg = (p + 31) / 32, nbp = (n + 127) / 128, nchunk = (nbp + kTrBlocks - 1) / kTrBlocks;
    if (src->nbp * nchunk >= (1ll << 31)) { set_error("the matrix has too many tiles for one launch"); return MIH_BAD_DIM; }

    // one more image plus its lists and statistics, and the counters of this call: asked of the device before anything is allocated
    const double image = (double)ncg * (double)nbp * 1024.0;
    const double rest = 16.0 * (double)p + 8.0 * (double)(p + 1) + 4.0 * (double)src->total_missing      // mu, sinv, the lists
                      + 12.0 * (double)p + (src->total_missing > 0 ? 16.0 * (double)src->p + 4.0 * (double)src->n : 0.0);
    size_t free_b = 0, total_b = 0;
    MIH_HIP(hipMemGetInfo(&free_b, &total_b));
    if (image + rest > (double)free_b && trim_score_images(src->device) > 0) MIH_HIP(hipMemGetInfo(&free_b, &total_b));
    if (image + rest > (double)free_b) {
        set_error("mih_snp_transpose: the image of the %lld x %lld transposed matrix needs %.0f bytes of device memory and its lists, statistics "
                  "and counters %.0f more, %.0f bytes are free", (long long)n, (long long)p, image, rest, (double)free_b);
        return MIH_OOM;
    }

    DevBuf<int32_t> cnt, cnt4, rm;
    MIH_TRY(cnt.alloc((size_t)(3 * p)));
    if (src->total_missing > 0) {
        MIH_TRY(cnt4.alloc((size_t)(4 * src->p)));
        MIH_TRY(rm.alloc((size_t)src->n));
    }
    mih_mat *h = new mih_mat();
    h->kind = 0; h->device = src->device; h->n = n; h->p = p;
    h->center = center; h->scale = scale; h->impute = impute;
    auto fail = [&](int code) { mih_mat_destroy(h); return code; };
    int rc = alloc_snp(h);
    if (rc) return fail(rc);
    if (hipStreamCreate(&h->stream) != hipSuccess) return fail(MIH_HIP_ERROR);
    if (hipStreamSynchronize(src->stream) != hipSuccess) return fail(MIH_HIP_ERROR);      // whatever was queued on the source has finished
    hipStream_t s = h->stream;
    if (hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * 3 * (size_t)p, s) != hipSuccess) return fail(MIH_HIP_ERROR);
    hipLaunchKernelGGL(k_transpose_tiles, dim3((unsigned)(src->nbp * nchunk)), dim3(64), 0, s, reinterpret_cast<const uint4 *>(src->X), src->ncg,
                       src->nbp, src->n, reinterpret_cast<uint4 *>(h->X), ncg, nbp, nchunk, cnt.p);
    if (src->total_missing > 0) {                                  // (a matrix without missing genotypes: no scatter, no list kernel)
        if (hipMemsetAsync(cnt4.p, 0, sizeof(int32_t) * 4 * (size_t)src->p, s) != hipSuccess ||
            hipMemsetAsync(rm.p, 0, sizeof(int32_t) * (size_t)src->n, s) != hipSuccess) return fail(MIH_HIP_ERROR);
        launch_missing_counts(src, nullptr, nullptr, cnt4.p, rm.p, s);
        hipLaunchKernelGGL(k_place_missing, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, s, rm.p, p, cnt.p);
        const int64_t slab = 1ll << 30;
        for (int64_t j0 = 0; j0 < src->p; j0 += slab)
            hipLaunchKernelGGL(k_transpose_missing, dim3((unsigned)std::min(slab, src->p - j0)), dim3(64), 0, s, src->miss_ptr, src->miss_row, j0,
                               h->X, nbp);
    }
    if ((rc = finish_tiles(h, cnt.p))) {                           // mu, sinv, the ascending lists; code 3 back to code 0
        set_error("the transpose kernels failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(rc);
    }
    if (h->total_missing != src->total_missing) {
        set_error("mih_snp_transpose: %lld missing genotypes listed, the source has %lld", (long long)h->total_missing, (long long)src->total_missing);
        return fail(MIH_HIP_ERROR);
    }
    if (reserve_bytes == 0) reserve_fit_memory(h);
    else if (reserve_bytes > 0) reserve_fit_memory(h, true, (size_t)reserve_bytes);
    *out = h;
    return MIH_OK;
}

}  // extern "C"
