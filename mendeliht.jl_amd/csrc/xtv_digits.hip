// xtv_digits.hip -- the residual statistics and the residual's fixed-point digit planes (the B operands of xtv.hip's passes)
#include "common.h"
#include "peel.h"

namespace mih {

// ---- residual -> fixed-point digit planes -------------------------------------------------
// scal[4v + 0] = max|r_v|, scal[4v + 1] = 2^-e, scal[4v + 2] = sum r_v, scal[4v + 3] = 2^e
// The block that finishes last (a counter per residual, left at zero again) adds up the partials in block order and
// writes scal: one launch instead of two; the sums do not depend on which block that is.
__global__ void __launch_bounds__(256)
k_r_stats(const double *__restrict__ r, int64_t n, int m, double *__restrict__ part /* [m][gridDim.x][2] */,
          unsigned *__restrict__ done /* [m], zero */, int ebits, double *__restrict__ scal,
          const int32_t *__restrict__ gate, int32_t gate_val, double *__restrict__ peel /* [m][kPeelStride], or null */)
{
    if (gate && *gate != gate_val) return;
    __shared__ double smax[256], ssum[256];
    __shared__ bool last;
    const int v = blockIdx.y;                    // one grid row per residual
    double mx = 0.0, sm = 0.0;
    // eight rows of the thread's walk in flight (the residual is cold after the pass: one load at a time was a round trip per row,
    // 30 of them at n = 500 000); the additions stay in the order of the walk
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += 8 * stride) {
        double x8[8];
        #pragma unroll
        for (int u = 0; u < 8; ++u) x8[u] = (i + u * stride < n) ? r[(int64_t)v * n + i + u * stride] : 0.0;
        #pragma unroll
        for (int u = 0; u < 8; ++u) if (i + u * stride < n) { mx = fmax(mx, fabs(x8[u])); sm += x8[u]; }
    }
    smax[threadIdx.x] = mx; ssum[threadIdx.x] = sm;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) { smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + k]); ssum[threadIdx.x] += ssum[threadIdx.x + k]; }
        __syncthreads();
    }
    const int nblocks = (int)gridDim.x;
    if (threadIdx.x == 0) {
        part[((int64_t)v * nblocks + blockIdx.x) * 2] = smax[0]; part[((int64_t)v * nblocks + blockIdx.x) * 2 + 1] = ssum[0];
        __threadfence();
        last = atomicAdd(&done[v], 1u) == (unsigned)nblocks - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // (round 6) the outlier side channel (peel.h): the whole block looks at the block maxima; rows that tower over the rest leave the
    // fixed-point residual and the scale is taken from what is left.  No outlier (every residual so far): `top` is max|r|, as before.
    double top = -1.0;
    if (peel) {
        const int64_t nb64 = (n + 255) / 256;
        top = peel_decide(r + (int64_t)v * n, n, part + (int64_t)v * nblocks * 2, (int)(nb64 < nblocks ? nb64 : nblocks), peel + (int64_t)v * kPeelStride);
    }
    if (threadIdx.x == 0) {
        double fmx = 0.0, fsm = 0.0;
        for (int b = 0; b < nblocks; ++b) {
            fmx = fmax(fmx, __hip_atomic_load(&part[((int64_t)v * nblocks + b) * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            fsm += __hip_atomic_load(&part[((int64_t)v * nblocks + b) * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (top < 0.0) top = fmx;
        // exponent e with top * 2^e < 2^(ebits+1) (DigitMode::ebits); an all-zero (or non-finite) residual keeps e = 0.  Every FINITE
        // top has its exponent (e >= ebits - 1023: 2^e and 2^-e are finite); the same rule in k_digits' stats hook below
        int e = 0;
        if (top > 0.0 && top <= kMaxFinite) e = ebits - ilogb(top);
        if (e > 1000) e = 1000;          // a (numerically zero) residual below 2^-947: keep 2^e finite
        scal[4 * v + 0] = fmx;
        scal[4 * v + 1] = ldexp(1.0, -e);
        scal[4 * v + 2] = fsm;
        scal[4 * v + 3] = ldexp(1.0, e);
        done[v] = 0;
    }
}

// digit of residue m (0..12) in the base-13 system: {-8,-6,-4..4,6,8} is a complete residue system mod 13 whose
// halves are all FP4 (e2m1) numbers; every |R| <= 2^57 has a 16-digit representation (|R| <= 2^27: 8 digits)
__device__ __forceinline__ int digit13(int m)
{
    return m <= 4 ? m : m >= 9 ? m - 13 : m == 5 ? -8 : m == 6 ? 6 : m == 7 ? -6 : 8;
}
// base 49: residues 0..16 and 33..48 (= -16..-1) directly, 17..32 as the even number itself or the odd number
// minus 49 (-32..-18, even): all of them eighths that FP6 (e2m3) represents; |R| <= 2^54 has 10 digits, 2^43 has 8
__device__ __forceinline__ int digit49(int m)
{
    return m <= 16 ? m : m >= 33 ? m - 49 : (m & 1) ? m - 49 : m;
}

// grid (ceil(nblk / 4), residual slots).  One thread per row turns the scaled residual into its digits (FP4 code of
// d/2 or FP6 code of d/8, packed 16 x 4 or 10 x 6 bits per 64-bit word); the 64 rows of a block are then
// transposed through LDS into the B-operand fragment: column sub*slots + t of operand v / per_op holds digit t of
// residual v, lane 32*h + column carries the 32 rows of half h (element order identical to the A fragment built in
// mfma_fp4; an FP6 element j sits in bits 6j..6j+5 of the lane's 192 bits, the last 64 of them in `dig2`).
__global__ void __launch_bounds__(256)
k_digits(const double *__restrict__ r, int64_t n, int64_t nblk, int m, DigitMode dm,
         double *scal, uint4 *__restrict__ dig /* [nops][nblk][64] */, uint2 *__restrict__ dig2, FlatPasses fp, XtvStatsHook sh,
         const double *__restrict__ peel /* [m][kPeelStride]: rows that left the fixed-point residual (peel.h), or null */)
{
    // The wave's 64 rows go into the B-operand image of their block directly: img[wave][half][digit] is the 128 (FP4) or 192 (FP6)
    // bits lane (half, digit) of the fragment carries, and every row ORs its code into its element's place (LDS atomics; round 4 --
    // before, the 2 x slots lanes that own an image gathered it with 32 LDS reads and 64-bit shifts each while the other 44 idled:
    // 60 % of the kernel's time at ten digits).
    if (dm.gate && *dm.gate != dm.gate_val) return;
    __shared__ uint32_t img[4][2][32][6];
    __shared__ double s_scale;
    if (sh.spart) {           // (device-resident steps, one residual) k_r_stats's second stage, by every block for itself; block 0 also leaves it -- and Z'r
        if (threadIdx.x == 0) {
            double fmx = 0.0, fsm = 0.0;
            for (int b = 0; b < 64; ++b) { fmx = fmax(fmx, sh.spart[2 * b]); fsm += sh.spart[2 * b + 1]; }
            const double top = (peel && peel[0] > 0.0) ? peel[2] : fmx;       // (k_res_peel took rows out: the scale of the rest)
            int e = 0;
            if (top > 0.0 && top <= kMaxFinite) e = sh.ebits - ilogb(top);
            if (e > 1000) e = 1000;
            s_scale = ldexp(1.0, e);
            if (blockIdx.x == 0) { scal[0] = fmx; scal[1] = ldexp(1.0, -e); scal[2] = fsm; scal[3] = ldexp(1.0, e); }
        }
        if (blockIdx.x == 0 && (int)threadIdx.x >= 64 && (int)threadIdx.x < 64 + sh.q) {
            const int l = threadIdx.x - 64;
            double a = 0.0;
            for (int b = 0; b < sh.zblocks; ++b) a += sh.zpart[(int64_t)l * sh.zblocks + b];
            sh.df2[l] = a;
        }
        __syncthreads();
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t blk = blockIdx.x * 4ll + w;
    const int vs = blockIdx.y;
    const int slots = dm.slots, op = vs / dm.per_op, sub = vs % dm.per_op;
    const bool fp6 = dm.base == 49;
    {
        uint32_t *z = &img[w][0][0][0];
        #pragma unroll
        for (int e = 0; e < 6; ++e) z[e * 64 + lane] = 0u;
    }
    __syncthreads();
    if (vs < m && blk < nblk) {
        const int64_t i = blk * 64 + lane;
        double x = (i < n) ? r[(int64_t)vs * n + i] : 0.0;
        if (peel) {                                     // a peeled row's digits are zero: k_xtv_finalize adds its term in f64
            const double *pl = peel + (int64_t)vs * kPeelStride;
            if (pl[0] > 0.0 && fabs(x) > pl[1]) x = 0.0;
        }
        long long R = __double2ll_rn(x * (sh.spart ? s_scale : scal[4 * vs + 3]));
        // element of this row in its half's fragment (the A fragment's order, mfma_fp4): 8 (2u + (s & 1)) + (s >> 1) for row 16u + s
        const int hh = lane >> 5, uu = (lane >> 4) & 1, ss = lane & 15;
        const int el = 8 * (2 * uu + (ss & 1)) + (ss >> 1);
        const int bit = (fp6 ? 6 : 4) * el, dwd = bit >> 5, sh = bit & 31;
        uint32_t *mine = &img[w][hh][0][0];
        // base 49: the standard digits of |R| come from two 5-digit limbs (49^5 < 2^29: 32-bit divisions instead of ten 64-bit
        // ones) and carry into the balanced residue system; the system is symmetric, digits(-R) = -digits(R)
        const bool neg = R < 0;
        const unsigned long long aR = neg ? 0ull - (unsigned long long)R : (unsigned long long)R;
        uint32_t limb_hi = (uint32_t)(aR / 282475249ull), limb_lo = (uint32_t)(aR - (unsigned long long)limb_hi * 282475249ull);
        int carry = 0;
        if (dm.base == 4) {
            // (round 5) all 28 balanced base-4 digits at once: with d_t in {-2,-1,0,1}, R + sum_t 2 * 4^t = sum_t (d_t + 2) 4^t has the
            // ORDINARY base-4 digits u_t = d_t + 2 in {0..3} -- the representation is unique, so these are the digits the division
            // loop below produces -- and the FP4 (e2m1) code of d_t / 2 is a four-entry table: u = 0 -> -1.0 (1010), 1 -> -0.5 (1001),
            // 2 -> 0, 3 -> +0.5 (0001).  No loop-carried dependency.
            const unsigned long long U = (unsigned long long)R + 0x00AAAAAAAAAAAAAAull;
            if (dm.hom_u && vs == 0) dm.hom_u[i] = U;        // a pass over the score image follows: k_xtv_hom sums these digits (a peeled or pad row: all d_t = 0)
            for (int t = 0; t < dm.ndig; ++t) {
                const uint32_t u = (uint32_t)(U >> (2 * t)) & 3u;
                const uint32_t code = (0x109Au >> (4u * u)) & 15u;
                if (code) atomicOr(mine + t * 6 + dwd, code << sh);
            }
        } else
        for (int t = 0; t < dm.ndig; ++t) {
            int d;
            if (dm.base == 49) {
                const uint32_t L = t < 5 ? limb_lo : limb_hi, qd = L / 49u;
                const int v = (int)(L - qd * 49u) + carry;
                if (t < 5) limb_lo = qd; else limb_hi = qd;
                if (v == 49) { d = 0; carry = 1; }
                else { d = digit49(v); carry = d < 0; }
                if (neg) d = -d;
            } else if (dm.base == 4) {
                const int mm = (int)(R & 3);
                d = mm < 2 ? mm : mm - 4;
                R = (R - d) >> 2;
            } else {
                int mm = (int)(R % 13);
                if (mm < 0) mm += 13;
                d = digit13(mm);
                R = (R - d) / 13;
            }
            const unsigned a = (unsigned)(d < 0 ? -d : d);
            uint32_t code;
            if (fp6) code = (a < 8 ? a : a < 16 ? a : a <= 30 ? 8u + (a >> 1) : 16u + (a >> 2)) | (d < 0 ? 32u : 0u);   // e2m3 of a/8
            else code = (a <= 4 ? a : a == 6 ? 5u : 6u) | (d < 0 ? 8u : 0u);                                          // e2m1 of a/2
            if (code) {
                atomicOr(mine + t * 6 + dwd, code << sh);
                if (sh > 26) atomicOr(mine + t * 6 + dwd + 1, code >> (32 - sh));       // (an FP6 code across a dword boundary)
            }
        }
    }
    __syncthreads();
    if (blk < nblk && lane < 2 * slots) {
        const int h = lane / slots, dg = lane % slots;
        int64_t o = ((int64_t)op * nblk + blk) * 64 + h * 32 + sub * slots + dg;
        if (dm.lay16) {       // image b = column / 16 of the 128-row block, lane 16 * (e + 2h) + column % 16 (k_xtv_dma16)
            int col = sub * slots + dg, opc = op;
            if (dm.flat) {    // digit dg of residual vs sits in column 10 (vs - u0) + dg of its pass, counted across the pass's operands
                int q = 0;
                while (q + 1 < fp.npass && vs >= fp.u0[q + 1]) ++q;
                const int cg = (vs - fp.u0[q]) * slots + dg;
                opc = fp.t0[q] + (cg >> 5); col = cg & 31;
            }
            const int e = (int)(blk & 1);
            o = ((int64_t)opc * nblk + (blk - e) + (col >> 4)) * 64 + 16 * (e + 2 * h) + (col & 15);
        }
        const uint32_t *q = &img[w][h][dg][0];
        dig[o] = make_uint4(q[0], q[1], q[2], q[3]);
        if (fp6) dig2[o] = make_uint2(q[4], q[5]);
    }
}

void launch_r_stats(const double *r_dev, int64_t n, int m, double *part, unsigned *done, int ebits, double *scal,
                    const int32_t *gate, int32_t gate_val, double *peel, hipStream_t s)
{
    hipLaunchKernelGGL(k_r_stats, dim3(kStatBlocks, (unsigned)m), dim3(256), 0, s, r_dev, n, m, part, done, ebits, scal, gate, gate_val, peel);
}

void launch_digits(const double *r_dev, int64_t n, int64_t nblk, int m, int slots, const DigitMode &dm, double *scal, uint4 *dig, uint2 *dig2,
                   const FlatPasses &fp, const XtvStatsHook &sh, const double *peel, hipStream_t s)
{
    hipLaunchKernelGGL(k_digits, dim3((unsigned)((nblk + 3) / 4), (unsigned)slots), dim3(256), 0, s, r_dev, n, nblk, m, dm, scal, dig, dig2, fp, sh, peel);
}

}  // namespace mih
