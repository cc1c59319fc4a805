// assoc.hip -- the marginal association scan (mih_assoc_score): one null model on the covariates, then a GLM score test of every
// column of the matrix by itself, for up to 32 traits at once.  tests/assoc_spec.py states the definitions in numpy.
//
// Per column j the test needs U_js = sum_i x_ij A_is, b_j = sum_i x_ij w_i Z_i. and Q_j = sum_i x_ij^2 w_i.  The linear terms are
// the library's fused X'R pass over R = [A | w o Z]; new here is the quadratic term under non-constant weights.  A 2-bit column
// takes four values, so Q_j is four class-weight sums, and two of them come off the matrix cores without a decode: codes are
// 01 = dosage 1 and 10 = dosage 2 (11 never occurs), so tile & 0x11111111 is the FP4 plane 0.5 [g = 1] and tile & 0x22222222 the
// FP4 plane 1.0 [g = 2] under the expansion mfma_fp4 applies with 0x33333333 (the trick of ld.hip).  Multiplied against the FP4
// digit planes of the fixed-point weights they give, per base-4 digit, the exact integer sum of that digit over the rows of the
// class.  Everything up to one rounding per class sum is an integer: no result depends on how the rows are cut into slices.
#include "grm.h"
#include "normal_tail.h"
#include "assoc.h"
#include <algorithm>
#include <cmath>
#include <limits>

namespace mih {

typedef float as_f32x16 __attribute__((ext_vector_type(16)));
typedef int as_i32x8 __attribute__((ext_vector_type(8)));

constexpr int kAssocDigits = 28;                 // digit columns of the weights' B operand (27 carry digits: R < 2^54)
constexpr int kAssocEbits = 53;                  // max w * 2^e < 2^54
// Rows of a slice.  The digits are the ORDINARY base-4 digits u in {0, 1, 2, 3} of R_i = rint(w_i 2^e) >= 0: u / 2 is the FP4
// number whose code is u itself.  A row adds 0.5 u / 2 (dosage 1) or 1.0 u / 2 (dosage 2) to an accumulator: a multiple of 1/4,
// at most 1.5 = six quarters.  An f32 accumulator holds every multiple of 1/4 up to 2^24 quarters, so a slice of at most
// floor(2^24 / 6) = 2 796 202 rows is exact; in whole tiles 21 845 block pairs = 2 796 160 rows.
constexpr int64_t kAssocSliceBp = 21845;
constexpr int64_t kAssocWaves = 8192;            // work items a launch should have: 8 waves on each of the 1024 SIMDs
constexpr int64_t kAssocMinBp = 32;              // ... but no slice shorter than 4096 rows

// an unsigned 128-bit integer in two words: the class sums sum_t 4^t S_t reach 2^54 n
struct U128 { unsigned long long hi, lo; };
__host__ __device__ inline U128 u128_add(U128 a, U128 b) { U128 r; r.lo = a.lo + b.lo; r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull); return r; }
__host__ __device__ inline U128 u128_sub(U128 a, U128 b) { U128 r; r.lo = a.lo - b.lo; r.hi = a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull); return r; }
__host__ __device__ inline U128 u128_shl(unsigned long long v, int s)      // v << s, 0 <= s < 64
{
    U128 r; r.lo = v << s; r.hi = s ? v >> (64 - s) : 0ull; return r;
}
// the nearest double of v 2^-e (ties to even): the top 64 bits with everything below folded into the last of them are converted
// by one correctly rounded instruction (at least 11 bits sit below the 53 it keeps), the scaling is by a power of two
__host__ __device__ inline double u128_scaled(U128 v, int e)
{
    if (v.hi == 0) return ldexp((double)v.lo, -e);
    int lz = 0;
    for (unsigned long long t = v.hi; !(t >> 63); t <<= 1) ++lz;          // v.hi != 0
    const int sh = 64 - lz;                                              // bits of v.lo that drop out, 1 .. 64
    unsigned long long top = sh == 64 ? v.hi : (v.hi << lz) | (v.lo >> sh);
    const unsigned long long rest = sh == 64 ? v.lo : v.lo << lz;
    if (rest) top |= 1ull;
    return ldexp((double)top, sh - e);
}

// ---- 1. the front ends ---------------------------------------------------------------------------------------------------------------
// R = [A | w o Z], n x (t + c) column-major
__global__ void __launch_bounds__(256)
k_assoc_rhs(const double *__restrict__ A, const double *__restrict__ w, const double *__restrict__ Z, int64_t n, int t, int c, double *__restrict__ R)
{
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    const int v = blockIdx.y;
    if (i >= n) return;
    R[(int64_t)v * n + i] = v < t ? A[(int64_t)v * n + i] : w[i] * Z[(int64_t)(v - t) * n + i];
}

// The B operand of the weights: dig[blk 64 + 32 h + d] carries, for the 64-row block blk and its half h, base-4 digit d of the 32
// rows 64 blk + 32 h + (0 .. 31) in the element order of the A fragment (8 (2 u + (s & 1)) + (s >> 1) for row 16 u + s, as
// k_digits writes it); the columns d >= 28 and the rows >= n are zero.  One thread per lane of the operand.
__global__ void __launch_bounds__(256)
k_assoc_digits(const unsigned long long *__restrict__ R, int64_t n, int64_t nblk, uint4 *__restrict__ dig)
{
    const int64_t idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= nblk * 64) return;
    const int64_t blk = idx >> 6;
    const int lane = (int)(idx & 63), h = lane >> 5, d = lane & 31;
    uint32_t q[4] = {0u, 0u, 0u, 0u};
    if (d < kAssocDigits) {
        for (int rr = 0; rr < 32; ++rr) {
            const int64_t i = blk * 64 + 32 * h + rr;
            if (i >= n) break;
            const uint32_t u = (uint32_t)(R[i] >> (2 * d)) & 3u;
            const int uu = rr >> 4, s = rr & 15, el = 8 * (2 * uu + (s & 1)) + (s >> 1);
            q[el >> 3] |= u << (4 * (el & 7));
        }
    }
    dig[idx] = make_uint4(q[0], q[1], q[2], q[3]);
}

// ---- 2. the class kernel ---------------------------------------------------------------------------------------------------------------
// one class plane of the two dwords of a lane that cover 64 rows (M = 0x11111111: 0.5 [g = 1], M = 0x22222222: 1.0 [g = 2])
// against a digit operand
__device__ __forceinline__ as_f32x16 assoc_mfma(uint32_t a0, uint32_t a1, uint32_t M, const uint4 &b, as_f32x16 acc)
{
    as_i32x8 a = {(int)(a0 & M), (int)((a0 >> 2) & M), (int)(a1 & M), (int)((a1 >> 2) & M), 0, 0, 0, 0};
    as_i32x8 bb = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bb, acc, 4, 4, 0, 0, 0, 0);
}

// A wave's work item: (pair of column groups 2 gp, 2 gp + 1, row slice sl), item = gp nsl + sl -- two groups a wave, so that a
// digit operand fetched from the cache serves two tiles.  It walks the slice's block pairs with the tiles and the digit operands
// of the next two steps in flight (the last steps load the last tile again: no branch around the accumulators), four MFMAs per tile, and
// leaves, as integers,
//     part[(((sl ncg + cg) 2 + k) 32 + m) 32 + d] = sum over the slice's rows with g_i,32 cg + m = k + 1 of digit d of R_i
// (k = 0: 4 acc, k = 1: 2 acc).  D layout of the instruction: column d = lane & 31, row m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// Plain stores, every entry written by one lane.  An odd last group is computed twice and stored once.
__global__ void __launch_bounds__(256)
k_assoc_classes(const uint4 *__restrict__ X, const uint4 *__restrict__ dig, int64_t nbp, int64_t ncg, int64_t bps, int nsl,
                int32_t *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t item = blockIdx.x * 4ll + (threadIdx.x >> 6);
    const int64_t ngp = (ncg + 1) / 2;
    if (item >= ngp * nsl) return;
    const int sl = (int)(item % nsl);
    const int64_t cg0 = 2 * (item / nsl), cg1 = min(cg0 + 1, ncg - 1);
    const int64_t b0 = sl * bps, b1 = min(nbp, b0 + bps);
    const uint4 *xa = X + cg0 * nbp * 64 + lane, *xb = X + cg1 * nbp * 64 + lane, *dg = dig + lane;

    as_f32x16 acc[2][2];
    #pragma unroll
    for (int g = 0; g < 2; ++g)
        #pragma unroll
        for (int k = 0; k < 2; ++k)
            #pragma unroll
            for (int r = 0; r < 16; ++r) acc[g][k][r] = 0.f;
    // two steps ahead: a wave keeps 4 KB of tiles and 4 KB of digit operands in flight beside the step it multiplies
    const int64_t s1 = min(b0 + 1, b1 - 1);
    uint4 ta = xa[b0 * 64], tb = xb[b0 * 64], d0 = dg[b0 * 128], d1 = dg[b0 * 128 + 64];
    uint4 ua = xa[s1 * 64], ub = xb[s1 * 64], e0 = dg[s1 * 128], e1 = dg[s1 * 128 + 64];
    for (int64_t bp = b0; bp < b1; ++bp) {
        const int64_t nx = min(bp + 2, b1 - 1);
        const uint4 na = xa[nx * 64], nb = xb[nx * 64], n0 = dg[nx * 128], n1 = dg[nx * 128 + 64];
        acc[0][0] = assoc_mfma(ta.x, ta.y, 0x11111111u, d0, acc[0][0]);
        acc[0][1] = assoc_mfma(ta.x, ta.y, 0x22222222u, d0, acc[0][1]);
        acc[1][0] = assoc_mfma(tb.x, tb.y, 0x11111111u, d0, acc[1][0]);
        acc[1][1] = assoc_mfma(tb.x, tb.y, 0x22222222u, d0, acc[1][1]);
        acc[0][0] = assoc_mfma(ta.z, ta.w, 0x11111111u, d1, acc[0][0]);
        acc[0][1] = assoc_mfma(ta.z, ta.w, 0x22222222u, d1, acc[0][1]);
        acc[1][0] = assoc_mfma(tb.z, tb.w, 0x11111111u, d1, acc[1][0]);
        acc[1][1] = assoc_mfma(tb.z, tb.w, 0x22222222u, d1, acc[1][1]);
        ta = ua; tb = ub; d0 = e0; d1 = e1;
        ua = na; ub = nb; e0 = n0; e1 = n1;
    }

    #pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int64_t cg = cg0 + g;
        if (cg >= ncg) break;
        int32_t *out = part + (((int64_t)sl * ncg + cg) * 2) * 1024 + (lane & 31);
        #pragma unroll
        for (int k = 0; k < 2; ++k)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                out[k * 1024 + m * 32] = (int32_t)(acc[g][k][r] * (k == 0 ? 4.f : 2.f));
            }
    }
}

// Wm: the sum of R over the column's missing rows, one wave per column, as two 64-bit sums of the rows' low and high 32 bits
// (integers: the order of the additions does not matter).  tm[2 j] = sum of low halves, tm[2 j + 1] = sum of high halves.
__global__ void __launch_bounds__(256)
k_assoc_missing(const int64_t *__restrict__ miss_ptr, const int32_t *__restrict__ miss_row, const unsigned long long *__restrict__ R,
                int64_t p, unsigned long long *__restrict__ tm)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (j >= p) return;
    unsigned long long lo = 0, hi = 0;
    for (int64_t t = miss_ptr[j] + lane, e = miss_ptr[j + 1]; t < e; t += 64) {
        const unsigned long long r = R[miss_row[t]];
        lo += r & 0xFFFFFFFFull; hi += r >> 32;
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo += __shfl_xor(lo, off, 64); hi += __shfl_xor(hi, off, 64); }
    if (lane == 0) { tm[2 * j] = lo; tm[2 * j + 1] = hi; }
}

// One thread per column: the slices' digit sums added per digit in int64, the digits recombined once (digit 0 upward) into the
// exact integers T1, T2; Tm from k_assoc_missing; T0 = sum_i R_i - T1 - T2 - Tm.  Each becomes a double by ONE rounding:
// Wc[4 j ..] = W0, W1, W2, Wm in the weights' own unit.
__global__ void __launch_bounds__(256)
k_assoc_wsum(const int32_t *__restrict__ part, int nsl, int64_t ncg, int64_t p, const unsigned long long *__restrict__ tm,
             unsigned long long rsum_hi, unsigned long long rsum_lo, int e, double *__restrict__ Wc)
{
    const int64_t j = blockIdx.x * 256ll + threadIdx.x;
    if (j >= p) return;
    const int64_t cg = j >> 5;
    const int m = (int)(j & 31);
    U128 T[2];
    for (int k = 0; k < 2; ++k) {
        U128 acc = {0ull, 0ull};
        for (int d = 0; d < kAssocDigits; ++d) {
            long long sd = 0;
            for (int sl = 0; sl < nsl; ++sl) sd += part[((((int64_t)sl * ncg + cg) * 2 + k) * 32 + m) * 32 + d];
            acc = u128_add(acc, u128_shl((unsigned long long)sd, 2 * d));
        }
        T[k] = acc;
    }
    const U128 Tm = u128_add(U128{0ull, tm[2 * j]}, u128_shl(tm[2 * j + 1], 32));
    const U128 T0 = u128_sub(u128_sub(u128_sub(U128{rsum_hi, rsum_lo}, T[0]), T[1]), Tm);
    Wc[4 * j] = u128_scaled(T0, e); Wc[4 * j + 1] = u128_scaled(T[0], e); Wc[4 * j + 2] = u128_scaled(T[1], e); Wc[4 * j + 3] = u128_scaled(Tm, e);
}

// ---- 3. Q ------------------------------------------------------------------------------------------------------------------------------
// 2-bit: the four values of a column as k_xtv_finalize multiplies them (k_ib_solve's expressions), squared, times the class sums,
// in the order tests/assoc_spec.py writes it
__global__ void __launch_bounds__(256)
k_assoc_q_snp(const double *__restrict__ Wc, const double *__restrict__ mu, const double *__restrict__ sinv, int center, int scale, int impute,
              int64_t p, double *__restrict__ Q)
{
#pragma clang fp contract(off)
    const int64_t j = blockIdx.x * 256ll + threadIdx.x;
    if (j >= p) return;
    const double m = mu[j], s = scale ? sinv[j] : 1.0, cm = center ? m : 0.0;
    const double x0 = (0.0 - cm) * s, x1 = (1.0 - cm) * s, x2 = (2.0 - cm) * s, xm = ((impute ? m : 0.0) - cm) * s;
    double q = (x0 * x0) * Wc[4 * j];
    q = q + (x1 * x1) * Wc[4 * j + 1];
    q = q + (x2 * x2) * Wc[4 * j + 2];
    q = q + (xm * xm) * Wc[4 * j + 3];
    Q[j] = q;
}

// dense f64 / f32 and 16-bit dosage handles: one block per column, every thread its rows in ascending order, then a fixed tree
template <int KIND>      // 0: f64, 1: f32, 2: dosage
__global__ void __launch_bounds__(256)
k_assoc_q_dense(const double *__restrict__ D, const float *__restrict__ Df, DosageView dv, const double *__restrict__ w, int64_t n,
                double *__restrict__ Q)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int64_t j = blockIdx.x;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double x = KIND == 0 ? D[j * n + i] : KIND == 1 ? (double)Df[j * n + i] : dosage_x(dv, j, i);
        v = v + (x * x) * w[i];
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) Q[j] = red[0];
}

// ---- 4. the finish ---------------------------------------------------------------------------------------------------------------------
// V_j = Q_j - |L^-1 b_j|^2, one thread per column: u_k = sum_{l <= k} Linv[k][l] b_l (l ascending), r2 += u_k u_k (k ascending).
// S: p x (t + c), the columns t .. t + c - 1 are b.  Linv: c x c row-major.  NaN for a degenerate column and where V <= 0.
__global__ void __launch_bounds__(256)
k_assoc_var(const double *__restrict__ S, int64_t p, int t, int c, const double *__restrict__ Linv, const double *__restrict__ Q,
            const uint8_t *__restrict__ degenerate, double *__restrict__ V)
{
#pragma clang fp contract(off)
    const int64_t j = blockIdx.x * 256ll + threadIdx.x;
    if (j >= p) return;
    double r2 = 0.0;
    for (int k = 0; k < c; ++k) {
        double u = 0.0;
        for (int l = 0; l <= k; ++l) u = u + Linv[k * c + l] * S[(int64_t)(t + l) * p + j];
        r2 = r2 + u * u;
    }
    const double v = Q[j] - r2;
    V[j] = (degenerate[j] || !(v > 0.0)) ? std::numeric_limits<double>::quiet_NaN() : v;
}

// one thread per (j, s): z = U / sqrt V, beta = U / V, se = 1 / sqrt V (written by s = 0)
__global__ void __launch_bounds__(256)
k_assoc_finish(const double *__restrict__ S, const double *__restrict__ V, int64_t p, int t, double *__restrict__ z,
               double *__restrict__ beta, double *__restrict__ se)
{
#pragma clang fp contract(off)
    const int64_t idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= p * t) return;
    const int64_t j = idx % p;
    const double v = V[j], u = S[idx], rt = sqrt(v);
    const bool bad = v != v;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    z[idx] = bad ? nan : u / rt;
    beta[idx] = bad ? nan : u / v;
    if (idx < p) se[j] = bad ? nan : 1.0 / rt;
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------
static bool all_finite(const double *x, size_t len)
{
    for (size_t i = 0; i < len; ++i) if (!std::isfinite(x[i])) return false;
    return true;
}

// G = Z'WZ = L L' (unpivoted Cholesky, f64), Linv = L^-1 (c x c row-major, lower); false: G is not positive definite
static bool assoc_null_factor(const double *Z, const double *w, int64_t n, int c, std::vector<double> &Linv)
{
    std::vector<double> G((size_t)c * c, 0.0), wz((size_t)n);
    for (int k = 0; k < c; ++k) {
        for (int64_t i = 0; i < n; ++i) wz[(size_t)i] = (w ? w[i] : 1.0) * Z[(size_t)k * n + i];
        for (int l = 0; l <= k; ++l) {
            double a = 0.0;
            const double *zl = Z + (size_t)l * n;
            for (int64_t i = 0; i < n; ++i) a += wz[(size_t)i] * zl[i];
            G[(size_t)k * c + l] = a;
        }
    }
    std::vector<double> L((size_t)c * c, 0.0);
    for (int k = 0; k < c; ++k) {
        for (int l = 0; l <= k; ++l) {
            double a = G[(size_t)k * c + l];
            for (int q = 0; q < l; ++q) a -= L[(size_t)k * c + q] * L[(size_t)l * c + q];
            if (l == k) {
                if (!(a > 0.0) || !std::isfinite(a)) return false;
                L[(size_t)k * c + k] = std::sqrt(a);
            } else L[(size_t)k * c + l] = a / L[(size_t)l * c + l];
        }
    }
    Linv.assign((size_t)c * c, 0.0);
    for (int col = 0; col < c; ++col) {              // forward substitution L x = e_col
        for (int k = col; k < c; ++k) {
            double a = k == col ? 1.0 : 0.0;
            for (int q = col; q < k; ++q) a -= L[(size_t)k * c + q] * Linv[(size_t)q * c + col];
            Linv[(size_t)k * c + col] = a / L[(size_t)k * c + k];
        }
    }
    return all_finite(Linv.data(), Linv.size());
}

static unsigned blocks_of(int64_t items) { return (unsigned)((items + 255) / 256); }

// A call as its entry point states it: mih_assoc_score's arguments, and what the other three add (nullptr: that pass does not run)
struct AssocCall {
    const mih_mat *h; const double *A; int32_t t; const double *w, *Z; int32_t c; int64_t slice_rows;
    double *z, *beta, *se, *neglog10p, *wsum;
    const SpaCall *spa; const FirthCall *firth; const SetsCall *sets;
    // the entry point that the texts about eta, the cutoff and the selection name
    const char *who() const { return firth ? "mih_assoc_score_firth" : "mih_assoc_score_spa"; }
    const double *eta() const { return firth ? firth->eta : spa ? spa->eta : nullptr; }
};

// What the steps of a call hand on to the later ones, each group filled by the step named beside it.  The host arrays that an
// asynchronous upload reads live here, until the call returns.
struct AssocWork {
    double wmax = 0.0;                           // assoc_refuse
    std::vector<double> Linv;
    bool snp = false, classes = false;           // assoc_slice_plan: a 2-bit handle; ... with weights, which takes the class kernel
    int64_t bps = 0, nsl = 1;                    // block pairs of a row slice, slices
    std::vector<uint8_t> deg;                    // assoc_degenerate
    std::vector<int32_t> counts;
    int e = 0;                                   // assoc_fixed_weights
    std::vector<unsigned long long> Rw;
    U128 rsum = {0ull, 0ull};
    DevBuf<double> Ad, Zd, wd, R, S, Q, V, Ld, Wc, zd, bd, sd;     // assoc_linear; Wc, Rd, tm, dig, part: assoc_q
    DevBuf<uint8_t> degd;
    DevBuf<unsigned long long> Rd, tm;
    DevBuf<uint32_t> dig;
    DevBuf<int32_t> part;
    XtvWork xw;
    std::vector<double> ones;
    std::vector<double> hz, hb, hs, hw, hn;      // assoc_finish: z, beta, se, the class sums, neglog10p on the host
};

// ---- refusals: host only, nothing allocated, nothing written ----
static int assoc_refuse(const AssocCall &a, AssocWork &k)
{
    const mih_mat *h = a.h;
    const double *A = a.A, *w = a.w, *Z = a.Z, *eta = a.eta();
    const int32_t t = a.t, c = a.c;
    const SpaCall *spa = a.spa;
    const FirthCall *firth = a.firth;
    const char *who = a.who();
    if (!h || !A || !Z || !a.z || !a.beta || !a.se || !a.neglog10p) { set_error("mih_assoc_score: null argument"); return MIH_BAD_ARG; }
    if (spa) {
        if (!w || !spa->eta || !spa->neglog10p_spa || !spa->state) { set_error("%s: null argument", who); return MIH_BAD_ARG; }
        if (!(spa->cutoff >= 0.0)) { set_error("%s: cutoff must not be negative or NaN, got %g", who, spa->cutoff); return MIH_BAD_ARG; }
    }
    if (firth) {
        if (!w || !firth->eta || !firth->beta || !firth->se || !firth->neglog10p || !firth->state) { set_error("%s: null argument", who); return MIH_BAD_ARG; }
        if (!(firth->cutoff >= 0.0)) { set_error("%s: cutoff must not be negative or NaN, got %g", who, firth->cutoff); return MIH_BAD_ARG; }
    }
    if (t < 1 || t > 32) { set_error("mih_assoc_score: 1 <= t <= 32 traits, got %d", (int)t); return MIH_BAD_ARG; }
    if (c < 1 || c > 64) { set_error("mih_assoc_score: 1 <= c <= 64 covariates, got %d", (int)c); return MIH_BAD_ARG; }
    if (a.slice_rows < 0) { set_error("mih_assoc_score: slice_rows must not be negative, got %lld", (long long)a.slice_rows); return MIH_BAD_ARG; }
    const int64_t n = h->n, p = h->p;
    if (n < 1 || p < 1) { set_error("mih_assoc_score: an empty matrix"); return MIH_BAD_DIM; }
    double wmax = 0.0;                           // the fixed-point scale needs the maximum, and this loop has it
    if (w)
        for (int64_t i = 0; i < n; ++i) {
            if (!(w[i] >= 0.0) || !std::isfinite(w[i])) { set_error("mih_assoc_score: weight %lld is negative or not finite", (long long)i + 1); return MIH_BAD_ARG; }
            wmax = std::max(wmax, w[i]);
        }
    if (!all_finite(A, (size_t)n * (size_t)t)) { set_error("mih_assoc_score: a score residual is not finite"); return MIH_BAD_ARG; }
    if (!all_finite(Z, (size_t)n * (size_t)c)) { set_error("mih_assoc_score: a covariate is not finite"); return MIH_BAD_ARG; }
    if (eta && !all_finite(eta, (size_t)n)) { set_error("%s: a linear predictor is not finite", who); return MIH_BAD_ARG; }
    if (a.sets) MIH_TRY(assoc_sets_check(*a.sets, p));
    if (!assoc_null_factor(Z, w, n, c, k.Linv)) { set_error("mih_assoc_score: Z'WZ is not positive definite"); return MIH_BAD_ARG; }
    k.wmax = wmax;
    return MIH_OK;
}

// ---- the slice plan: the row slices of the class kernel, never longer than the exact range of an f32 accumulator, whatever the
// caller asks for ----
static int assoc_slice_plan(const AssocCall &a, AssocWork &k)
{
    const mih_mat *h = a.h;
    const int64_t slice_rows = a.slice_rows, nbp = h->nbp, ncg = h->ncg;
    k.snp = h->kind == 0; k.classes = k.snp && a.w != nullptr;
    int64_t bps = slice_rows > 0 ? std::min(kAssocSliceBp, (std::min(slice_rows, kAssocSliceBp * 128) + 127) / 128) : kAssocSliceBp;
    int64_t nsl = 1;
    if (k.classes) {
        const int64_t ngp = (ncg + 1) / 2;
        if (slice_rows == 0) {          // a launch with few column groups: more, shorter slices (the sums are integers: same bits)
            const int64_t want = (kAssocWaves + ngp - 1) / ngp;
            bps = std::min(bps, std::max(kAssocMinBp, (nbp + want - 1) / want));
        }
        bps = std::min(bps, std::max<int64_t>(nbp, 1));
        nsl = (nbp + bps - 1) / bps;
        if ((double)ngp * (double)nsl / 4.0 >= 2147483648.0 || nsl >= (1ll << 31)) {
            set_error("mih_assoc_score: %lld column groups in %lld row slices are too many work items for one launch", (long long)ncg, (long long)nsl);
            return MIH_BAD_DIM;
        }
    }
    k.bps = bps; k.nsl = nsl;
    return MIH_OK;
}

// ---- the memory rule: everything the call will hold beyond the handle, against what the device has free ----
static int assoc_memory_rule(const AssocCall &a, const AssocWork &k)
{
    const mih_mat *h = a.h;
    const SpaCall *spa = a.spa;
    const FirthCall *firth = a.firth;
    const SetsCall *sets = a.sets;
    const int32_t t = a.t, c = a.c;
    const int m = t + c;
    const bool snp = k.snp, classes = k.classes;
    const int64_t n = h->n, p = h->p, ncg = h->ncg, nblk = 2 * h->nbp, nsl = k.nsl;
    MIH_HIP(hipSetDevice(h->device));
    const double dn = (double)n, dp = (double)p;
    double need = 8.0 * dn * (2.0 * m + 1.0)                               // A, Z, w and R = [A | w o Z]
                + 8.0 * dp * (m + 2.0 * t + 3.0) + dp + 8.0 * c * c;       // S, z, beta, se, Q, V, the degenerate flags, Linv
    if (snp) {
        const double ops = std::ceil(10.0 * m / 32.0) + std::ceil(m / 19.0);
        need += ops * (double)nblk * 64.0 * 24.0 + 16.0 * m * (double)ncg * 32.0 * 8.0 + 32.0 * dp;      // the fused pass's digit planes and partial sums; Wc
        if (classes) need += 8.0 * (double)h->n_pad + (double)nblk * 1024.0 + (double)nsl * (double)ncg * 8192.0 + 16.0 * dp;   // R_i, their digit planes, the integer partials, Tm
    }
    // the selection, alpha and the slabs are held once, whichever passes run on them
    const double need_spa = spa ? assoc_spa_bytes(n, p, (int)c) : firth ? assoc_flag_bytes(n, p, (int)c) : 0.0;
    const double need_firth = firth ? assoc_firth_bytes(p) : 0.0;
    need += need_spa + need_firth;
    double sets_resident = 0.0;
    const double need_sets = sets ? assoc_sets_bytes(*sets, (int)c, &sets_resident) : 0.0;
    size_t free_b = 0, total_b = 0;
    MIH_HIP(hipMemGetInfo(&free_b, &total_b));
    if (sets && need + need_sets > (double)free_b) {
        set_error("mih_assoc_sets: the scan needs %.0f bytes of device memory and the set pass %.0f more (%.0f of them the covariance and Jacobi slabs of %d sets, the rest their lists, u and results), %.0f bytes are free",
                  need, need_sets, sets_resident, (int)sets->nsets, (double)free_b);
        return MIH_OOM;
    }
    if (firth && need > (double)free_b) {
        set_error("mih_assoc_score_firth: the scan needs %.0f bytes of device memory, the selection %.0f more (the linear predictor, the flagged columns' alpha%s, %lld slabs of %lld adjusted genotypes, held once) and the Firth pass %.0f more (the roots of up to %lld columns), %.0f bytes are free",
                  need - need_spa - need_firth, need_spa, spa ? " and saddlepoint tails" : "", (long long)std::min<int64_t>(p, kSpaSlabs), (long long)n, need_firth,
                  (long long)p, (double)free_b);
        return MIH_OOM;
    }
    if (spa && need > (double)free_b) {
        set_error("mih_assoc_score_spa: the scan needs %.0f bytes of device memory and the saddlepoint pass %.0f more (the linear predictor, the flagged columns' alpha and tails, %lld slabs of %lld adjusted genotypes), %.0f bytes are free",
                  need - need_spa, need_spa, (long long)std::min<int64_t>(p, kSpaSlabs), (long long)n, (double)free_b);
        return MIH_OOM;
    }
    if (need > (double)free_b) {
        set_error("mih_assoc_score: %d traits and %d covariates on %lld x %lld (residuals, the fused pass, class sums and results) need %.0f bytes of device memory, %.0f bytes are free",
                  (int)t, (int)c, (long long)n, (long long)p, need, (double)free_b);
        return MIH_OOM;
    }
    return MIH_OK;
}

// ---- the degenerate columns of a 2-bit handle, decided in integers: no observed genotype, or one class holds all observed ones ----
static int assoc_degenerate(const AssocCall &a, AssocWork &k)
{
    const int64_t p = a.h->p;
    k.deg.assign((size_t)p, 0);
    if (!k.snp) return MIH_OK;
    std::vector<int32_t> &counts = k.counts;
    counts.resize((size_t)(4 * p));
    MIH_TRY(mih_snp_counts(a.h, nullptr, nullptr, counts.data(), nullptr));
    for (int64_t j = 0; j < p; ++j) {
        const int64_t n0 = counts[4 * j], n1 = counts[4 * j + 1], n2 = counts[4 * j + 2], nobs = n0 + n1 + n2;
        k.deg[(size_t)j] = (nobs == 0 || n0 == nobs || n1 == nobs || n2 == nobs) ? 1 : 0;
    }
    return MIH_OK;
}

// ---- the fixed-point weights R_i = rint(w_i 2^e), max w 2^e < 2^54, and their sum (host) ----
static void assoc_fixed_weights(const AssocCall &a, AssocWork &k)
{
    if (!k.classes) return;
    if (k.wmax > 0.0) k.e = std::min(kAssocEbits - std::ilogb(k.wmax), 1000);
    k.Rw.assign((size_t)a.h->n_pad, 0ull);
    for (int64_t i = 0; i < a.h->n; ++i) {
        k.Rw[(size_t)i] = (unsigned long long)std::llrint(std::ldexp(a.w[i], k.e));
        k.rsum = u128_add(k.rsum, U128{0ull, k.Rw[(size_t)i]});
    }
}

// ---- the uploads, and the linear terms: one fused X'R over [A | w o Z] into S ----
static int assoc_linear(const AssocCall &a, AssocWork &k)
{
    const mih_mat *h = a.h;
    hipStream_t s = h->stream;
    const double *w = a.w;
    const int32_t t = a.t, c = a.c;
    const int m = t + c;
    const int64_t n = h->n, p = h->p;
    MIH_TRY(k.Ad.alloc((size_t)n * t)); MIH_TRY(k.Zd.alloc((size_t)n * c)); MIH_TRY(k.wd.alloc((size_t)n)); MIH_TRY(k.R.alloc((size_t)n * m));
    MIH_TRY(k.S.alloc((size_t)p * m)); MIH_TRY(k.Q.alloc((size_t)p)); MIH_TRY(k.V.alloc((size_t)p)); MIH_TRY(k.Ld.alloc((size_t)c * c));
    MIH_TRY(k.zd.alloc((size_t)p * t)); MIH_TRY(k.bd.alloc((size_t)p * t)); MIH_TRY(k.sd.alloc((size_t)p)); MIH_TRY(k.degd.alloc((size_t)p));
    MIH_TRY(xtv_work_init(h, k.xw, m, xtv_tune(0)));
    MIH_HIP(hipMemcpyAsync(k.Ad.p, a.A, sizeof(double) * (size_t)n * t, hipMemcpyHostToDevice, s));
    MIH_HIP(hipMemcpyAsync(k.Zd.p, a.Z, sizeof(double) * (size_t)n * c, hipMemcpyHostToDevice, s));
    if (!w) k.ones.assign((size_t)n, 1.0);
    MIH_HIP(hipMemcpyAsync(k.wd.p, w ? w : k.ones.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    MIH_HIP(hipMemcpyAsync(k.Ld.p, k.Linv.data(), sizeof(double) * (size_t)c * c, hipMemcpyHostToDevice, s));
    MIH_HIP(hipMemcpyAsync(k.degd.p, k.deg.data(), (size_t)p, hipMemcpyHostToDevice, s));

    hipLaunchKernelGGL(k_assoc_rhs, dim3(blocks_of(n), (unsigned)m), dim3(256), 0, s, k.Ad.p, k.wd.p, k.Zd.p, n, (int)t, (int)c, k.R.p);
    MIH_TRY(launch_failed("k_assoc_rhs"));
    return xtv_device(h, k.xw, k.R.p, m, k.S.p, s);
}

// ---- Q, three routes ----
// 2-bit with weights: the class sums Wc from the class kernel over the fixed-point weights
static int assoc_q_classes(const AssocCall &a, AssocWork &k)
{
    const mih_mat *h = a.h;
    hipStream_t s = h->stream;
    const int64_t n = h->n, p = h->p, nbp = h->nbp, ncg = h->ncg, nblk = 2 * nbp, nsl = k.nsl;
    MIH_TRY(k.Rd.alloc((size_t)h->n_pad)); MIH_TRY(k.dig.alloc((size_t)(nblk * 64 * 4))); MIH_TRY(k.part.alloc((size_t)(nsl * ncg * 2048)));
    MIH_TRY(k.tm.alloc((size_t)(2 * p)));
    MIH_HIP(hipMemcpyAsync(k.Rd.p, k.Rw.data(), sizeof(unsigned long long) * (size_t)h->n_pad, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_assoc_digits, dim3(blocks_of(nblk * 64)), dim3(256), 0, s, k.Rd.p, n, nblk, reinterpret_cast<uint4 *>(k.dig.p));
    MIH_TRY(launch_failed("k_assoc_digits"));
    const int64_t items = (ncg + 1) / 2 * nsl;
    PassRecord rec;
    const bool timed = prof_begin(h, s, rec);
    hipLaunchKernelGGL(k_assoc_classes, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const uint4 *>(h->X),
                       reinterpret_cast<const uint4 *>(k.dig.p), nbp, ncg, k.bps, (int)nsl, k.part.p);
    if (timed) { snprintf(rec.kernel, sizeof(rec.kernel), "k_assoc_classes"); rec.residuals = 1; rec.operands = (int)nsl; prof_end(h, s, rec); }
    MIH_TRY(launch_failed("k_assoc_classes"));
    hipLaunchKernelGGL(k_assoc_missing, dim3((unsigned)((p + 3) / 4)), dim3(256), 0, s, h->miss_ptr, h->miss_row, k.Rd.p, p, k.tm.p);
    MIH_TRY(launch_failed("k_assoc_missing"));
    hipLaunchKernelGGL(k_assoc_wsum, dim3(blocks_of(p)), dim3(256), 0, s, k.part.p, (int)nsl, ncg, p, k.tm.p, k.rsum.hi, k.rsum.lo, k.e, k.Wc.p);
    return launch_failed("k_assoc_wsum");
}

// 2-bit with unit weights: the four class sums are the integer counts
static int assoc_q_counts(const AssocCall &a, AssocWork &k)
{
    hipStream_t s = a.h->stream;
    const int64_t p = a.h->p;
    std::vector<double> wc((size_t)(4 * p));
    for (int64_t j = 0; j < 4 * p; ++j) wc[(size_t)j] = (double)k.counts[(size_t)j];
    MIH_HIP(hipMemcpyAsync(k.Wc.p, wc.data(), sizeof(double) * (size_t)(4 * p), hipMemcpyHostToDevice, s));
    MIH_HIP(hipStreamSynchronize(s));            // wc ends here
    return MIH_OK;
}

static int assoc_q(const AssocCall &a, AssocWork &k)
{
    const mih_mat *h = a.h;
    hipStream_t s = h->stream;
    const int64_t n = h->n, p = h->p;
    if (k.snp) {
        MIH_TRY(k.Wc.alloc((size_t)(4 * p)));
        MIH_TRY(k.classes ? assoc_q_classes(a, k) : assoc_q_counts(a, k));
        hipLaunchKernelGGL(k_assoc_q_snp, dim3(blocks_of(p)), dim3(256), 0, s, k.Wc.p, h->mu, h->sinv, h->center, h->scale, h->impute, p, k.Q.p);
        return launch_failed("k_assoc_q_snp");
    }
    const DosageView dv = dosage_view(h);        // dense and dosage: straight from the entries
    by_kind(h, [&](auto K) {
        if constexpr (decltype(K)::value < 3)    // a 2-bit handle went the other way
            hipLaunchKernelGGL(k_assoc_q_dense<decltype(K)::value>, dim3((unsigned)p), dim3(256), 0, s, h->D, h->Df, dv, k.wd.p, n, k.Q.p);
    });
    return launch_failed("k_assoc_q_dense");
}

// ---- the finish: V, then z, beta and se, and all of it on the host with the normal p-values ----
static int assoc_finish(const AssocCall &a, AssocWork &k)
{
    const mih_mat *h = a.h;
    hipStream_t s = h->stream;
    const int32_t t = a.t, c = a.c;
    const int64_t p = h->p;
    hipLaunchKernelGGL(k_assoc_var, dim3(blocks_of(p)), dim3(256), 0, s, k.S.p, p, (int)t, (int)c, k.Ld.p, k.Q.p, k.degd.p, k.V.p);
    MIH_TRY(launch_failed("k_assoc_var"));
    hipLaunchKernelGGL(k_assoc_finish, dim3(blocks_of(p * t)), dim3(256), 0, s, k.S.p, k.V.p, p, (int)t, k.zd.p, k.bd.p, k.sd.p);
    MIH_TRY(launch_failed("k_assoc_finish"));
    k.hz.resize((size_t)p * t); k.hb.resize((size_t)p * t); k.hs.resize((size_t)p);
    MIH_HIP(hipMemcpyAsync(k.hz.data(), k.zd.p, sizeof(double) * (size_t)p * t, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipMemcpyAsync(k.hb.data(), k.bd.p, sizeof(double) * (size_t)p * t, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipMemcpyAsync(k.hs.data(), k.sd.p, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
    if (a.wsum && k.snp) {
        k.hw.resize((size_t)(4 * p));
        MIH_HIP(hipMemcpyAsync(k.hw.data(), k.Wc.p, sizeof(double) * (size_t)(4 * p), hipMemcpyDeviceToHost, s));
    }
    MIH_HIP(hipStreamSynchronize(s));
    k.hn.resize(k.hz.size());
    for (size_t i = 0; i < k.hz.size(); ++i) k.hn[i] = neglog10p_of_z(k.hz[i]);
    return MIH_OK;
}

// ---- the optional passes, on what the finish left: the two solvers on one selection, then the sets ----
static int assoc_passes(const AssocCall &a, const AssocWork &k, SpaOut &spa_out, FirthOut &firth_out, SetsOut &sets_out)
{
    const AssocScan sc = {a.h, a.h->stream, (int)a.c, k.S.p, k.V.p, k.Ld.p, k.Zd.p, k.wd.p, k.zd.p, k.hb.data(), k.hs.data(), k.hn.data()};
    if (a.spa || a.firth) {
        AssocFlagged fl;
        MIH_TRY(assoc_flag_run(a.who(), sc, a.eta(), a.firth ? a.firth->cutoff : a.spa->cutoff, fl));
        if (a.spa) MIH_TRY(assoc_spa_run(sc, fl, spa_out));
        if (a.firth) MIH_TRY(assoc_firth_run(sc, fl, firth_out));
    }
    if (a.sets) MIH_TRY(assoc_sets_run(sc, *a.sets, sets_out));
    return MIH_OK;
}

// ---- publish: the caller's arrays are written here and nowhere else ----
static void assoc_publish(const AssocCall &a, const AssocWork &k)
{
    memcpy(a.z, k.hz.data(), sizeof(double) * k.hz.size());
    memcpy(a.beta, k.hb.data(), sizeof(double) * k.hb.size());
    memcpy(a.se, k.hs.data(), sizeof(double) * k.hs.size());
    memcpy(a.neglog10p, k.hn.data(), sizeof(double) * k.hn.size());
    if (a.wsum)
        for (int64_t j = 0; j < a.h->p; ++j)
            for (int q = 0; q < 3; ++q) a.wsum[3 * j + q] = k.snp ? k.hw[(size_t)(4 * j + 1 + q)] : std::numeric_limits<double>::quiet_NaN();
}

// the body of the four entry points; the results reach the caller's arrays only when all of them are there
static int assoc_score_run(const AssocCall &a)
{
    AssocWork k;
    MIH_TRY(assoc_refuse(a, k));
    MIH_TRY(assoc_slice_plan(a, k));
    MIH_TRY(assoc_memory_rule(a, k));
    MIH_TRY(assoc_degenerate(a, k));
    assoc_fixed_weights(a, k);
    MIH_TRY(assoc_linear(a, k));
    MIH_TRY(assoc_q(a, k));
    MIH_TRY(assoc_finish(a, k));
    SpaOut spa_out;
    FirthOut firth_out;
    SetsOut sets_out;
    MIH_TRY(assoc_passes(a, k, spa_out, firth_out, sets_out));
    assoc_publish(a, k);
    if (a.spa) spa_publish(*a.spa, spa_out);
    if (a.firth) firth_publish(*a.firth, firth_out);
    if (a.sets) sets_publish(*a.sets, sets_out);
    return MIH_OK;
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_assoc_score(const mih_mat *h, const double *A, int32_t t, const double *w, const double *Z, int32_t c, int64_t slice_rows,
                    double *z, double *beta, double *se, double *neglog10p, double *wsum)
{
    return assoc_score_run(AssocCall{h, A, t, w, Z, c, slice_rows, z, beta, se, neglog10p, wsum, nullptr, nullptr, nullptr});
}

int mih_assoc_score_spa(const mih_mat *h, const double *A, const double *w, const double *Z, int32_t c, const double *eta, double cutoff,
                        int64_t slice_rows, double *z, double *beta, double *se, double *neglog10p, double *neglog10p_spa, uint8_t *state,
                        double *t_hat)
{
    const SpaCall spa = {eta, cutoff, neglog10p_spa, state, t_hat};
    return assoc_score_run(AssocCall{h, A, 1, w, Z, c, slice_rows, z, beta, se, neglog10p, nullptr, &spa, nullptr, nullptr});
}

int mih_assoc_score_firth(const mih_mat *h, const double *A, const double *w, const double *Z, int32_t c, const double *eta, double cutoff,
                          int64_t slice_rows, double *z, double *beta, double *se, double *neglog10p, double *beta_firth, double *se_firth,
                          double *neglog10p_firth, uint8_t *firth_state, int32_t *firth_evals, double *neglog10p_spa, uint8_t *spa_state,
                          double *t_hat)
{
    const FirthCall firth = {eta, cutoff, beta_firth, se_firth, neglog10p_firth, firth_state, firth_evals};
    const SpaCall spa = {eta, cutoff, neglog10p_spa, spa_state, t_hat};
    return assoc_score_run(AssocCall{h, A, 1, w, Z, c, slice_rows, z, beta, se, neglog10p, nullptr, neglog10p_spa ? &spa : nullptr, &firth, nullptr});
}

int mih_assoc_sets(const mih_mat *h, const double *A, const double *w, const double *Z, int32_t c, int64_t slice_rows, int32_t nsets,
                   const int64_t *set_ptr, const int32_t *set_col, const double *omega, double *z, double *beta, double *se, double *neglog10p,
                   int32_t *m_used, double *burden_z, double *neglog10p_burden, double *skat_q, double *neglog10p_skat, uint8_t *skat_state,
                   double *lambda, double *cov)
{
    const SetsCall sets = {nsets, set_ptr, set_col, omega, m_used, burden_z, neglog10p_burden, skat_q, neglog10p_skat, skat_state, lambda, cov, nullptr};
    return assoc_score_run(AssocCall{h, A, 1, w, Z, c, slice_rows, z, beta, se, neglog10p, nullptr, nullptr, nullptr, &sets});
}

int mih_assoc_sets_skato(const mih_mat *h, const double *A, const double *w, const double *Z, int32_t c, int64_t slice_rows, int32_t nsets,
                         const int64_t *set_ptr, const int32_t *set_col, const double *omega, int32_t nrho, const double *rho, double *z, double *beta,
                         double *se, double *neglog10p, int32_t *m_used, double *burden_z, double *neglog10p_burden, double *skat_q,
                         double *neglog10p_skat, uint8_t *skat_state, double *lambda, double *cov, double *neglog10p_skato, double *skato_rho,
                         uint8_t *skato_state, double *neglog10p_rho, double *lambda_rho)
{
    const SkatoCall skato = {nrho, rho, neglog10p_skato, skato_rho, skato_state, neglog10p_rho, lambda_rho};
    const SetsCall sets = {nsets, set_ptr, set_col, omega, m_used, burden_z, neglog10p_burden, skat_q, neglog10p_skat, skat_state, lambda, cov, &skato};
    return assoc_score_run(AssocCall{h, A, 1, w, Z, c, slice_rows, z, beta, se, neglog10p, nullptr, nullptr, nullptr, &sets});
}

}  // extern "C"
