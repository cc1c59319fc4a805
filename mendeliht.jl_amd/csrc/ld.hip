// ld.hip -- the correlation of SNP pairs inside a window of columns (linkage disequilibrium) and the pruning of the 2-bit matrix
// by it (mih_ld_band, mih_ld_pairs, mih_ld_prune): what `plink --indep-pairwise` does between SnpArrays.filter and the kinship
// matrix in manuscript/NFBC_sim/NFBC_data_qc.jl:18-33 -- without the matrix leaving the device.
//
// LD of column j with column k is a dot product over the samples, and the tile layout stores 32 columns x 128 samples as the FP4
// fragment of v_mfma_f32_32x32x64_f8f6f4 with K = sample (common.h).  The instruction places row m of A and column n
// of B, K-half h, in the same lane 32 h + m / 32 h + n with the same element order, so the registers of tile(a) are the A operand
// and the registers of tile(b) the B operand as they are: one MFMA per 64 samples yields the 32 x 32 block of sum_i g_ij g_ik / 4,
// exact integers in f32.  No decode, no f64 panel, no transposed image.  Missing genotypes are code 0 in the tiles; a second image
// of the same layout with code 10 (FP4 1.0) at the missing entries gives the three correction sums the mean imputation needs
// through the same instruction.  Everything up to the last dozen f64 operations per pair is an exact integer, so the results do
// not depend on how the columns are cut into panels or the rows into slices.  tests/ld_spec.py states the definitions in numpy.
#include "grm.h"
#include <algorithm>
#include <cmath>
#include <limits>

namespace mih {

typedef float ld_f32x16 __attribute__((ext_vector_type(16)));
typedef int ld_i32x8 __attribute__((ext_vector_type(8)));

constexpr int64_t kLdPanelCols = 4096;          // the library's panel width ...
constexpr int64_t kLdPanelEntries = 1ll << 26;  // ... narrowed until a panel's band has at most this many entries (512 MB of r)
constexpr int64_t kLdSliceBp = 1 << 15;         // block pairs of a row slice: 2^22 rows x products <= 1, multiples of 1/4: exact in f32
constexpr int64_t kLdWaves = 8192;              // work items a launch should have: 8 waves on each of the 1024 SIMDs
constexpr int64_t kLdMinBp = 32;                // ... but no slice shorter than 4096 rows

// ---- 1. the missing-mask tiles ----------------------------------------------------------------------------------------------------
// Img: a zeroed image in the tile layout of columns [c0, c0 + gridDim.x), c0 a multiple of 32.  One wave per column ORs code 10
// into the places of the column's missing rows; the order of the ORs does not matter.
__global__ void __launch_bounds__(64)
k_ld_mask(const int64_t *__restrict__ miss_ptr, const int32_t *__restrict__ miss_row, int64_t c0, int64_t nbp, uint32_t *__restrict__ Img)
{
    const int64_t j = c0 + blockIdx.x;
    for (int64_t t = miss_ptr[j] + threadIdx.x, e = miss_ptr[j + 1]; t < e; t += 64) {
        const int64_t i = miss_row[t];
        atomicOr(&Img[xword(nbp, j - c0, i >> 4)], 2u << (2 * (int)(i & 15)));
    }
}

// ---- 2. the band kernel ------------------------------------------------------------------------------------------------------------
// the two dwords of a lane that cover 64 rows, as FP4 elements, on both sides (the expansion of mfma_fp4, xtv_kernels.h)
__device__ __forceinline__ ld_f32x16 ld_mfma(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, ld_f32x16 acc)
{
    const uint32_t M = 0x33333333u;
    ld_i32x8 a = {(int)(a0 & M), (int)((a0 >> 2) & M), (int)(a1 & M), (int)((a1 >> 2) & M), 0, 0, 0, 0};
    ld_i32x8 b = {(int)(b0 & M), (int)((b0 >> 2) & M), (int)(b1 & M), (int)((b1 >> 2) & M), 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 4, 4, 0, 0, 0, 0);
}

// A wave's work item: (column group a = A0 + al, partner b = a + g with 0 <= g <= G, row slice sl), item = (al (G + 1) + g) nsl + sl.
// It walks the slice's block pairs with both tiles of the next step in flight (the last step loads its own tiles again: no
// branch around the accumulators), two MFMAs per tile pair, and leaves
//     part[((sl nag + al (G + 1) + g) NACC + q) 1024 + 32 m + n],   m = column of a, n = column of b,
// as integers: q = 0: D = 4 acc (genotype x genotype); with HAS_MISSING q = 1: A_jk = 2 acc (mask(a) x genotype(b)), q = 2:
// A_kj = 2 acc (genotype(a) x mask(b)), q = 3: M = acc (mask x mask).  D layout of the instruction: column n = lane & 31,
// row m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (above xtv_epilogue).  Plain stores, every entry written by one lane.
// Img holds the mask tiles of the groups from A0 on.  A partner beyond the last group is not computed and never read.
template <bool HAS_MISSING>
__global__ void __launch_bounds__(256)
k_ld_band(const uint4 *__restrict__ X, const uint4 *__restrict__ Img, int64_t nbp, int64_t ncg, int64_t A0, int64_t nag, int G,
          int64_t bps, int nsl, int32_t *__restrict__ part)
{
    constexpr int NACC = HAS_MISSING ? 4 : 1;
    const int lane = threadIdx.x & 63;
    const int64_t item = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (item >= nag * nsl) return;
    const int sl = (int)(item % nsl);
    const int64_t ag = item / nsl, al = ag / (G + 1), g = ag % (G + 1);
    const int64_t a = A0 + al, b = a + g;
    if (b >= ncg) return;
    const int64_t b0 = sl * bps, b1 = min(nbp, b0 + bps);
    const uint4 *xa = X + a * nbp * 64 + lane, *xb = X + b * nbp * 64 + lane;
    const uint4 *ma = Img + al * nbp * 64 + lane, *mb = Img + (al + g) * nbp * 64 + lane;

    ld_f32x16 acc[NACC];
    #pragma unroll
    for (int q = 0; q < NACC; ++q)
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    uint4 ta = xa[b0 * 64], tb = xb[b0 * 64], ua = make_uint4(0, 0, 0, 0), ub = ua;
    if (HAS_MISSING) { ua = ma[b0 * 64]; ub = mb[b0 * 64]; }
    for (int64_t bp = b0; bp < b1; ++bp) {
        const int64_t nx = min(bp + 1, b1 - 1) * 64;
        const uint4 na = xa[nx], nb = xb[nx];
        uint4 va = ua, vb = ub;
        if (HAS_MISSING) { va = ma[nx]; vb = mb[nx]; }
        acc[0] = ld_mfma(ta.x, ta.y, tb.x, tb.y, acc[0]);
        acc[0] = ld_mfma(ta.z, ta.w, tb.z, tb.w, acc[0]);
        if (HAS_MISSING) {
            acc[1] = ld_mfma(ua.x, ua.y, tb.x, tb.y, acc[1]);
            acc[1] = ld_mfma(ua.z, ua.w, tb.z, tb.w, acc[1]);
            acc[2] = ld_mfma(ta.x, ta.y, ub.x, ub.y, acc[2]);
            acc[2] = ld_mfma(ta.z, ta.w, ub.z, ub.w, acc[2]);
            acc[3] = ld_mfma(ua.x, ua.y, ub.x, ub.y, acc[3]);
            acc[3] = ld_mfma(ua.z, ua.w, ub.z, ub.w, acc[3]);
        }
        ta = na; tb = nb; ua = va; ub = vb;
    }

    int32_t *out = part + (((int64_t)sl * nag + ag) * NACC) * 1024 + (lane & 31);
    #pragma unroll
    for (int q = 0; q < NACC; ++q) {
        const float unit = q == 0 ? 4.f : q == 3 ? 1.f : 2.f;
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            out[q * 1024 + m * 32] = (int32_t)(acc[q][r] * unit);
        }
    }
}

// ---- 3. the finish -----------------------------------------------------------------------------------------------------------------
// a column without an observed genotype, or monomorphic among its observed ones: n_j D_jj = s_j^2, decided in integers
__host__ __device__ inline bool ld_degenerate(int64_t n, int64_t s, int64_t m, int64_t djj)
{
    const uint64_t nj = (uint64_t)(n - m);
    return nj == 0 || nj * (uint64_t)djj == (uint64_t)s * (uint64_t)s;
}

// r_jk from the integers, the float operations in the order tests/ld_spec.py writes them, each rounded by itself
__device__ __forceinline__ double ld_r(int64_t n, int64_t D, int64_t Ajk, int64_t Akj, int64_t M, int64_t sj, int64_t mj, int64_t djj,
                                       int64_t sk, int64_t mk, int64_t dkk)
{
#pragma clang fp contract(off)
    if (ld_degenerate(n, sj, mj, djj) || ld_degenerate(n, sk, mk, dkk)) return 0.0;
    const double nj = (double)(n - mj), nk = (double)(n - mk);
    const double muj = (double)sj / nj, muk = (double)sk / nk;
    const double t1 = muj * (double)(sk - Ajk);
    const double t2 = muk * (double)(sj - Akj);
    const double t3 = (muj * muk) * (double)(n - mj - mk + M);
    const double c = (((double)D - t1) - t2) + t3;
    const double cjj = (double)djj - (double)((uint64_t)sj * (uint64_t)sj) / nj;
    const double ckk = (double)dkk - (double)((uint64_t)sk * (uint64_t)sk) / nk;
    return c / sqrt(cjj * ckk);
}

// One thread per (j, d), j0 <= j < j1, 1 <= d <= wm1: the slices' integers summed, s and m from the upload's counts (col[3 j ..] =
// s_j, m_j, D_jj), r[(j - j0) wm1 + d - 1] = r_{j, j + d}, NaN where j + d >= p; stats (may be null) the four integers, 0 there.
__global__ void __launch_bounds__(256)
k_ld_finish(const int32_t *__restrict__ part, int nacc, int64_t nag, int nsl, int G, int64_t A0, int64_t j0, int64_t j1, int64_t p,
            int64_t n, int64_t wm1, const int64_t *__restrict__ col, double *__restrict__ r, int64_t *__restrict__ stats)
{
    const int64_t idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= (j1 - j0) * wm1) return;
    const int64_t j = j0 + idx / wm1, k = j + idx % wm1 + 1;
    int64_t D = 0, Ajk = 0, Akj = 0, M = 0;
    double v = std::numeric_limits<double>::quiet_NaN();
    if (k < p) {
        const int64_t ag = ((j >> 5) - A0) * (G + 1) + ((k >> 5) - (j >> 5));
        const int64_t e = (j & 31) * 32 + (k & 31);
        for (int sl = 0; sl < nsl; ++sl) {
            const int32_t *q = part + (((int64_t)sl * nag + ag) * nacc) * 1024 + e;
            D += q[0];
            if (nacc == 4) { Ajk += q[1024]; Akj += q[2048]; M += q[3072]; }
        }
        v = ld_r(n, D, Ajk, Akj, M, col[3 * j], col[3 * j + 1], col[3 * j + 2], col[3 * k], col[3 * k + 1], col[3 * k + 2]);
    }
    r[idx] = v;
    if (stats) { stats[4 * idx] = D; stats[4 * idx + 1] = Ajk; stats[4 * idx + 2] = Akj; stats[4 * idx + 3] = M; }
}

// ---- 4. the pair scan --------------------------------------------------------------------------------------------------------------
// The pairs of a panel's band with r r > thr (strictly; a NaN is no pair) in the order (j, k).  One wave per column j, the lanes
// over d in ascending chunks of 64.  off == nullptr: the column's pairs are counted into cnt[j - j0].  Otherwise off[j - j0] is
// where they start in the panel's list -- the exclusive prefix sum of those counts -- and those that start below cap are
// written, a lane's place inside a chunk being the hits of the lanes below it.  No sort, a cut list holds the first pairs, and a
// second call finds the same (k_grm_pairs works the same way).
__global__ void __launch_bounds__(256)
k_ld_pairs(const double *__restrict__ r, int64_t nj, int64_t wm1, int64_t j0, double thr, const int64_t *__restrict__ off,
           int32_t *__restrict__ cnt, int64_t cap, int64_t *__restrict__ col_j, int64_t *__restrict__ col_k, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t jl = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (jl >= nj) return;
    const int64_t base = off ? off[jl] : 0;
    int64_t c = 0;
    for (int64_t d0 = 0; d0 < wm1; d0 += 64) {
        const int64_t d = d0 + lane;
        double v = 0.0;
        bool hit = false;
        if (d < wm1) { v = r[jl * wm1 + d]; hit = v * v > thr; }
        const unsigned long long hits = __ballot(hit);
        if (off && hit) {
            const int64_t at = base + c + __popcll(hits & ((1ull << lane) - 1ull));
            if (at < cap) { col_j[at] = j0 + jl; col_k[at] = j0 + jl + d + 1; out[at] = v; }
        }
        c += __popcll(hits);
    }
    if (!off && lane == 0) cnt[jl] = (int32_t)c;
}

// ---- the driver ----------------------------------------------------------------------------------------------------------------------
struct LdRun {
    int64_t n = 0, p = 0, w = 0, wm1 = 0;              // w = min(window, p)
    std::vector<int32_t> counts;                       // 4 p: n0, n1, n2, nmiss (mih_snp_counts)
    std::vector<int64_t> col;                          // 3 p: s_j, m_j, D_jj
    bool degenerate(int64_t j) const { return ld_degenerate(n, col[3 * j], col[3 * j + 1], col[3 * j + 2]); }
};
// what a caller does with a panel's band while it is on the device: columns [j0, j1), r and stats (null unless asked for) of
// (j1 - j0) wm1 entries
typedef std::function<int(int64_t j0, int64_t j1, const double *r_dev, const int64_t *stats_dev)> LdPanelFn;
// ... and what it allocates once, beside the band, before the first panel is computed (pc: the columns of a full panel)
typedef std::function<int(int64_t pc)> LdPrepFn;

static int ld_check(const char *who, const mih_mat *h, int64_t window)
{
    if (!h || h->kind != 0) { set_error("%s needs a 2-bit (SnpLinAlg) handle", who); return MIH_BAD_ARG; }
    if (window < 2) { set_error("%s: window must be at least 2, got %lld", who, (long long)window); return MIH_BAD_ARG; }
    return MIH_OK;
}

// extra_entry: bytes per band entry the caller's panel function allocates on top (the pair list), extra_col: per panel column
static int ld_run(const char *who, const mih_mat *h, int64_t window, int64_t panel_cols, int64_t slice_rows, bool want_stats,
                  double extra_entry, double extra_col, LdRun &run, const LdPrepFn &prep, const LdPanelFn &fn)
{
    const int64_t n = h->n, p = h->p, nbp = h->nbp, ncg = h->ncg;
    const int64_t w = std::min(window, p), wm1 = w - 1;
    run.n = n; run.p = p; run.w = w; run.wm1 = wm1;
    const int G = (int)std::min((w + 30) / 32, ncg - 1);                 // column 32 a + 31 reaches column 32 a + 31 + wm1
    int64_t pc = panel_cols > 0 ? round_up(panel_cols, 32)
                                : std::max<int64_t>(32, std::min(kLdPanelCols, kLdPanelEntries / std::max<int64_t>(wm1, 1) / 32 * 32));
    pc = std::min(pc, round_up(p, 32));
    const int64_t na = pc / 32, nag = na * (G + 1);
    // no slice is longer than 2^22 rows, whatever the caller asks for: beyond that an f32 accumulator is no longer exact
    int64_t bps = slice_rows > 0 ? std::min(kLdSliceBp, (std::min(slice_rows, kLdSliceBp * 128) + 127) / 128) : kLdSliceBp;
    if (slice_rows <= 0)            // a launch with few (group, partner) items: more, shorter slices, so that its waves fill the device --
        bps = std::min(bps, std::max(kLdMinBp, (nbp + (kLdWaves + nag - 1) / nag - 1) / ((kLdWaves + nag - 1) / nag)));   // the sums are integers: same bits
    const int64_t nsl = (nbp + bps - 1) / bps;
    const bool any_missing = h->total_missing > 0;
    if ((double)nag * (double)nsl / 4.0 >= 2147483648.0 || (double)pc * (double)wm1 / 256.0 >= 2147483648.0 || nsl >= (1ll << 31)) {
        set_error("%s: panels of %lld columns with a window of %lld are too many work items for one launch", who, (long long)pc, (long long)w);
        return MIH_BAD_DIM;
    }

    // the memory rule: everything the call will hold, against what the device has free, before anything is allocated
    MIH_HIP(hipSetDevice(h->device));
    const double entries = (double)pc * (double)wm1;
    const double need = (any_missing ? (double)(na + G) * (double)nbp * 1024.0 : 0.0)              // the panel's mask image
                      + (double)nsl * (double)nag * (any_missing ? 4.0 : 1.0) * 4096.0              // its integer partials
                      + entries * (8.0 + (want_stats ? 32.0 : 0.0) + extra_entry) + (double)pc * extra_col     // its band and the lists
                      + 40.0 * (double)p + 32.0 * (double)nbp;                                      // the columns' counts
    size_t free_b = 0, total_b = 0;
    MIH_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > (double)free_b) {
        set_error("%s: a panel of %lld columns with a window of %lld (mask image, partial sums, band and lists) needs %.0f bytes of device memory, %.0f bytes are free",
                  who, (long long)pc, (long long)w, need, (double)free_b);
        return MIH_OOM;
    }

    hipStream_t s = h->stream;
    run.counts.resize((size_t)(4 * p));
    MIH_TRY(mih_snp_counts(h, nullptr, nullptr, run.counts.data(), nullptr));
    run.col.resize((size_t)(3 * p));
    for (int64_t j = 0; j < p; ++j) {
        const int64_t n1 = run.counts[4 * j + 1], n2 = run.counts[4 * j + 2];
        run.col[3 * j] = n1 + 2 * n2; run.col[3 * j + 1] = run.counts[4 * j + 3]; run.col[3 * j + 2] = n1 + 4 * n2;
    }
    if (wm1 == 0) return MIH_OK;                                          // one column: no pair
    std::vector<int64_t> mptr;
    if (any_missing) {
        mptr.resize((size_t)(p + 1));
        MIH_HIP(hipMemcpyAsync(mptr.data(), h->miss_ptr, sizeof(int64_t) * (size_t)(p + 1), hipMemcpyDeviceToHost, s));
    }
    DevBuf<int64_t> col, stats;
    DevBuf<uint32_t> img;
    DevBuf<int32_t> part;
    DevBuf<double> r;
    MIH_TRY(col.alloc((size_t)(3 * p)));
    MIH_HIP(hipMemcpyAsync(col.p, run.col.data(), sizeof(int64_t) * (size_t)(3 * p), hipMemcpyHostToDevice, s));
    MIH_HIP(hipStreamSynchronize(s));
    if (any_missing) MIH_TRY(img.alloc((size_t)((na + G) * nbp * 256)));
    MIH_TRY(part.alloc((size_t)(nsl * nag * (any_missing ? 4 : 1) * 1024)));
    MIH_TRY(r.alloc((size_t)(pc * wm1)));
    if (want_stats) MIH_TRY(stats.alloc((size_t)(4 * pc * wm1)));
    if (prep) MIH_TRY(prep(pc));

    for (int64_t j0 = 0; j0 < p; j0 += pc) {
        const int64_t j1 = std::min(p, j0 + pc), A0 = j0 / 32, pna = (j1 - j0 + 31) / 32, pnag = pna * (G + 1);
        const int64_t c0 = A0 * 32, c1 = std::min(p, (A0 + pna + G) * 32);       // the columns whose tiles the panel reads
        const bool missing = any_missing && mptr[(size_t)c1] > mptr[(size_t)c0];
        if (missing) {
            MIH_HIP(hipMemsetAsync(img.p, 0, (size_t)((c1 - c0 + 31) / 32 * nbp) * 1024, s));
            hipLaunchKernelGGL(k_ld_mask, dim3((unsigned)(c1 - c0)), dim3(64), 0, s, h->miss_ptr, h->miss_row, c0, nbp, img.p);
            MIH_TRY(launch_failed("k_ld_mask"));
        }
        const dim3 grid((unsigned)((pnag * nsl + 3) / 4));
        const uint4 *X = reinterpret_cast<const uint4 *>(h->X), *I = reinterpret_cast<const uint4 *>(img.p);
        PassRecord rec;
        const bool timed = prof_begin(h, s, rec);
        if (missing) hipLaunchKernelGGL(k_ld_band<true>, grid, dim3(256), 0, s, X, I, nbp, ncg, A0, pnag, G, bps, (int)nsl, part.p);
        else hipLaunchKernelGGL(k_ld_band<false>, grid, dim3(256), 0, s, X, I, nbp, ncg, A0, pnag, G, bps, (int)nsl, part.p);
        if (timed) { snprintf(rec.kernel, sizeof(rec.kernel), missing ? "k_ld_band<missing>" : "k_ld_band"); rec.residuals = (int)pna; rec.operands = G + 1; prof_end(h, s, rec); }
        MIH_TRY(launch_failed("k_ld_band"));
        hipLaunchKernelGGL(k_ld_finish, dim3((unsigned)(((j1 - j0) * wm1 + 255) / 256)), dim3(256), 0, s, part.p, missing ? 4 : 1, pnag, (int)nsl, G,
                           A0, j0, j1, p, n, wm1, col.p, r.p, stats.p);
        MIH_TRY(launch_failed("k_ld_finish"));
        MIH_TRY(fn(j0, j1, r.p, stats.p));
    }
    return MIH_OK;
}

// the pair list of the whole band, the first min(cap, *count) pairs in (j, k) order
static int ld_pairs_run(const char *who, const mih_mat *h, int64_t window, double threshold, int64_t panel_cols, int64_t slice_rows,
                        int64_t cap, LdRun &run, std::vector<int64_t> &vj, std::vector<int64_t> &vk, std::vector<double> &vr, int64_t *count)
{
    hipStream_t s = h->stream;
    int64_t total = 0, room = 0;
    // The counts, the offsets and the panel's list live beside the band for the whole call.  The list starts with room for four
    // pairs per column (at most cap, at most the band) and is replaced by a larger one only when a panel has more: the memory
    // rule counts it as if every entry of a panel's band were a pair.
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> off, lj, lk;
    DevBuf<double> lr;
    auto list_room = [&](int64_t want) -> int {
        if (want <= room) return MIH_OK;
        MIH_TRY(lj.alloc((size_t)want));
        MIH_TRY(lk.alloc((size_t)want));
        MIH_TRY(lr.alloc((size_t)want));
        room = want;
        return MIH_OK;
    };
    MIH_TRY(ld_run(who, h, window, panel_cols, slice_rows, false, cap > 0 ? 24.0 : 0.0, 12.0, run,
                   [&](int64_t pc) -> int {
        MIH_TRY(cnt.alloc((size_t)pc));
        MIH_TRY(off.alloc((size_t)pc));
        return list_room(std::min(cap, std::min(pc * run.wm1, std::max<int64_t>(1024, 4 * pc))));
    },
                   [&](int64_t j0, int64_t j1, const double *r_dev, const int64_t *) -> int {
        const int64_t nj = j1 - j0;
        const unsigned blocks = (unsigned)((nj + 3) / 4);
        hipLaunchKernelGGL(k_ld_pairs, dim3(blocks), dim3(256), 0, s, r_dev, nj, run.wm1, j0, threshold, (const int64_t *)nullptr, cnt.p,
                           (int64_t)0, (int64_t *)nullptr, (int64_t *)nullptr, (double *)nullptr);
        MIH_TRY(launch_failed("k_ld_pairs"));
        std::vector<int32_t> hcnt((size_t)nj);
        MIH_HIP(hipMemcpyAsync(hcnt.data(), cnt.p, sizeof(int32_t) * (size_t)nj, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));
        std::vector<int64_t> hoff((size_t)nj);
        int64_t found = 0;
        for (int64_t t = 0; t < nj; ++t) { hoff[(size_t)t] = found; found += hcnt[(size_t)t]; }
        const int64_t take = std::max<int64_t>(0, std::min(cap - std::min(cap, total), found));
        if (take > 0) {
            MIH_TRY(list_room(take));
            MIH_HIP(hipMemcpyAsync(off.p, hoff.data(), sizeof(int64_t) * (size_t)nj, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_ld_pairs, dim3(blocks), dim3(256), 0, s, r_dev, nj, run.wm1, j0, threshold, (const int64_t *)off.p,
                               (int32_t *)nullptr, take, lj.p, lk.p, lr.p);
            MIH_TRY(launch_failed("k_ld_pairs"));
            const size_t at = vj.size();
            vj.resize(at + (size_t)take); vk.resize(at + (size_t)take); vr.resize(at + (size_t)take);
            MIH_HIP(hipMemcpyAsync(vj.data() + at, lj.p, sizeof(int64_t) * (size_t)take, hipMemcpyDeviceToHost, s));
            MIH_HIP(hipMemcpyAsync(vk.data() + at, lk.p, sizeof(int64_t) * (size_t)take, hipMemcpyDeviceToHost, s));
            MIH_HIP(hipMemcpyAsync(vr.data() + at, lr.p, sizeof(double) * (size_t)take, hipMemcpyDeviceToHost, s));
            MIH_HIP(hipStreamSynchronize(s));
        }
        total += found;
        return MIH_OK;
    }));
    *count = total;
    return MIH_OK;
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_ld_band(const mih_mat *h, int64_t window, int64_t panel_cols, int64_t slice_rows, double *r, int64_t *stats, int64_t *diag)
{
    MIH_TRY(ld_check("mih_ld_band", h, window));
    if (!r) { set_error("mih_ld_band: null argument"); return MIH_BAD_ARG; }
    hipStream_t s = h->stream;
    LdRun run;
    MIH_TRY(ld_run("mih_ld_band", h, window, panel_cols, slice_rows, stats != nullptr, 0.0, 0.0, run, LdPrepFn(),
                   [&](int64_t j0, int64_t j1, const double *r_dev, const int64_t *stats_dev) -> int {
        const size_t at = (size_t)(j0 * run.wm1), cnt = (size_t)((j1 - j0) * run.wm1);
        MIH_HIP(hipMemcpyAsync(r + at, r_dev, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
        if (stats) MIH_HIP(hipMemcpyAsync(stats + 4 * at, stats_dev, sizeof(int64_t) * 4 * cnt, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));                       // the next panel writes the same device buffers
        return MIH_OK;
    }));
    if (diag)
        for (int64_t j = 0; j < run.p; ++j) diag[j] = run.col[(size_t)(3 * j + 2)];
    return MIH_OK;
}

int mih_ld_pairs(const mih_mat *h, int64_t window, double threshold, int64_t panel_cols, int64_t slice_rows, int64_t cap,
                 int64_t *col_j, int64_t *col_k, double *r, int64_t *count)
{
    MIH_TRY(ld_check("mih_ld_pairs", h, window));
    if (std::isnan(threshold)) { set_error("mih_ld_pairs: the threshold is NaN"); return MIH_BAD_ARG; }
    if (cap < 0) { set_error("mih_ld_pairs: cap must not be negative, got %lld", (long long)cap); return MIH_BAD_ARG; }
    if (!count || (cap > 0 && !(col_j && col_k && r))) { set_error("mih_ld_pairs: null argument"); return MIH_BAD_ARG; }
    LdRun run;
    std::vector<int64_t> vj, vk;
    std::vector<double> vr;
    int64_t total = 0;
    MIH_TRY(ld_pairs_run("mih_ld_pairs", h, window, threshold, panel_cols, slice_rows, cap, run, vj, vk, vr, &total));
    if (!vj.empty()) {
        memcpy(col_j, vj.data(), sizeof(int64_t) * vj.size());
        memcpy(col_k, vk.data(), sizeof(int64_t) * vk.size());
        memcpy(r, vr.data(), sizeof(double) * vr.size());
    }
    *count = total;
    return MIH_OK;
}

int mih_ld_prune(const mih_mat *h, int64_t window, int64_t step, double threshold, int64_t panel_cols, int64_t slice_rows,
                 uint8_t *keep, int64_t *n_pairs)
{
    MIH_TRY(ld_check("mih_ld_prune", h, window));
    if (step < 1) { set_error("mih_ld_prune: step must be at least 1, got %lld", (long long)step); return MIH_BAD_ARG; }
    if (std::isnan(threshold)) { set_error("mih_ld_prune: the threshold is NaN"); return MIH_BAD_ARG; }
    if (!keep) { set_error("mih_ld_prune: null argument"); return MIH_BAD_ARG; }
    LdRun run;
    std::vector<int64_t> vj, vk;
    std::vector<double> vr;
    int64_t total = 0;
    MIH_TRY(ld_pairs_run("mih_ld_prune", h, window, threshold, panel_cols, slice_rows, std::numeric_limits<int64_t>::max(), run, vj, vk, vr,
                         &total));
    const int64_t p = run.p;
    // the greedy pass of ld_spec.prune: the list is in (j, k) order, so the partners of a column above the threshold are a run of it
    std::vector<int64_t> start((size_t)(p + 1), 0);
    for (int64_t j : vj) ++start[(size_t)(j + 1)];
    for (int64_t j = 0; j < p; ++j) start[(size_t)(j + 1)] += start[(size_t)j];
    std::vector<double> maf((size_t)p);
    std::vector<uint8_t> kp((size_t)p);
    for (int64_t j = 0; j < p; ++j) {
        const double n0 = run.counts[4 * j], n1 = run.counts[4 * j + 1], n2 = run.counts[4 * j + 2];
        const double f = (n1 + 2.0 * n2) / (2.0 * (n0 + n1 + n2));
        maf[(size_t)j] = std::min(f, 1.0 - f);
        kp[(size_t)j] = run.degenerate(j) ? 0 : 1;
    }
    for (int64_t s0 = 0; s0 < p; s0 += step) {
        const int64_t e = std::min(p, s0 + run.w);
        for (int64_t i = s0; i < e; ++i) {
            if (!kp[(size_t)i]) continue;
            for (int64_t t = start[(size_t)i]; t < start[(size_t)(i + 1)]; ++t) {
                const int64_t k = vk[(size_t)t];
                if (k >= e) break;
                if (!kp[(size_t)k]) continue;
                if (maf[(size_t)i] < maf[(size_t)k]) { kp[(size_t)i] = 0; break; }
                kp[(size_t)k] = 0;
            }
        }
        if (p - s0 <= step) break;                              // (s0 + step must not overflow)
    }
    memcpy(keep, kp.data(), (size_t)p);
    if (n_pairs) *n_pairs = total;
    return MIH_OK;
}

}  // extern "C"
