// score_image.hip -- the score image of a 2-bit matrix: a second, derived image of an immutable handle that only the
// single-residual X'r pass (428 format) reads.  The saving comes from allele frequency: a column with few dosage-2 entries is
// almost a 0/1 column, and a 0/1 column needs one bit per genotype.
//   class 1 (at most tau * n dosage-2 entries): one-bit tiles of the plane [g >= 1] -- 1 KB holds two column groups x 128 rows,
//            the A fragments come out of a dword by (u >> k) & 0x11111111 (score_image.h) -- and, per (sub-slice of the rows,
//            column), the list of its dosage-2 rows.  k_xtv_hom turns the lists into the exact digit sums the one-bit tile misses
//            (a 2 was multiplied as 1), the pass adds them to its accumulator tile before the f64 recombination;
//   class 2 (the rest): the matrix's own tiles, regrouped.
// Both regions keep the matrix's column order inside the class; col_of maps an image position back to its column, so the pass
// writes the same partial[slice][column] the 2-bit pass writes -- every partial, and so every result, is bit for bit the 2-bit
// pass's.  The image is a cache: workspaces pin it (XtvWork::img), mih_device_trim and an allocation that runs out of memory
// release the unpinned ones.
#include "common.h"
#include "score_image.h"
#include <algorithm>

namespace mih {

ScoreImage::~ScoreImage()
{
    // (the last reference can go anywhere -- a workspace's end, a trim inside somebody's allocation: the thread's device stays what it was)
    int was = -1;
    if (hipGetDevice(&was) != hipSuccess) { (void)hipGetLastError(); was = -1; }
    if (was != device) (void)hipSetDevice(device);
    struct Back { int was, dev; ~Back() { if (was >= 0 && was != dev) (void)hipSetDevice(was); } } back{was, device};
    if (tiles) (void)hipFree(tiles);
    if (col_of) (void)hipFree(col_of);
    if (seg_off) (void)hipFree(seg_off);
    if (order) (void)hipFree(order);
    if (rows) (void)hipFree(rows);
}

// ---- the registry of handles that hold an image (mih_device_trim) ----------------------------------------------------------
static std::mutex g_reg_mu;
static std::vector<const mih_mat *> g_reg;

std::shared_ptr<const ScoreImage> score_image_of(const mih_mat *h)
{
    std::lock_guard<std::mutex> g(h->img_mu);
    return h->img;
}
static void set_image(const mih_mat *h, std::shared_ptr<const ScoreImage> im)
{
    std::shared_ptr<const ScoreImage> old;
    {
        std::lock_guard<std::mutex> r(g_reg_mu);
        auto it = std::find(g_reg.begin(), g_reg.end(), h);
        if (im && it == g_reg.end()) g_reg.push_back(h);
        if (!im && it != g_reg.end()) g_reg.erase(it);
        std::lock_guard<std::mutex> g(h->img_mu);
        old.swap(h->img);
        h->img = std::move(im);
    }
}       // (`old` goes here, outside both locks: the memory is freed unless a workspace still pins it)
void score_image_forget(const mih_mat *h) { set_image(h, nullptr); }

// releases every image of the device that nobody but its handle holds; the bytes released
size_t trim_score_images(int device)
{
    std::vector<std::shared_ptr<const ScoreImage>> gone;
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> r(g_reg_mu);
        for (size_t i = 0; i < g_reg.size();) {
            const mih_mat *h = g_reg[i];
            std::lock_guard<std::mutex> g(h->img_mu);
            if (h->device == device && h->img && h->img.use_count() == 1) {
                bytes += h->img->bytes;
                gone.push_back(std::move(h->img));
                h->img.reset();
                g_reg.erase(g_reg.begin() + (long)i);
            } else ++i;
        }
    }
    if (!gone.empty()) {               // no pass of a finished workspace is still reading
        int was = -1;
        if (hipGetDevice(&was) != hipSuccess) { (void)hipGetLastError(); was = -1; }
        if (was != device) (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        if (was >= 0 && was != device) (void)hipSetDevice(was);
    }
    gone.clear();
    return bytes;
}

// ---- building the image -----------------------------------------------------------------------------------------------------
// dosage-2 entries of every column (INT32_MAX if the column holds the code 3, which no finished matrix does: such a column stays class 2)
__global__ void __launch_bounds__(256)
k_img_count2(const uint4 *__restrict__ X, int64_t nbp, int64_t p, int32_t *__restrict__ c2)
{
    const int64_t j = blockIdx.x * 256ll + threadIdx.x;
    if (j >= p) return;
    const uint4 *q = X + (j >> 5) * nbp * 64 + (j & 31);
    uint32_t cnt = 0, bad = 0;
    for (int64_t b = 0; b < nbp; ++b)
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint4 v = q[b * 64 + h * 32];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t hi = w[k] & 0xAAAAAAAAu;
                bad |= hi & ((w[k] & 0x55555555u) << 1);
                cnt += __popc(hi);
            }
        }
    c2[j] = bad ? 0x7fffffff : (int32_t)cnt;
}

// image tile t (class 2: t < ncg2, a copy of 32 gathered columns; class 1: two gathered column groups at one bit), blocks of rows
// blockIdx.y * 4 + wave, + 4 * gridDim.y, ...
__global__ void __launch_bounds__(256)
k_img_pack(const uint4 *__restrict__ X, int64_t nbp, int64_t ncg2, const int32_t *__restrict__ col_of, uint4 *__restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, h = lane >> 5;
    const int64_t t = blockIdx.x;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    if (t < ncg2) {
        const int64_t j = col_of[t * 32 + m];
        const uint4 *src = j < 0 ? nullptr : X + (j >> 5) * nbp * 64 + h * 32 + (j & 31);
        for (int64_t b = blockIdx.y * 4ll + wave; b < nbp; b += 4ll * gridDim.y)
            out[(t * nbp + b) * 64 + lane] = src ? src[b * 64] : zero;
        return;
    }
    const int64_t g = ncg2 + 2 * (t - ncg2);
    const int64_t ja = col_of[g * 32 + m], jb = col_of[(g + 1) * 32 + m];
    const uint4 *sa = ja < 0 ? nullptr : X + (ja >> 5) * nbp * 64 + h * 32 + (ja & 31);
    const uint4 *sb = jb < 0 ? nullptr : X + (jb >> 5) * nbp * 64 + h * 32 + (jb & 31);
    for (int64_t b = blockIdx.y * 4ll + wave; b < nbp; b += 4ll * gridDim.y) {
        const uint4 va = sa ? sa[b * 64] : zero, vb = sb ? sb[b * 64] : zero;
        out[(t * nbp + b) * 64 + lane] = make_uint4(onebit_pack(va.x, va.y), onebit_pack(va.z, va.w), onebit_pack(vb.x, vb.y), onebit_pack(vb.z, vb.w));
    }
}

// The dosage-2 rows of one (sub-slice, class-1 position): FILL = false counts them, FILL = true writes them, ascending, as row
// numbers inside the sub-slice and pads the list to a multiple of 8 entries with the number one past a sub-slice's last row.
// Thread = one list, by slot (position through `order`): a wave is a slot group of k_xtv_hom, the lists of one (slice, group,
// sub-slice) share a block of chunks and a list's chunk c goes to hom_chunk_slot() of the group's 64 chunk counts (score_image.h).
// The reads of X are scattered (the slots of a group are columns from all over the matrix): build time.
MIH_HD int64_t hom_seg(int split, int64_t pos1, int64_t slot, int nss, int k)      // seg_off's index of a list: (slice, group, sub-slice, lane)
{
    return (((int64_t)split * (pos1 / kHomGroup) + slot / kHomGroup) * nss + k) * kHomGroup + slot % kHomGroup;
}
template <bool FILL>
__global__ void __launch_bounds__(256)
k_img_lists(const uint4 *__restrict__ X, int64_t nbp, int splits, int nss, int64_t pos1, const int32_t *__restrict__ col1,
            const int32_t *__restrict__ order, uint32_t *__restrict__ count, const uint32_t *__restrict__ seg_off, uint16_t *__restrict__ rows)
{
    __shared__ uint32_t chunks[4][kHomGroup];
    const int64_t slot = blockIdx.x * 256ll + threadIdx.x;
    const bool live = slot < pos1;                       // (pos1 is a multiple of 64: whole waves)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = blockIdx.y;                          // slice * nss + sub-slice of it
    const int split = sub / nss, k = sub - split * nss;
    const int64_t bps = (nbp + splits - 1) / splits;
    const int64_t s1 = std::min<int64_t>((int64_t)(split + 1) * bps, nbp);
    const int64_t b0 = split * bps + (int64_t)k * kHomSubBlocks, b1 = std::min<int64_t>(b0 + kHomSubBlocks, s1);
    const int64_t seg = live ? hom_seg(split, pos1, slot, nss, k) : 0;
    if (FILL) {
        chunks[wave][lane] = live ? seg_off[seg + 1] - seg_off[seg] : 0u;
        __syncthreads();
    }
    if (!live) return;
    const int64_t j = col1[order[slot]];
    uint32_t cnt = 0;
    const uint32_t *gc = chunks[wave];
    uint16_t *blk = FILL ? rows + (size_t)seg_off[seg - lane] * 8 : nullptr, *dst = blk;      // the group's block; the list's current chunk
    if (j >= 0) {
        const uint4 *q = X + (j >> 5) * nbp * 64 + (j & 31);
        for (int64_t b = b0; b < b1; ++b) {
            const uint4 v0 = q[b * 64], v1 = q[b * 64 + 32];
            // ascending rows of the block: 64 e + 32 h + 16 u + s
            const uint32_t w[8] = {v0.x, v0.y, v1.x, v1.y, v0.z, v0.w, v1.z, v1.w};
            #pragma unroll
            for (int i = 0; i < 8; ++i) {
                uint32_t hi = w[i] & 0xAAAAAAAAu;
                if (!FILL) cnt += __popc(hi);
                else
                    while (hi) {
                        const int bit = __ffs(hi) - 1;
                        if ((cnt & 7u) == 0) dst = blk + (size_t)hom_chunk_slot(gc, lane, cnt >> 3) * 8;
                        dst[cnt++ & 7u] = (uint16_t)((b - b0) * 128 + 16 * i + (bit >> 1));
                        hi &= hi - 1;
                    }
            }
        }
    }
    if (!FILL) count[seg] = cnt;
    else
        while (cnt & 7u) dst[cnt++ & 7u] = (uint16_t)(kHomSubBlocks * 128);   // padding: the slot behind the sub-slice's rows (U of R = 0)
}

// ---- the exception kernel ---------------------------------------------------------------------------------------------------
// E[slice][class-1 position][t] = sum of digit t of R over the position's dosage-2 rows in the slice.  A workgroup takes 512
// positions of one row slice and walks the slice's sub-slices: U of the sub-slice's rows goes to LDS once, every thread then
// follows its own list (16 B = 8 row numbers a load; the loads of a wave are one contiguous run of the group's block, and the
// next one is in flight while this one is added) and counts the set bits of U[row] by position with carry-save adders, four
// chunks a round (HomCsa of score_image.h; the digit sums are HomSum's).  Integer sums: no order to keep.  Runs between k_digits
// and the pass, under the same gate.
constexpr int kHomThreads = 512;
__global__ void __launch_bounds__(kHomThreads, 4)      // (4 waves a SIMD = two workgroups a CU: at most 128 VGPRs)
k_xtv_hom(const unsigned long long *__restrict__ U, int64_t nbp, int splits, int nss, int64_t pos1, const uint32_t *__restrict__ seg_off,
          const uint16_t *__restrict__ rows, const int32_t *__restrict__ order, float *__restrict__ E, const int32_t *__restrict__ gate,
          int32_t gate_val)
{
    if (gate && *gate != gate_val) return;
    constexpr int SUB = kHomSubBlocks * 128;
    __shared__ __align__(16) unsigned long long su[SUB + 2];      // [SUB]: what a padding entry reads: U of R = 0
    const int split = blockIdx.x % splits;
    // thread -> position through `order`: the positions by falling number of dosage-2 entries, so that the lanes of a wave walk
    // lists of about the same length and the long lists start first (of every slice: the slice is the fast grid index)
    const int64_t slot = (blockIdx.x / splits) * (int64_t)kHomThreads + threadIdx.x;
    const int64_t pos = slot < pos1 ? order[slot] : pos1;
    const int64_t bps = (nbp + splits - 1) / splits;
    const int64_t s0 = split * bps, s1 = std::min<int64_t>(s0 + bps, nbp);
    HomCsa hc;
    hc.init();
    if (threadIdx.x == 0) su[SUB] = hom_u(0);
    // The wave is one slot group (kHomGroup = 64 = the wave; pos1 is a multiple of 64, so a wave is live or not as a whole).  Its
    // offsets of a sub-slice are 64 consecutive entries of seg_off: a lane's chunk count is the difference to its successor's
    // entry (lane 63: lane 0's of the next sub-slice), the block of the group's chunks starts at lane 0's.  Chunk c of the lane
    // is at base_c + (lower lanes with more than c chunks), base_c+1 = base_c + (lanes with more than c chunks): hom_chunk_slot()
    // of score_image.h by ballots.  The wave's load of its chunks c is one contiguous run.
    const uint4 *all = reinterpret_cast<const uint4 *>(rows);
    const int lane = threadIdx.x & 63;
    const bool live = slot < pos1;
    const uint32_t *off = seg_off + (live ? hom_seg(split, pos1, slot - lane, nss, 0) : 0);
    uint32_t o_cur = live ? off[lane] : 0u;
    // U of a sub-slice goes through registers, 16 bytes a thread and round, every round's load in flight at once (one load, one wait,
    // one LDS write per round cost sixteen trips to the L2 between the two barriers), and the NEXT sub-slice's loads are issued
    // before this one's lists are walked.  (A macro, not a lambda: captured by a lambda, st[] went to scratch memory.)
    constexpr int kStage = SUB / (2 * kHomThreads);
    static_assert(SUB % (2 * kHomThreads) == 0, "a sub-slice is a whole number of 16-byte rounds of the workgroup");
    const ulonglong2 *U2 = reinterpret_cast<const ulonglong2 *>(U);
    ulonglong2 st[kStage];
#define MIH_HOM_FETCH(k_)                                                                                               \
    {   /* (past the slice's end: nothing is read) */                                                                    \
        const int64_t fb0 = s0 + (int64_t)(k_) * kHomSubBlocks, fb1 = std::min<int64_t>(fb0 + kHomSubBlocks, s1);         \
        const int len2 = (int)(fb1 - fb0) * 64;                                                                          \
        _Pragma("unroll")                                                                                                \
        for (int j = 0; j < kStage; ++j) {                                                                               \
            const int i = j * kHomThreads + (int)threadIdx.x;                                                            \
            st[j] = i < len2 ? U2[fb0 * 64 + i] : make_ulonglong2(0, 0);                                                 \
        }                                                                                                                \
    }
    MIH_HOM_FETCH(0)
    for (int k = 0; k < nss; ++k) {
        const int64_t b0 = s0 + (int64_t)k * kHomSubBlocks, b1 = std::min<int64_t>(b0 + kHomSubBlocks, s1);
        if (b0 >= b1) break;                              // (uniform)
        const int len = (int)(b1 - b0) * 128;
        // the next sub-slice's offsets, requested before the barrier (behind the group's last sub-slice only lane 0's entry
        // exists for certain: it is seg_off's last)
        const uint32_t o_nxt = live ? off[(k + 1) * kHomGroup + (k + 1 < nss ? lane : 0)] : 0u;
        __syncthreads();
        #pragma unroll
        for (int j = 0; j < kStage; ++j) {
            const int i = j * kHomThreads + (int)threadIdx.x;
            if (2 * i < len) reinterpret_cast<ulonglong2 *>(su)[i] = st[j];
        }
        __syncthreads();
        if (k + 1 < nss) MIH_HOM_FETCH(k + 1)
        if (live) {
            const uint32_t up = (uint32_t)__shfl_down((int)o_cur, 1);
            const uint32_t nxt0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)o_nxt);      // (by the whole wave: not inside the select)
            const uint32_t cnt = (lane == 63 ? nxt0 : up) - o_cur;
            uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)o_cur);
            uint64_t m = __ballot(cnt > 0u);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (cnt > 0u) v = all[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))];
            // (wave-uniform: rounds of kCsaGroup chunks, as many as the longest list needs; a list that has ended adds zero carry words)
            for (uint32_t c = 0; m != 0; c += (uint32_t)kCsaGroup) {
                uint32_t c16[kCsaGroup / 2][2];
                #pragma unroll
                for (int j2 = 0; j2 < kCsaGroup / 2; ++j2) {
                    uint32_t c8[2][2];
                    #pragma unroll
                    for (int j1 = 0; j1 < 2; ++j1) {
                        const uint32_t cj = c + 2 * j2 + j1;
                        base += (uint32_t)__popcll(m);
                        const uint64_t m1 = __ballot(cnt > cj + 1u);
                        uint4 vn = v;                     // chunk cj + 1 is on its way while chunk cj is gathered and added
                        if (cnt > cj + 1u) vn = all[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u))];
                        c8[j1][0] = c8[j1][1] = 0u;
                        if (cnt > cj) {
                            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                            uint64_t u8[kHomChunk];
                            #pragma unroll
                            for (int i = 0; i < kHomChunk; ++i) u8[i] = su[(w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu];
                            hc.chunk_carry(u8, c8[j1]);                        // (seven adders a half, score_image.h)
                        }
                        v = vn;
                        m = m1;
                    }
                    hc.pair_carry(c8[0], c8[1], c16[j2]);
                }
                hc.add_pairs(c16[0], c16[1]);                                  // (by the whole wave: its flush is one branch for all lanes)
            }
            hc.terms += (uint32_t)kHomChunk * cnt;                            // (padding entries are terms, a missing chunk is not)
        }
        o_cur = o_nxt;
    }
    if (pos >= pos1) return;
    hc.finish();
    float *e = E + ((int64_t)split * pos1 + pos) * 32;
    #pragma unroll
    for (int q = 0; q < 8; ++q) {
        float4 f;
        f.x = 4 * q + 0 < kHomDigits ? (float)hc.digit_sum(4 * q + 0 < kHomDigits ? 4 * q + 0 : 0) : 0.f;
        f.y = 4 * q + 1 < kHomDigits ? (float)hc.digit_sum(4 * q + 1 < kHomDigits ? 4 * q + 1 : 0) : 0.f;
        f.z = 4 * q + 2 < kHomDigits ? (float)hc.digit_sum(4 * q + 2 < kHomDigits ? 4 * q + 2 : 0) : 0.f;
        f.w = 4 * q + 3 < kHomDigits ? (float)hc.digit_sum(4 * q + 3 < kHomDigits ? 4 * q + 3 : 0) : 0.f;
        reinterpret_cast<float4 *>(e)[q] = f;
    }
}
#undef MIH_HOM_FETCH

void launch_xtv_hom(const ScoreImage &im, const unsigned long long *U, float *E, const int32_t *gate, int32_t gate_val, hipStream_t s)
{
    if (im.pos1 == 0) return;
    hipLaunchKernelGGL(k_xtv_hom, dim3((unsigned)((im.pos1 + kHomThreads - 1) / kHomThreads * im.splits)), dim3(kHomThreads), 0, s,
                       U, im.nbp, im.splits, im.nss, im.pos1, im.seg_off, im.rows, im.order, E, gate, gate_val);
}

// The library's default threshold: a column is class 1 if at most this fraction of its entries is a dosage 2
// (profiles/score_image.md §9: the sweep it comes from; 0.015 .. 0.025 are within its noise of each other).
constexpr double kDefaultHomFraction = 0.02;

// classification: c2 of every column on the host, the image's positions, and what the image would weigh
struct ImagePlan { std::vector<int32_t> col_of, order; int64_t ncg2 = 0, nt1 = 0, p1 = 0, hom_entries = 0; size_t tile_bytes = 0; };
// the image's row slices (those of the library's default pass) and the sub-slices of one; false: the matrix is too tall for the pass
static bool image_slices(const mih_mat *h, int &splits, int &nss)
{
    DigitMode dm = {4, 28, 1, 32, 53, 22};
    splits = xtv_default_splits(h, dm);
    if (splits <= 0) return false;
    const int64_t bps = (h->nbp + splits - 1) / splits;
    nss = (int)((bps + kHomSubBlocks - 1) / kHomSubBlocks);
    return true;
}
// an upper bound of what the lists and their offset table weigh: 2 bytes an entry, at most 14 bytes of padding a list
static size_t plan_list_bytes(const mih_mat *h, const ImagePlan &pl)
{
    int splits = 0, nss = 0;
    if (!image_slices(h, splits, nss)) return 0;
    const size_t nseg = (size_t)splits * (size_t)nss * (size_t)pl.nt1 * 64;
    return 2 * (size_t)pl.hom_entries + 14 * nseg + sizeof(uint32_t) * (nseg + 1);
}
static int plan_image(const mih_mat *h, double tau, ImagePlan &pl)
{
    if (h->p >= (1ll << 31)) { set_error("the score image needs p < 2^31"); return MIH_BAD_DIM; }       // (its column maps are int32)
    DevBuf<int32_t> c2;
    MIH_TRY(c2.alloc((size_t)h->p));
    hipLaunchKernelGGL(k_img_count2, dim3((unsigned)((h->p + 255) / 256)), dim3(256), 0, h->stream, reinterpret_cast<const uint4 *>(h->X), h->nbp, h->p, c2.p);
    std::vector<int32_t> hc((size_t)h->p);
    MIH_HIP(hipMemcpyAsync(hc.data(), c2.p, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, h->stream));
    MIH_HIP(hipStreamSynchronize(h->stream));
    const double lim = tau * (double)h->n;
    std::vector<int32_t> one, two;
    for (int64_t j = 0; j < h->p; ++j) ((double)hc[(size_t)j] <= lim ? one : two).push_back((int32_t)j);
    pl.p1 = (int64_t)one.size();
    pl.hom_entries = 0;
    for (int32_t j : one) pl.hom_entries += hc[(size_t)j];
    pl.ncg2 = ((int64_t)two.size() + 31) / 32;
    pl.nt1 = (pl.p1 + 63) / 64;
    pl.col_of.assign((size_t)(pl.ncg2 + 2 * pl.nt1) * 32, -1);
    std::copy(two.begin(), two.end(), pl.col_of.begin());
    std::copy(one.begin(), one.end(), pl.col_of.begin() + pl.ncg2 * 32);
    pl.tile_bytes = (size_t)(pl.ncg2 + pl.nt1) * (size_t)h->nbp * 1024;
    // k_xtv_hom's thread order: the class-1 positions by falling count of dosage-2 entries (pads last)
    pl.order.resize((size_t)pl.nt1 * 64);
    for (size_t i = 0; i < pl.order.size(); ++i) pl.order[i] = (int32_t)i;
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](int32_t a, int32_t b) {
        const int32_t ca = (size_t)a < one.size() ? hc[(size_t)one[(size_t)a]] : -1, cb = (size_t)b < one.size() ? hc[(size_t)one[(size_t)b]] : -1;
        return ca > cb;
    });
    return MIH_OK;
}

static int build_image(const mih_mat *h, double tau, const ImagePlan &pl, std::shared_ptr<const ScoreImage> &out)
{
    std::shared_ptr<ScoreImage> im(new ScoreImage());
    im->device = h->device; im->tau = tau; im->nbp = h->nbp;
    im->ncg2 = pl.ncg2; im->nt1 = pl.nt1; im->p1 = pl.p1; im->pos1 = 2 * pl.nt1 * 32;
    if (!image_slices(h, im->splits, im->nss)) { set_error("the matrix is too tall for the single-residual pass"); return MIH_BAD_DIM; }
    hipStream_t s = h->stream;
    auto oom = [&](const char *what) { (void)hipGetLastError(); set_error("no device memory for the score image (%s)", what); return MIH_OOM; };
    if (device_malloc(&im->tiles, std::max<size_t>(pl.tile_bytes, 1024)) != hipSuccess) return oom("tiles");
    if (device_malloc(&im->col_of, sizeof(int32_t) * pl.col_of.size() + 256) != hipSuccess) return oom("column map");
    MIH_HIP(hipMemcpyAsync(im->col_of, pl.col_of.data(), sizeof(int32_t) * pl.col_of.size(), hipMemcpyHostToDevice, s));
    if (device_malloc(&im->order, sizeof(int32_t) * pl.order.size() + 256) != hipSuccess) return oom("thread order");
    MIH_HIP(hipMemcpyAsync(im->order, pl.order.data(), sizeof(int32_t) * pl.order.size(), hipMemcpyHostToDevice, s));
    if (pl.ncg2 + pl.nt1 > 0) {
        const unsigned gy = (unsigned)std::min<int64_t>((h->nbp + 3) / 4, 64);
        hipLaunchKernelGGL(k_img_pack, dim3((unsigned)(pl.ncg2 + pl.nt1), gy), dim3(256), 0, s, reinterpret_cast<const uint4 *>(h->X), h->nbp, pl.ncg2,
                           im->col_of, reinterpret_cast<uint4 *>(im->tiles));
    }
    const size_t nseg = (size_t)im->splits * (size_t)im->nss * (size_t)im->pos1;
    if (device_malloc(&im->seg_off, sizeof(uint32_t) * (nseg + 1)) != hipSuccess) return oom("list offsets");
    size_t list_bytes = 16;
    if (nseg > 0) {
        DevBuf<uint32_t> cnt;
        MIH_TRY(cnt.alloc(nseg));
        const dim3 grid((unsigned)((im->pos1 + 255) / 256), (unsigned)(im->splits * im->nss));
        const int32_t *col1 = im->col_of + pl.ncg2 * 32;
        hipLaunchKernelGGL(k_img_lists<false>, grid, dim3(256), 0, s, reinterpret_cast<const uint4 *>(h->X), h->nbp, im->splits, im->nss, im->pos1, col1,
                           im->order, cnt.p, (const uint32_t *)nullptr, (uint16_t *)nullptr);
        std::vector<uint32_t> hc(nseg + 1);
        MIH_HIP(hipMemcpyAsync(hc.data(), cnt.p, sizeof(uint32_t) * nseg, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));
        uint64_t run = 0;
        for (size_t i = 0; i < nseg; ++i) { const uint32_t c = hc[i]; hc[i] = (uint32_t)run; run += (c + 7) / 8; }
        if (run >= (1ull << 32)) { set_error("too many dosage-2 entries for the score image's lists: lower max_hom_fraction"); return MIH_BAD_ARG; }
        hc[nseg] = (uint32_t)run;
        list_bytes = std::max<size_t>((size_t)run * 16, 16);
        if (device_malloc(&im->rows, list_bytes) != hipSuccess) return oom("lists");
        MIH_HIP(hipMemcpyAsync(im->seg_off, hc.data(), sizeof(uint32_t) * (nseg + 1), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_img_lists<true>, grid, dim3(256), 0, s, reinterpret_cast<const uint4 *>(h->X), h->nbp, im->splits, im->nss, im->pos1, col1,
                           im->order, (uint32_t *)nullptr, im->seg_off, im->rows);
        MIH_HIP(hipStreamSynchronize(s));
    } else {
        const uint32_t z = 0;
        MIH_HIP(hipMemcpyAsync(im->seg_off, &z, sizeof(z), hipMemcpyHostToDevice, s));
    }
    MIH_HIP(hipStreamSynchronize(s));
    MIH_HIP(hipGetLastError());
    im->bytes = pl.tile_bytes + sizeof(int32_t) * (pl.col_of.size() + pl.order.size()) + sizeof(uint32_t) * (nseg + 1) + list_bytes;
    out = im;
    return MIH_OK;
}

// The automatic rule (set-up of a session whose workspace will ride the image -- xtv_rides_image; never inside a step): a 2-bit matrix of
// 4 GiB or more (the reserve rule's size) gets an image if the image's tiles are at most 0.97 of the matrix's bytes and the device
// has the image's size -- the tiles, and the lists by the plan's count of dosage-2 entries (plan_list_bytes) -- plus kImageMargin
// free.  Failure is silent: the 2-bit pass runs.
constexpr size_t kImageMinMatrix = 4ull << 30;
constexpr size_t kImageMargin = 8ull << 30;
void score_image_auto(const mih_mat *h)
{
    if (!h || h->kind != 0 || score_image_of(h)) return;
    const size_t x_bytes = (size_t)h->ncg * (size_t)h->nbp * 1024;
    if (x_bytes < kImageMinMatrix) return;
    // one automatic build at a time: of two sessions set up together the second finds the first one's image (or its refusal)
    static std::mutex one_at_a_time;
    std::lock_guard<std::mutex> serial(one_at_a_time);
    if (score_image_of(h)) return;
    {
        std::lock_guard<std::mutex> g(h->img_mu);
        if (h->img_declined) return;       // (the classification is a pass over the whole matrix: once per handle)
    }
    if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return; }
    ImagePlan pl;
    std::shared_ptr<const ScoreImage> im;
    size_t free_b = 0, total_b = 0;
    const bool ok = plan_image(h, kDefaultHomFraction, pl) == MIH_OK && pl.p1 > 0 && (double)pl.tile_bytes <= 0.97 * (double)x_bytes &&
                    hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                    free_b >= pl.tile_bytes + plan_list_bytes(h, pl) + kImageMargin &&
                    build_image(h, kDefaultHomFraction, pl, im) == MIH_OK;
    (void)hipGetLastError();
    if (ok) set_image(h, im);
    else { std::lock_guard<std::mutex> g(h->img_mu); h->img_declined = true; }
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_mat_score_image(mih_mat *h, int mode, double max_hom_fraction, int64_t *bytes, int64_t *class1_cols)
{
    if (!h) { set_error("null handle"); return MIH_BAD_ARG; }
    if (h->kind != 0) { set_error("only a 2-bit matrix has a score image"); return MIH_BAD_ARG; }
    if (mode != MIH_IMAGE_QUERY && mode != MIH_IMAGE_BUILD && mode != MIH_IMAGE_RELEASE) { set_error("mode must be MIH_IMAGE_QUERY, MIH_IMAGE_BUILD or MIH_IMAGE_RELEASE"); return MIH_BAD_ARG; }
    MIH_HIP(hipSetDevice(h->device));
    if (mode == MIH_IMAGE_RELEASE) set_image(h, nullptr);
    if (mode == MIH_IMAGE_BUILD) {
        const double tau = max_hom_fraction > 0.0 ? max_hom_fraction : kDefaultHomFraction;
        if (!(tau <= 1.0)) { set_error("max_hom_fraction must be at most 1"); return MIH_BAD_ARG; }
        ImagePlan pl;
        MIH_TRY(plan_image(h, tau, pl));
        // no column qualifies: an image would be a copy of the matrix
        if (pl.p1 == 0) { set_error("no column has at most %g x n dosage-2 entries: the score image would save nothing", tau); return MIH_BAD_ARG; }
        std::shared_ptr<const ScoreImage> im;
        MIH_TRY(build_image(h, tau, pl, im));
        set_image(h, im);
    }
    const std::shared_ptr<const ScoreImage> im = score_image_of(h);
    if (bytes) *bytes = im ? (int64_t)im->bytes : 0;
    if (class1_cols) *class1_cols = im ? im->p1 : 0;
    return MIH_OK;
}

int mih_device_trim(int device, int64_t *released_bytes)
{
    MIH_TRY(select_device(device));
    const size_t b = trim_score_images(device);
    if (released_bytes) *released_bytes = (int64_t)b;
    return MIH_OK;
}

}  // extern "C"
