// score_image.h -- the two identities the score image of a 2-bit matrix rests on (score_image.hip), as functions the host can call
// too: tests/score_image_harness.cpp checks them against the plain definitions.  No HIP types: plain C++.
#pragma once
#include <cstdint>
#if defined(__HIPCC__)
#define MIH_HD __host__ __device__ inline
#else
#define MIH_HD inline
#endif

namespace mih {

// Class-1 tile: a lane's dword holds the 32 rows of one (SNP, 64-row half e, K-half h) at one bit each.  Row r = 16 u + s of those
// 32 is element el = 8 (2u + (s & 1)) + (s >> 1) of the A fragment (k_digits' order); element 8k + q sits at bit 4q + k, so that
// (dword >> k) & 0x11111111 is A-fragment dword k of the plane [g >= 1] with FP4 code 0001 = 0.5 in every set nibble.
MIH_HD int onebit_element(int r) { const int u = r >> 4, s = r & 15; return 8 * (2 * u + (s & 1)) + (s >> 1); }
MIH_HD int onebit_pos(int r) { const int el = onebit_element(r); return 4 * (el & 7) + (el >> 3); }
// the one-bit dword of the matrix's two 2-bit dwords of those rows (x0: rows 0..15, x1: rows 16..31; codes 0, 1, 2)
MIH_HD uint32_t onebit_pack(uint32_t x0, uint32_t x1)
{
    const uint32_t n0 = (x0 | (x0 >> 1)) & 0x55555555u, n1 = (x1 | (x1 >> 1)) & 0x55555555u;      // bit 2s: g_s >= 1
    const uint32_t t0 = (n0 & 0x11111111u) | ((n0 & 0x44444444u) >> 1);                          // s = 2a + b: bit 4a + 2b -> 4a + b
    const uint32_t t1 = (n1 & 0x11111111u) | ((n1 & 0x44444444u) >> 1);
    return t0 | (t1 << 2);
}

// Sums of the balanced base-4 digits d_t in {-2,-1,0,1} of integers R, |R| < 2^54, over a list of rows.  k_digits forms
// U = R + 0x00AAAAAAAAAAAAAA, whose ORDINARY base-4 digits are u_t = d_t + 2, so sum d_t = sum u_t - 2 * terms.  The 28 two-bit
// fields of U are added in SWAR form on 32-bit words (w = 0: digits 0..15, w = 1: digits 16..27), in two levels:
//   level 1  n4[2w + c] += (word_w >> 2c) & 0x33333333: digit 16w + 2j + c in the 4-bit field j -- at most kHomFold terms of 3;
//   level 2  fold4(): n8[4w + 2c + h] += (n4[2w + c] >> 4h) & 0x0F0F0F0F: digit 16w + 4i + 2h + c in byte i -- at most kHomFlush
//            terms of 3 before flush() empties the bytes into the 32-bit counters.
// A list's padding entry reads U of R = 0 (every u_t = 2, d_t = 0): it is a term like any other and adds nothing.
constexpr int kHomDigits = 28;
constexpr int kHomFold = 5;
constexpr int kHomFlush = 85;
constexpr int kHomChunk = 8;          // entries of one 16-byte load of a list
constexpr int kHomChunkFold = 4;      // add_chunk folds after every 4 terms (<= kHomFold)
struct HomSum {
    uint32_t n4[4], n8[8];
    uint32_t cnt[kHomDigits];
    uint32_t terms, pend4, pend;
    MIH_HD void init()
    {
        for (int k = 0; k < 4; ++k) n4[k] = 0;
        for (int k = 0; k < 8; ++k) n8[k] = 0;
        for (int t = 0; t < kHomDigits; ++t) cnt[t] = 0;
        terms = 0; pend4 = 0; pend = 0;
    }
    // one term, no fold: the caller calls fold4() after at most kHomFold of them and flush() after at most kHomFlush
    MIH_HD void accumulate(uint64_t U)
    {
        const uint32_t lo = (uint32_t)U, hi = (uint32_t)(U >> 32), M = 0x33333333u;
        n4[0] += lo & M; n4[1] += (lo >> 2) & M; n4[2] += hi & M; n4[3] += (hi >> 2) & M;
        ++terms;
    }
    MIH_HD void fold4()
    {
        for (int x = 0; x < 4; ++x) {
            n8[2 * x] += n4[x] & 0x0F0F0F0Fu;
            n8[2 * x + 1] += (n4[x] >> 4) & 0x0F0F0F0Fu;
            n4[x] = 0;
        }
        pend4 = 0;
    }
    MIH_HD void flush()
    {
        fold4();
        for (int w = 0; w < 2; ++w)
            for (int c = 0; c < 2; ++c)
                for (int h = 0; h < 2; ++h) {
                    for (int i = 0; i < 4; ++i) {
                        const int t = 16 * w + 4 * i + 2 * h + c;
                        if (t < kHomDigits) cnt[t] += (n8[4 * w + 2 * c + h] >> (8 * i)) & 0xFFu;
                    }
                    n8[4 * w + 2 * c + h] = 0;
                }
        pend = 0;
    }
    // a list's chunk of kHomChunk terms, the cadence of k_xtv_hom: a fold after every kHomChunkFold terms, and a flush when the
    // NEXT chunk could pass kHomFlush terms since the last one
    MIH_HD void add_chunk(const uint64_t (&U)[8])
    {
        static_assert(kHomChunk == 8 && kHomChunkFold <= kHomFold && kHomChunk % kHomChunkFold == 0, "chunk cadence");
#if defined(__HIPCC__)
        #pragma unroll      // (U stays in registers)
#endif
        for (int i = 0; i < kHomChunk; ++i) {
            accumulate(U[i]);
            if (i % kHomChunkFold == kHomChunkFold - 1) fold4();
        }
        if ((pend += kHomChunk) > (uint32_t)(kHomFlush - kHomChunk)) flush();
    }
    // one term; folds and flushes by itself
    MIH_HD void add(uint64_t U)
    {
        accumulate(U);
        if (++pend4 == (uint32_t)kHomFold) fold4();
        if (++pend == (uint32_t)kHomFlush) flush();
    }
    MIH_HD int32_t digit_sum(int t) const { return (int32_t)cnt[t] - 2 * (int32_t)terms; }      // after a flush()
};
MIH_HD uint64_t hom_u(long long R) { return (uint64_t)R + 0x00AAAAAAAAAAAAAAull; }

// Where the 16-byte chunks of a slot group's lists live.  A slot group is the 64 consecutive slots one wave of k_xtv_hom owns; per
// (slice, group, sub-slice) its lists share one block of sum cnt[] chunks, chunk-index-major and compacted: chunk 0 of every
// lane that has one, in lane order, then chunk 1 of every lane that has two, ...  A wave's load of its chunks c is then one
// contiguous run.  cnt: the 64 lanes' chunk counts; the results are relative to the block's first chunk.
constexpr int kHomGroup = 64;
// first place of the chunks of index c: sum of min(cnt[l], c)
MIH_HD uint32_t hom_chunk_base(const uint32_t *cnt, uint32_t c)
{
    uint32_t s = 0;
    for (int l = 0; l < kHomGroup; ++l) s += cnt[l] < c ? cnt[l] : c;
    return s;
}
// the lane's place among them: the lower lanes whose list is longer than c chunks (the kernel: one ballot, one masked bit count)
MIH_HD uint32_t hom_chunk_rank(const uint32_t *cnt, int lane, uint32_t c)
{
    uint32_t r = 0;
    for (int l = 0; l < lane; ++l) r += cnt[l] > c ? 1u : 0u;
    return r;
}
// place of chunk c < cnt[lane] of the lane's list
MIH_HD uint32_t hom_chunk_slot(const uint32_t *cnt, int lane, uint32_t c) { return hom_chunk_base(cnt, c) + hom_chunk_rank(cnt, lane, c); }

}  // namespace mih
