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

// The same sums by counting bit positions (what k_xtv_hom runs; HomSum above is the plain statement it is held to).  With C[b] the
// number of terms whose U has bit b set, sum u_t = C[2t] + 2 C[2t + 1]: a word whose bit b is a count's bit of weight v, read as
// 2-bit fields, is a word of digit sums of weight v.  The counts are kept bit-sliced on the two 32-bit halves w of U (as above):
//   s[v][w], v = 0..4   bit b = bit v of C[32w + b] (weights 1, 2, 4, 8, 16), by carry-save adders -- csa(): three operations, two on gfx950;
//   chunk_carry()       a chunk's 8 words into s[0..2] with 7 adders a half; what comes out is one carry word of weight 8;
//   pair_carry()        the carry words of two consecutive chunks into s[3]: one carry word of weight 16;
//   add_pairs()         the carry words of two consecutive pairs into s[4]: one carry word of weight 32 per group of kCsaGroup = 4
//                       chunks, whose 2-bit fields go to the 4-bit fields f[c][w] += (carry >> 2c) & 0x33333333 (digit
//                       16w + 2j + c in field j);
//   flush()             the 4-bit fields, times 32, into the 32-bit counters cnt[].  A field gains at most 3 per carry word:
//                       flush() runs BEFORE the carry word that would be the (kCsaFlush + 1)-th since the last one;
//   finish()            the planes into cnt[] as well, once per list: per half and j, sum_v ((s[v][w] >> 2j) & 0x03030303) << v has
//                       digit 16w + 4i + j in byte i, at most 3 * 31 = 93.
// A chunk that is missing from a pair or a group is a zero carry word: it adds nothing and is no term.  A list's padding entry
// (U of R = 0) is a term.  Every plane is a count modulo 32, and cnt[t] <= 3 * 2^22 < 2^24 for the 2^22 terms a lane can see in a
// slice.
constexpr int kCsaGroup = 4;          // chunks per carry word of weight 32: 4 * kHomChunk = 32 terms
constexpr int kCsaFlush = 5;          // carry words between two flush(): 5 * 3 = 15 fits a 4-bit field, 6 * 3 does not
constexpr int kCsaPlanes = 5;         // weights 1 .. 16: the planes hold a count below kCsaGroup * kHomChunk = 32
struct HomCsa {
    uint32_t s[kCsaPlanes][2];
    uint32_t f[2][2];
    uint32_t cnt[kHomDigits];
    uint32_t terms;
    uint32_t pend;                           // carry words the fields may hold: groups, and add()'s blocks of 32 terms begun
    uint32_t pend1;                          // add()'s terms in its current block of 32
    uint32_t open[kCsaGroup][2], phase;      // add_chunk's carry words of a group that is not full yet
    MIH_HD void init()
    {
        for (int v = 0; v < kCsaPlanes; ++v) s[v][0] = s[v][1] = 0;
        for (int c = 0; c < 2; ++c) f[c][0] = f[c][1] = 0;
        for (int t = 0; t < kHomDigits; ++t) cnt[t] = 0;
        for (int c = 0; c < kCsaGroup; ++c) open[c][0] = open[c][1] = 0;
        terms = 0; pend = 0; pend1 = 0; phase = 0;
    }
    // full adder on words: a + b + c = lo + 2 hi in every bit position (lo may be one of the inputs)
    static MIH_HD void csa(uint32_t &hi, uint32_t &lo, uint32_t a, uint32_t b, uint32_t c)
    {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
        // (two three-input bit operations, by truth table: the majority 0xE8 and the parity 0x96.  Left to itself the compiler
        // regroups the adders of chunk_carry() into four to five two- and three-input operations each.)
        const uint32_t m = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
        lo = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
        hi = m;
#else
        const uint32_t t = a ^ b;
        hi = (t & c) | (~t & a);
        lo = t ^ c;
#endif
    }
    // a chunk's 8 words into the planes of weight 1, 2, 4; c8: the carry word of weight 8 of either half.  Counts no terms.
    MIH_HD void chunk_carry(const uint64_t (&U)[8], uint32_t (&c8)[2])
    {
        static_assert(kHomChunk == 8, "seven adders reduce eight words");
        for (int w = 0; w < 2; ++w) {
            uint32_t x[8], a2, b2, c2, d2, a4, b4;
            for (int i = 0; i < 8; ++i) x[i] = (uint32_t)(U[i] >> (32 * w));
            csa(a2, s[0][w], s[0][w], x[0], x[1]);
            csa(b2, s[0][w], s[0][w], x[2], x[3]);
            csa(a4, s[1][w], s[1][w], a2, b2);
            csa(c2, s[0][w], s[0][w], x[4], x[5]);
            csa(d2, s[0][w], s[0][w], x[6], x[7]);
            csa(b4, s[1][w], s[1][w], c2, d2);
            csa(c8[w], s[2][w], s[2][w], a4, b4);
        }
    }
    // two carry words of weight 8 (zero where the list has no chunk any more) into the plane of weight 8; c16: the carry of weight 16
    MIH_HD void pair_carry(const uint32_t (&a8)[2], const uint32_t (&b8)[2], uint32_t (&c16)[2])
    {
        for (int w = 0; w < 2; ++w) csa(c16[w], s[3][w], s[3][w], a8[w], b8[w]);
    }
    // a carry word of weight 32 into the 4-bit fields (the caller has made room: room_for_carry())
    MIH_HD void add_carry32(int w, uint32_t c32)
    {
        for (int c = 0; c < 2; ++c) f[c][w] += (c32 >> (2 * c)) & 0x33333333u;
    }
    MIH_HD void room_for_carry()
    {
        if (pend == (uint32_t)kCsaFlush) flush();
        ++pend;
    }
    // a group's two carry words of weight 16 into the plane of weight 16 and the fields; flushes at its own cadence.
    // k_xtv_hom's call: once per round of kCsaGroup chunks, by the whole wave.
    MIH_HD void add_pairs(const uint32_t (&a16)[2], const uint32_t (&b16)[2])
    {
        static_assert(kCsaGroup == 4 && kCsaPlanes == 5, "three adders reduce four carry words of weight 8 to one of weight 32");
        room_for_carry();
        for (int w = 0; w < 2; ++w) {
            uint32_t c32;
            csa(c32, s[4][w], s[4][w], a16[w], b16[w]);
            add_carry32(w, c32);
        }
    }
    // the carry words of a group's chunks
    MIH_HD void add_group(const uint32_t (&c8)[kCsaGroup][2])
    {
        uint32_t a16[2], b16[2];
        pair_carry(c8[0], c8[1], a16);
        pair_carry(c8[2], c8[3], b16);
        add_pairs(a16, b16);
    }
    MIH_HD void flush()
    {
        for (int w = 0; w < 2; ++w)
            for (int c = 0; c < 2; ++c) {
                for (int j = 0; j < 8; ++j) {
                    const int t = 16 * w + 2 * j + c;
                    if (t < kHomDigits) cnt[t] += ((f[c][w] >> (4 * j)) & 0xFu) << kCsaPlanes;
                }
                f[c][w] = 0;
            }
        pend = 0; pend1 = 0;
    }
    // a list's chunk of kHomChunk terms; the group closes with its kCsaGroup-th chunk (or in finish())
    MIH_HD void add_chunk(const uint64_t (&U)[8])
    {
        chunk_carry(U, open[phase]);
        terms += kHomChunk;
        if (++phase == (uint32_t)kCsaGroup) close_group();
    }
    MIH_HD void close_group()
    {
        add_group(open);
        for (int c = 0; c < kCsaGroup; ++c) open[c][0] = open[c][1] = 0;
        phase = 0;
    }
    // one term: a half-adder chain through the planes.  A bit position sends a carry of weight 32 once in 32 terms, but the
    // positions do so at different terms: a block of 32 terms counts as one carry word from its first term on (T terms since a
    // flush() have sent a position at most ceil(T / 32) carries, its plane count being below 32 at the flush).
    MIH_HD void add(uint64_t U)
    {
        if (pend1 == 0) room_for_carry();
        if (++pend1 == (uint32_t)(kCsaGroup * kHomChunk)) pend1 = 0;
        for (int w = 0; w < 2; ++w) {
            uint32_t c = (uint32_t)(U >> (32 * w));
            for (int v = 0; v < kCsaPlanes; ++v) { const uint32_t t = s[v][w] & c; s[v][w] ^= c; c = t; }
            add_carry32(w, c);
        }
        ++terms;
    }
    // closes an open group with zero words and empties the fields and the planes into cnt[]: digit_sum() is exact from here on
    // (more terms may follow)
    MIH_HD void finish()
    {
        if (phase != 0) close_group();
        flush();
        for (int w = 0; w < 2; ++w)
            for (int j = 0; j < 4; ++j) {
                uint32_t b = 0;
                for (int v = 0; v < kCsaPlanes; ++v) b += ((s[v][w] >> (2 * j)) & 0x03030303u) << v;
                for (int i = 0; i < 4; ++i) {
                    const int t = 16 * w + 4 * i + j;
                    if (t < kHomDigits) cnt[t] += (b >> (8 * i)) & 0xFFu;
                }
            }
        for (int v = 0; v < kCsaPlanes; ++v) s[v][0] = s[v][1] = 0;
    }
    MIH_HD int32_t digit_sum(int t) const { return (int32_t)cnt[t] - 2 * (int32_t)terms; }      // after finish()
};

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
