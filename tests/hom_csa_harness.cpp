// The carry-save positional counter of k_xtv_hom (HomCsa, csrc/score_image.h) against the division-loop definition of the balanced
// base-4 digits and against HomSum, as a stand-alone host program: plain g++ with -fsanitize=address,undefined, no HIP, no GPU.
// Prints "ok" lines; any mismatch ends it with status 1.
#include "score_image.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mih;

static int fail(const char *what, long long a, long long b, long long c)
{
    fprintf(stderr, "FAIL %s: %lld %lld %lld\n", what, a, b, c);
    return 1;
}

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// the balanced base-4 digits by the division loop (k_digits' reference branch): d in {-2,-1,0,1}
static void digits_of(long long R, int d[kHomDigits])
{
    for (int t = 0; t < kHomDigits; ++t) {
        const int mm = (int)(R & 3);
        d[t] = mm < 2 ? mm : mm - 4;
        R = (R - d[t]) >> 2;
    }
}

// A list as the image stores it: `live` entries, padded with entries of R = 0 to whole chunks of 8, plus `pad_chunks` chunks of
// padding only.  The ways of driving the counter:
//   a  HomCsa::add, term by term (padding entries too: they are terms);
//   b  HomCsa::add_chunk, chunk by chunk: groups of kCsaGroup chunks, the last one closed with zero words by finish();
//   c  the kernel's own calls: the list cut into sub-slices at `cuts`; per sub-slice rounds of kCsaGroup chunks through chunk_carry,
//      pair_carry and add_pairs with zero carry words where the list has ended, `idle` more rounds of zero carry words (a wave
//      runs as long as its longest list), and terms += 8 * chunks;
// against the division loop and against HomSum.
static int check_list(const std::vector<long long> &live, size_t pad_chunks, const std::vector<size_t> &cuts, int idle, const char *what)
{
    std::vector<uint64_t> U;
    for (long long R : live) U.push_back(hom_u(R));
    while (U.size() % kHomChunk) U.push_back(hom_u(0));
    for (size_t i = 0; i < pad_chunks * kHomChunk; ++i) U.push_back(hom_u(0));
    long long want[kHomDigits] = {0};
    for (long long R : live) {
        int d[kHomDigits];
        digits_of(R, d);
        long long back = 0;
        for (int t = kHomDigits - 1; t >= 0; --t) back = back * 4 + d[t];
        if (back != R) return fail("digits do not recombine", R, back, 0);
        for (int t = 0; t < kHomDigits; ++t) want[t] += d[t];
    }
    HomSum h;
    h.init();
    for (uint64_t u : U) h.add(u);
    h.flush();
    HomCsa a, b, c;
    a.init(); b.init(); c.init();
    for (uint64_t u : U) a.add(u);
    a.finish();
    const size_t nchunks = U.size() / kHomChunk;
    for (size_t k = 0; k < nchunks; ++k) {
        uint64_t u8[kHomChunk];
        for (int i = 0; i < kHomChunk; ++i) u8[i] = U[k * kHomChunk + i];
        b.add_chunk(u8);
    }
    b.finish();
    size_t k0 = 0;
    for (size_t ci = 0; ci <= cuts.size(); ++ci) {
        const size_t k1 = ci < cuts.size() ? (cuts[ci] < nchunks ? cuts[ci] : nchunks) : nchunks;
        if (k1 < k0) return fail("cuts must ascend", (long long)k0, (long long)k1, 0);
        const size_t cnt = k1 - k0, rounds = (cnt + kCsaGroup - 1) / kCsaGroup + (size_t)idle;
        for (size_t r = 0; r < rounds; ++r) {
            uint32_t c16[kCsaGroup / 2][2];
            for (int j2 = 0; j2 < kCsaGroup / 2; ++j2) {
                uint32_t c8[2][2] = {{0, 0}, {0, 0}};
                for (int j1 = 0; j1 < 2; ++j1) {
                    const size_t cj = r * kCsaGroup + 2 * (size_t)j2 + (size_t)j1;
                    if (cj < cnt) {
                        uint64_t u8[kHomChunk];
                        for (int i = 0; i < kHomChunk; ++i) u8[i] = U[(k0 + cj) * kHomChunk + i];
                        c.chunk_carry(u8, c8[j1]);
                    }
                }
                c.pair_carry(c8[0], c8[1], c16[j2]);
            }
            c.add_pairs(c16[0], c16[1]);
        }
        c.terms += (uint32_t)(kHomChunk * cnt);
        k0 = k1;
    }
    c.finish();
    for (int t = 0; t < kHomDigits; ++t) {
        if (h.digit_sum(t) != want[t]) return fail(what, t, h.digit_sum(t), want[t]);
        if (a.digit_sum(t) != want[t]) return fail(what, 100 + t, a.digit_sum(t), want[t]);
        if (b.digit_sum(t) != want[t]) return fail(what, 200 + t, b.digit_sum(t), want[t]);
        if (c.digit_sum(t) != want[t]) return fail(what, 300 + t, c.digit_sum(t), want[t]);
    }
    if (a.terms != h.terms || b.terms != h.terms || c.terms != h.terms) return fail("terms", a.terms, b.terms, c.terms);
    return 0;
}
static int check_list(const std::vector<long long> &live, const char *what)
{
    return check_list(live, 0, {}, 0, what);
}

static const long long kTop = (1ll << 54) - 1;
static const long long kAllOnes = 0x0055555555555555ll;       // d_t = 1 in every place: every field of U is 3
static const long long kAllMinusTwo = -0x00AAAAAAAAAAAAAAll;  // d_t = -2 in every place: U = 0
static long long random_R() { return (long long)(rnd() % (2ull * (uint64_t)kTop + 1)) - kTop; }
// the values whose U is all zeros or all threes in some or all fields, and random ones
static long long pick_R(int kind)
{
    switch (kind % 6) {
    case 0: return kTop;
    case 1: return -kTop;
    case 2: return kAllOnes;
    case 3: return kAllMinusTwo;
    case 4: return 0;
    default: return random_R();
    }
}

int main()
{
    // the empty list, one term, and every length up to 400: an odd tail at every adder level (term, chunk, pair, group), the
    // group of 32 terms and the field flush after kCsaFlush groups (160 terms, add()'s as well) with a few groups beyond
    static_assert(kCsaGroup * kHomChunk == 32 && kCsaFlush * kCsaGroup * kHomChunk == 160, "the lengths below are built on these");
    for (int kind = 0; kind < 7; ++kind)
        for (size_t len = 0; len <= 400; ++len) {
            std::vector<long long> Rs;
            for (size_t i = 0; i < len; ++i) Rs.push_back(kind < 6 ? pick_R(kind) : pick_R((int)(rnd() % 6)));
            if (check_list(Rs, "length")) return 1;
        }
    printf("ok lengths 0..400\n");
    // at, one below and one above the flush cadence, counted in the terms, chunks and groups a list really has: 159, 160, 161 terms
    // (above), 19, 20, 21 chunks with 1 to 8 live entries in the last, and the same after a first flush (39, 40, 41 chunks)
    for (size_t chunks : {(size_t)kCsaFlush * kCsaGroup - 1, (size_t)kCsaFlush * kCsaGroup, (size_t)kCsaFlush * kCsaGroup + 1,
                          (size_t)2 * kCsaFlush * kCsaGroup - 1, (size_t)2 * kCsaFlush * kCsaGroup, (size_t)2 * kCsaFlush * kCsaGroup + 1})
        for (size_t last = 1; last <= 8; ++last) {
            std::vector<long long> Rs((chunks - 1) * kHomChunk + last, kAllOnes);
            if (check_list(Rs, "flush cadence")) return 1;
        }
    printf("ok flush cadence\n");
    // the fields' bound itself: kCsaFlush carry words of 3 fill a field, one more overflows it
    {
        HomCsa x; x.init();
        for (int i = 0; i < kCsaFlush; ++i) { x.add_carry32(0, 0xFFFFFFFFu); x.add_carry32(1, 0x00FFFFFFu); }
        x.finish();
        for (int t = 0; t < kHomDigits; ++t) if (x.digit_sum(t) != 32 * 3 * kCsaFlush) return fail("full fields", t, x.digit_sum(t), 32 * 3 * kCsaFlush);
        HomCsa y; y.init();
        for (int i = 0; i < kCsaFlush + 1; ++i) y.add_carry32(0, 0xFFFFFFFFu);
        y.finish();
        if (y.digit_sum(0) == 32 * 3 * (kCsaFlush + 1)) return fail("one carry word more should overflow a 4-bit field", y.digit_sum(0), 0, 0);
    }
    printf("ok field bound\n");
    // lists of padding entries only, and lists that end in 1 to 7 padding entries and whole chunks of them
    for (size_t pad = 0; pad <= 45; ++pad)
        for (size_t len : {(size_t)0, (size_t)1, (size_t)7, (size_t)9, (size_t)33, (size_t)161}) {
            std::vector<long long> Rs;
            for (size_t i = 0; i < len; ++i) Rs.push_back(pick_R((int)i));
            if (check_list(Rs, pad, {}, 0, "padding")) return 1;
        }
    printf("ok padding\n");
    // the kernel's cadence: sub-slices of every length, idle rounds, seeded random lists
    for (int it = 0; it < 400; ++it) {
        const size_t len = (size_t)(rnd() % 700);
        std::vector<long long> Rs;
        const int kind = (int)(rnd() % 7);
        for (size_t i = 0; i < len; ++i) Rs.push_back(kind < 6 ? pick_R(kind) : pick_R((int)(rnd() % 6)));
        std::vector<size_t> cuts;
        size_t at = 0;
        const size_t nchunks = (len + kHomChunk - 1) / kHomChunk, step = 1 + (size_t)(rnd() % 12);
        while (at < nchunks) { at += (size_t)(rnd() % (step + 1)); cuts.push_back(at); }      // (empty sub-slices too)
        if (check_list(Rs, (size_t)(rnd() % 3), cuts, (int)(rnd() % 3), "sub-slices")) return 1;
    }
    printf("ok sub-slices\n");
    // the overflow bound of the header: 2^22 terms with every field of U at 3
    {
        std::vector<long long> Rs((size_t)1 << 22, kAllOnes);
        if (check_list(Rs, 0, {(size_t)1 << 17, (size_t)3 << 17}, 1, "2^22 terms")) return 1;
    }
    printf("ok 2^22 terms\n");
    return 0;
}
