// The two identities of the score image (csrc/score_image.h) against their plain definitions, as a stand-alone host program:
// plain g++ with -fsanitize=address,undefined, no HIP, no GPU.  Prints "ok" lines; any mismatch ends it with status 1.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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

// 1. every row of a 128-row block lands on the element k_digits gives it.  The matrix's tile keeps row 64 e + 32 h + 16 u + s of a
// block in lane (m, h), dword 2 e + u, bits 2s, 2s + 1; the one-bit tile keeps the 32 rows of (e, h) in one dword.  Expanding that
// dword as the kernel does -- A-fragment dword k = (dword >> k) & 0x11111111 -- must give FP4 code 1 in exactly the nibble of
// element el = 8 (2u + (s & 1)) + (s >> 1), i.e. nibble el % 8 of fragment dword el / 8: the place the 2-bit expansion
// (x & M, (x >> 2) & M, y & M, (y >> 2) & M with M = 0x33333333) puts the row's code, and k_digits the row's digit.
static int check_row_map()
{
    for (int code = 1; code <= 2; ++code)
        for (int row = 0; row < 128; ++row) {
            const int e = row >> 6, h = (row >> 5) & 1, r = row & 31, u = r >> 4, s = r & 15;
            uint32_t tile[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};          // lane h of one SNP: four 2-bit dwords
            tile[h][2 * e + u] = (uint32_t)code << (2 * s);
            for (int hh = 0; hh < 2; ++hh)
                for (int ee = 0; ee < 2; ++ee) {
                    const uint32_t one = onebit_pack(tile[hh][2 * ee], tile[hh][2 * ee + 1]);
                    const uint32_t M = 0x33333333u, x = tile[hh][2 * ee], y = tile[hh][2 * ee + 1];
                    const uint32_t two[4] = {x & M, (x >> 2) & M, y & M, (y >> 2) & M};
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t frag = (one >> k) & 0x11111111u;
                        uint32_t want = 0;
                        for (int q = 0; q < 8; ++q) if ((two[k] >> (4 * q)) & 15u) want |= 1u << (4 * q);      // the plane [g >= 1]
                        if (frag != want) return fail("fragment", row, hh * 2 + ee, k);
                    }
                    if (hh == h && ee == e) {
                        const int el = 8 * (2 * u + (s & 1)) + (s >> 1);
                        if (onebit_element(r) != el) return fail("element", row, onebit_element(r), el);
                        if (one != (1u << onebit_pos(r))) return fail("bit", row, one, onebit_pos(r));
                        if (onebit_pos(r) != 4 * (el & 7) + (el >> 3)) return fail("pos", row, onebit_pos(r), el);
                    } else if (one != 0) return fail("stray bit", row, hh, ee);
                }
        }
    // a full dword pair: every row at once, and code 0 stays 0
    for (int it = 0; it < 1000; ++it) {
        uint32_t x0 = 0, x1 = 0, want = 0;
        for (int r = 0; r < 32; ++r) {
            const uint32_t g = (uint32_t)(rnd() % 3);
            (r < 16 ? x0 : x1) |= g << (2 * (r & 15));
            if (g) want |= 1u << onebit_pos(r);
        }
        if (onebit_pack(x0, x1) != want) return fail("random dwords", it, onebit_pack(x0, x1), want);
    }
    printf("ok row map\n");
    return 0;
}

// 2. sum of d_t over a list of R, both ways of driving HomSum (add: folds and flushes by itself; add_chunk: the call
// k_xtv_hom makes per 16-byte load -- 8 terms, a fold after every 4, a flush before 85 could be passed -- padding entries included), against the division loop
static int check_sums(const std::vector<long long> &Rs, const char *what)
{
    long long want[kHomDigits] = {0};
    for (long long R : Rs) {
        int d[kHomDigits];
        digits_of(R, d);
        long long back = 0;
        for (int t = kHomDigits - 1; t >= 0; --t) back = back * 4 + d[t];
        if (back != R) return fail("digits do not recombine", R, back, 0);
        for (int t = 0; t < kHomDigits; ++t) want[t] += d[t];
    }
    HomSum a, b;
    a.init(); b.init();
    for (long long R : Rs) a.add(hom_u(R));
    a.flush();
    for (size_t i = 0; i < Rs.size(); i += 5) {            // chunks of 8 entries: 5 live, 3 padding
        uint64_t u8[kHomChunk];
        for (size_t j = 0; j < (size_t)kHomChunk; ++j) {
            const bool live = j < 5 && i + j < Rs.size();
            u8[j] = live ? hom_u(Rs[i + j]) : hom_u(0);           // padding: the row of R = 0
        }
        b.add_chunk(u8);                                           // the kernel's own call
    }
    b.flush();
    for (int t = 0; t < kHomDigits; ++t) {
        if (a.digit_sum(t) != want[t]) return fail(what, t, a.digit_sum(t), want[t]);
        if (b.digit_sum(t) != want[t]) return fail(what, 100 + t, b.digit_sum(t), want[t]);
    }
    return 0;
}

int main()
{
    if (check_row_map()) return 1;
    const long long top = (1ll << 54) - 1;
    std::vector<long long> Rs;
    for (int i = 0; i < 1000; ++i) Rs.push_back((long long)(rnd() % (2ull * (uint64_t)top + 1)) - top);
    if (check_sums(Rs, "random")) return 1;
    Rs.assign(1000, top);                   // every digit at its largest: u_t = 3 wherever R's digit is 1
    if (check_sums(Rs, "top")) return 1;
    Rs.assign(1000, -top);
    if (check_sums(Rs, "-top")) return 1;
    Rs.assign(1000, 0x0055555555555555ll);  // d_t = 1 in every place: u_t = 3 in all 28 fields, 1000 terms = 11 flush intervals
    if (check_sums(Rs, "all ones")) return 1;
    Rs.assign(1000, -0x00AAAAAAAAAAAAAAll); // d_t = -2 in every place: U = 0
    if (check_sums(Rs, "all minus two")) return 1;
    Rs.clear();
    for (int i = 0; i < 1000; ++i) Rs.push_back(i % 3 == 0 ? top : i % 3 == 1 ? -top : 0);
    if (check_sums(Rs, "mixed")) return 1;
    Rs.assign(300, top);                    // more than 255 terms between two explicit flushes is what the cadence prevents:
    {                                       // show that 85 is the limit -- 86 terms of u_t = 3 without a flush do overflow a field
        HomSum c; c.init();
        for (int i = 0; i < 86; ++i) { c.accumulate(hom_u(0x0055555555555555ll)); if (i % 5 == 4) c.fold4(); }
        c.flush();
        if (c.digit_sum(0) == 86) return fail("86 unflushed terms should overflow an 8-bit field", c.digit_sum(0), 0, 0);
        HomSum d; d.init();
        for (int i = 0; i < 85; ++i) { d.accumulate(hom_u(0x0055555555555555ll)); if (i % 5 == 4) d.fold4(); }
        d.flush();
        for (int t = 0; t < kHomDigits; ++t) if (d.digit_sum(t) != 85) return fail("85 unflushed terms", t, d.digit_sum(t), 85);
    }
    if (check_sums(Rs, "300 x top")) return 1;
    printf("ok digit sums\n");
    return 0;
}
