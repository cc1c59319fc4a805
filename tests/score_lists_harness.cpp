// Where the chunks of a slot group's exception lists live (hom_chunk_base / hom_chunk_rank / hom_chunk_slot, csrc/score_image.h),
// as a stand-alone host program: plain g++ with -fsanitize=address,undefined, no HIP, no GPU.  For a vector of 64 chunk counts the
// map (lane, chunk) -> place must be a bijection onto [0, sum of the counts), the chunks of one index c must occupy one
// contiguous run in lane order, and the run of c + 1 must start where the run of c ends.  Prints "ok" lines; any mismatch ends it
// with status 1.
#include "score_image.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mih;

static int fail(const char *what, const char *which, long long a, long long b, long long c)
{
    fprintf(stderr, "FAIL %s (%s): %lld %lld %lld\n", what, which, a, b, c);
    return 1;
}

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static int check(const std::vector<uint32_t> &cnt, const char *which)
{
    if (cnt.size() != (size_t)kHomGroup) return fail("64 counts", which, (long long)cnt.size(), 0, 0);
    uint32_t total = 0, longest = 0;
    for (uint32_t c : cnt) { total += c; if (c > longest) longest = c; }
    std::vector<int> seen(total, 0);
    uint32_t next = 0;                                      // where the run of chunk index c must start
    for (uint32_t c = 0; c < longest; ++c) {
        if (hom_chunk_base(cnt.data(), c) != next) return fail("run does not follow its predecessor", which, c, hom_chunk_base(cnt.data(), c), next);
        for (int lane = 0; lane < kHomGroup; ++lane) {
            if (cnt[(size_t)lane] <= c) continue;
            const uint32_t at = hom_chunk_slot(cnt.data(), lane, c);
            if (at != next) return fail("run not contiguous in lane order", which, lane, c, at);       // (also: at >= total cannot pass)
            if (at >= total) return fail("place outside the block", which, lane, c, at);
            if (seen[at]++) return fail("place taken twice", which, lane, c, at);
            if (hom_chunk_rank(cnt.data(), lane, c) != at - hom_chunk_base(cnt.data(), c)) return fail("rank", which, lane, c, at);
            ++next;
        }
    }
    if (next != total) return fail("not onto", which, next, total, 0);
    if (hom_chunk_base(cnt.data(), longest) != total) return fail("end of the block", which, hom_chunk_base(cnt.data(), longest), total, 0);
    for (uint32_t i = 0; i < total; ++i) if (seen[i] != 1) return fail("hole", which, i, seen[i], 0);
    return 0;
}

int main()
{
    std::vector<uint32_t> cnt((size_t)kHomGroup, 0u);
    if (check(cnt, "every lane 0")) return 1;
    for (int lane : {0, 31, 32, 63})
        for (uint32_t len : {1u, 7u}) {
            cnt.assign((size_t)kHomGroup, 0u);
            cnt[(size_t)lane] = len;
            if (check(cnt, "one lane alone")) return 1;
        }
    printf("ok empty and single lanes\n");
    for (uint32_t len : {1u, 2u, 11u}) {
        cnt.assign((size_t)kHomGroup, len);
        if (check(cnt, "all equal")) return 1;
    }
    for (int l = 0; l < kHomGroup; ++l) cnt[(size_t)l] = (uint32_t)(kHomGroup - l);          // 64, 63, ..., 1
    if (check(cnt, "strictly falling")) return 1;
    for (int l = 0; l < kHomGroup; ++l) cnt[(size_t)l] = (uint32_t)(2 * (kHomGroup - 1 - l));  // ..., 2, 0: the last lane empty
    if (check(cnt, "strictly falling to 0")) return 1;
    for (int l = 0; l < kHomGroup; ++l) cnt[(size_t)l] = (uint32_t)l;                       // (and rising)
    if (check(cnt, "strictly rising")) return 1;
    printf("ok equal and monotone\n");
    for (int at : {0, 17, 63}) {                            // 1500 consecutive rows: 188 chunks, the neighbours 0 or 1
        for (int l = 0; l < kHomGroup; ++l) cnt[(size_t)l] = (uint32_t)(rnd() & 1u);
        cnt[(size_t)at] = 188u;
        if (check(cnt, "one lane of 188")) return 1;
    }
    printf("ok one long lane\n");
    for (int it = 0; it < 2000; ++it) {
        const uint32_t top = it % 4 == 0 ? 2u : it % 4 == 1 ? 9u : it % 4 == 2 ? 40u : 1025u;  // (a sub-slice's list: at most 8192 / 8 = 1024)
        for (int l = 0; l < kHomGroup; ++l) cnt[(size_t)l] = (uint32_t)(rnd() % top);
        if (check(cnt, "random")) return 1;
    }
    printf("ok random\n");
    return 0;
}
