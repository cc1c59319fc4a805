// Stand-alone check of transpose16x16_2bit (csrc/transpose_bits.h), the register transposition of k_transpose_tiles, against its
// definition: plain C++, built by tests/test_xb_spec_cpu.py under AddressSanitizer and UBSan.  No HIP, no GPU.
#include "transpose_bits.h"
#include <cstdint>
#include <cstdio>
#include <cstring>

static unsigned field(const uint32_t x[16], int r, int c) { return (x[r] >> (2 * c)) & 3u; }

// out[c] field r = in[r] field c, by the definition
static void reference(const uint32_t in[16], uint32_t out[16])
{
    for (int c = 0; c < 16; ++c) {
        out[c] = 0;
        for (int r = 0; r < 16; ++r) out[c] |= (uint32_t)field(in, r, c) << (2 * r);
    }
}

static bool same(const uint32_t a[16], const uint32_t b[16]) { return std::memcmp(a, b, 16 * sizeof(uint32_t)) == 0; }

static bool check(const uint32_t in[16], const char *what)
{
    uint32_t want[16], got[16], back[16];
    reference(in, want);
    std::memcpy(got, in, sizeof(got));
    mih::transpose16x16_2bit(got);
    if (!same(got, want)) { std::printf("FAIL %s: not the transpose\n", what); return false; }
    std::memcpy(back, got, sizeof(back));
    mih::transpose16x16_2bit(back);
    if (!same(back, in)) { std::printf("FAIL %s: twice is not the identity\n", what); return false; }
    return true;
}

int main()
{
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t)(state >> 16); };
    uint32_t x[16];
    for (int trial = 0; trial < 20000; ++trial) {
        for (int r = 0; r < 16; ++r) x[r] = next();
        if (!check(x, "random")) return 1;
    }
    std::printf("ok random fields\n");
    for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c)
            for (unsigned v = 1; v < 4; ++v) {
                std::memset(x, 0, sizeof(x));
                x[r] = v << (2 * c);
                if (!check(x, "single")) return 1;
                uint32_t got[16];
                std::memcpy(got, x, sizeof(got));
                mih::transpose16x16_2bit(got);
                for (int k = 0; k < 16; ++k)
                    if (got[k] != (k == c ? v << (2 * r) : 0u)) { std::printf("FAIL single (%d, %d)\n", r, c); return 1; }
            }
    std::printf("ok single fields at 256 positions\n");
    for (int r = 0; r < 16; ++r) x[r] = 0xFFFFFFFFu;
    if (!check(x, "all ones")) return 1;
    uint32_t ones[16];
    std::memcpy(ones, x, sizeof(ones));
    mih::transpose16x16_2bit(ones);
    for (int r = 0; r < 16; ++r) if (ones[r] != 0xFFFFFFFFu) { std::printf("FAIL all ones\n"); return 1; }
    std::memset(x, 0, sizeof(x));
    if (!check(x, "all zeros")) return 1;
    std::printf("ok all ones\n");
    std::printf("ok twice is the identity\n");
    return 0;
}
