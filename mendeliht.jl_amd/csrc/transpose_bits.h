// transpose_bits.h -- the 16 x 16 transposition of 2-bit fields behind k_transpose_tiles (transpose.hip).  Plain C++ that a host
// compiler takes too: tests/transpose_bits_harness.cpp checks it against the definition under the sanitizers.
#pragma once
#include <cstdint>
#if defined(__HIPCC__)
#define MIH_TB_HD __host__ __device__ __forceinline__
#else
#define MIH_TB_HD inline
#endif

namespace mih {

// One butterfly stage: in every pair of rows (r, r + J) with r & J == 0 the fields c & J != 0 of row r change places with the
// fields c & J == 0 of row r + J (MASK: both bits of every field with c & J == 0) -- a shift, two exclusive ors and a mask.
template <int J, uint32_t MASK>
MIH_TB_HD void transpose_stage_2bit(uint32_t x[16])
{
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 16; ++r) {
        if (r & J) continue;
        const uint32_t t = ((x[r] >> (2 * J)) ^ x[r + J]) & MASK;
        x[r + J] ^= t;
        x[r] ^= t << (2 * J);
    }
}

// x[r] holds field (r, c) at bits 2 c .. 2 c + 1, r, c = 0 .. 15; afterwards x[c] holds it at bits 2 r .. 2 r + 1.
MIH_TB_HD void transpose16x16_2bit(uint32_t x[16])
{
    transpose_stage_2bit<8, 0x0000FFFFu>(x);
    transpose_stage_2bit<4, 0x00FF00FFu>(x);
    transpose_stage_2bit<2, 0x0F0F0F0Fu>(x);
    transpose_stage_2bit<1, 0x33333333u>(x);
}

}  // namespace mih
