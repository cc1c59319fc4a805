// xtv_kernels.h -- the 2-bit MFMA device code of xtv.hip (included there only, inside namespace mih)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---- the matrix-pipe kernel -------------------------------------------------------------------
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// dosage tiles are read exactly once per pass: stream them past the caches (nt), so the digit
// planes every wave re-reads stay resident in L2
__device__ __forceinline__ uint4 ld_stream(const uint4 *p)
{
    u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// the same dosage tile against an FP6 (e2m3) B operand: 32 digits x 6 bits = 6 dwords per lane (blgp = 2)
__device__ __forceinline__ f32x16 mfma_fp6(uint32_t u0, uint32_t u1, const uint4 &b, const uint2 &b2, f32x16 acc)
{
    const uint32_t M = 0x33333333u;
    i32x8 a = {(int)(u0 & M), (int)((u0 >> 2) & M), (int)(u1 & M), (int)((u1 >> 2) & M), 0, 0, 0, 0};
    i32x8 bb = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, (int)b2.x, (int)b2.y, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bb, acc, 4, 2, 0, 0, 0, 0);
}

__device__ __forceinline__ f32x16 mfma_fp4(uint32_t u0, uint32_t u1, const uint4 &b, f32x16 acc)
{
    const uint32_t M = 0x33333333u;
    i32x8 a = {(int)(u0 & M), (int)((u0 >> 2) & M), (int)(u1 & M), (int)((u1 >> 2) & M), 0, 0, 0, 0};
    i32x8 bb = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    // cbsz = blgp = 4: A and B are FP4 (e2m1).  Literal zero scale operands make the compiler select the UNSCALED
    // v_mfma_f32_32x32x64_f8f6f4 (no v_mfma_ld_scale_b32 in front of every MFMA); tools/mfma_probe.hip checks that
    // form against exact integer data
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bb, acc, 4, 4, 0, 0, 0, 0);
}

// D layout: column n = lane & 31, row (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5) (SNP).  Column n holds digit
// n % slots of residual per_op*v + n / slots of B operand v.
// acc = (1/unit) sum_i g_i d_i exactly (unit 4 for FP4 digits d/2, 16 for FP6 digits d/8); recombine the digits:
// sum_t base^t * (unit * acc_t), then * 2^-e.
template <int CT, int NR>
__device__ __forceinline__ void xtv_epilogue(const f32x16 (&acc)[CT][NR], int lane, int64_t cg0, int64_t ncg, int split,
                                             int splits, DigitMode dm, const double *__restrict__ scal,
                                             double *__restrict__ partial)
{
    const int slots = dm.slots, col = lane & 31;
    const int sub = col / slots, dgt = col - sub * slots;
    const bool live = sub < dm.per_op;                   // columns past per_op * slots carry nothing
    double wgt = 0.0;
    if (live && dgt < dm.ndig) {
        unsigned long long w = dm.base == 49 ? 16 : 4;   // unit * base^dgt < 2^58: exact in 64 bits, one rounding to f64
        for (int t = 0; t < dgt; ++t) w *= (unsigned)dm.base;
        wgt = (double)w;
    }
    const bool tree = (slots & (slots - 1)) == 0;
    const int src0 = (lane & 32) + sub * slots;
    #pragma unroll
    for (int v = 0; v < NR; ++v) {
        const int rhs = v * dm.per_op + (live ? sub : 0);
        const double inv = scal[4 * rhs + 1];
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
            #pragma unroll
            for (int g = 0; g < 16; ++g) {
                double x = (double)acc[c][v][g] * wgt;
                if (tree) {                                                          // fixed tree within each group of
                    if (slots > 16) x += __shfl_xor(x, 16, 64);                      // `slots` lanes
                    if (slots > 8) x += __shfl_xor(x, 8, 64);
                    #pragma unroll
                    for (int off = 4; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
                } else {                                                             // 10 columns: digit 0 upward
                    double sum = 0.0;
                    #pragma unroll
                    for (int t = 0; t < 10; ++t) sum += __shfl(x, src0 + t, 64);
                    x = sum;
                }
                int row = (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5);
                if (dgt == 0 && live && cg0 + c < ncg)
                    partial[((int64_t)rhs * splits + split) * (ncg * 32) + (cg0 + c) * 32 + row] = x * inv;
            }
        }
    }
}

// The work item of a wave: workgroup blockIdx.x takes row slice blockIdx.x % splits -- the 128-row blocks [b0, b1) -- and its wave
// `wave` the CT column groups from cg0.  The ring kernels walk nb blocks from bb0 and mask the dosages with amask:
// (an empty trailing slice -- nbp not a multiple of the slice count -- runs one clamped, masked-out step so that
// the accumulators never live across a branch: that would push all of them through scratch)
struct RowSlice { int split; int64_t cg0, b0, b1, bb0; int nb, amask; };
template <int WAVES, int CT>
__device__ __forceinline__ RowSlice row_slice(int splits, int64_t nbp, int wave)
{
    RowSlice r;
    r.split = blockIdx.x % splits;
    const int64_t grp = blockIdx.x / splits;
    r.cg0 = (grp * WAVES + wave) * CT;
    const int64_t bps = (nbp + splits - 1) / splits;
    r.b0 = r.split * bps;
    r.b1 = (r.b0 + bps < nbp) ? r.b0 + bps : nbp;
    const bool empty = r.b0 >= r.b1;
    r.bb0 = empty ? nbp - 1 : r.b0;
    r.nb = empty ? 1 : (int)(r.b1 - r.b0);
    r.amask = empty ? 0 : -1;
    return r;
}

// NR (2 or 4) B operands per pass with the digit planes shared through LDS.  A workgroup of WAVES
// waves x CT column groups stages the 8 KB of digit planes of each 128-row block once (instead of once
// per wave: L2 traffic for the digits drops WAVES-fold, which is what keeps the pass off the L2
// roofline) and every wave feeds its dosage tiles to NR x 2 MFMAs per tile.  A barrier step covers RB
// blocks; the digits of step t+1 are loaded during step t-1 and stored to the idle LDS buffer at the
// top of step t, the dosage tiles of step t+1 are loaded at the top of step t, so no load is waited
// for in the step that issued it.  Measured (tools/sweep_multi.py, tools/probe_power.py,
// profiles/r01_power_clock_smi.log): every workgroup shape lands on 29.5 ms because the pass is
// POWER-bound, not issue- or latency-bound -- the package sits at its power cap and the shader clock
// drops to ~1870-1935 MHz for the 4-operand pass; all-zero digit planes run 17 % faster.
// MODE 1 / 2 (no MFMAs / no dosage loads) exist only for those timing probes.
// FP6: the B operands are FP6 digit planes, 24 B per lane: 16 B in `dig` and 8 B in `dig2`, staged side by side.
template <int NR, int CT, int RB, int MODE = 0, int WAVES = 8, bool FP6 = false>   // MODE 1: no MFMAs, 2: no dosage loads (timing probes only)
__global__ void __launch_bounds__(WAVES * 64, 2)
k_xtv_mfma_lds(const uint4 *__restrict__ X, int64_t nbp, int64_t ncg, const uint4 *__restrict__ dig, const uint2 *__restrict__ dig2,
               int64_t dig_stride, int splits, DigitMode dm, const double *__restrict__ scal,
               double *__restrict__ partial /* [NR*per_op][splits][ncg*32] */)
{
    constexpr int NT = WAVES * 64;
    constexpr int BLK = NR * 2 * 64;                 // uint4 slots of one 128-row block: (operand v, 64-row half e, lane)
    constexpr int S = RB * BLK;                      // slots staged per barrier step
    constexpr int PER = (S + NT - 1) / NT;           // slots per thread (the last one may be idle)
    __shared__ uint4 btile[2][S];
    __shared__ uint2 btile2[FP6 ? 2 : 1][FP6 ? S : 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RowSlice sl = row_slice<WAVES, CT>(splits, nbp, wave);
    const int split = sl.split;
    const int64_t cg0 = sl.cg0, b0 = sl.b0, b1 = sl.b1;

    f32x16 acc[CT][NR];
    #pragma unroll
    for (int c = 0; c < CT; ++c)
        #pragma unroll
        for (int v = 0; v < NR; ++v)
            #pragma unroll
            for (int g = 0; g < 16; ++g) acc[c][v][g] = 0.f;

    if (b0 < b1) {
        const int64_t last = b1 - 1;
        const uint4 *ap[CT];
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
            int64_t cg = cg0 + c < ncg ? cg0 + c : ncg - 1;      // idle waves redo the last group
            ap[c] = X + (cg * nbp) * 64 + lane;
        }
        // staged slot f = threadIdx.x + u*NT: block f / BLK of the step, operand (f % BLK) >> 7, half ((f % BLK) >> 6) & 1
        const uint4 *bsrc[PER]; const uint2 *bsrc2[PER]; int bq_[PER]; bool bon[PER];
        #pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int fs = threadIdx.x + u * NT;
            bon[u] = fs < S;
            const int fq = bon[u] ? fs : 0, wi = fq % BLK;
            bq_[u] = fq / BLK;
            const int64_t off = (int64_t)(wi >> 7) * dig_stride + ((wi >> 6) & 1) * 64 + (wi & 63);
            bsrc[u] = dig + off;
            bsrc2[u] = dig2 + off;
        }
        uint4 acur[RB][CT], anext[RB][CT];
        u32x4 bstage[PER];          // native vector type: stays in registers across the loop edge
        u32x2 bstage2[PER];
        #pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int64_t bq = (b0 + q < last) ? b0 + q : last;
            #pragma unroll
            for (int c = 0; c < CT; ++c) acur[q][c] = ld_stream(ap[c] + bq * 64);
        }
        #pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int64_t bq = (b0 + bq_[u] < last) ? b0 + bq_[u] : last;
            const int64_t b2 = (b0 + RB + bq_[u] < last) ? b0 + RB + bq_[u] : last;
            if (bon[u]) btile[0][threadIdx.x + u * NT] = bsrc[u][(2 * bq) * 64];
            bstage[u] = *reinterpret_cast<const u32x4 *>(bsrc[u] + (2 * b2) * 64);
            if (FP6) {
                if (bon[u]) btile2[0][threadIdx.x + u * NT] = bsrc2[u][(2 * bq) * 64];
                bstage2[u] = *reinterpret_cast<const u32x2 *>(bsrc2[u] + (2 * b2) * 64);
            }
        }
        __syncthreads();
        int buf = 0;
        // bstage is carried across the loop edge: the digits of step t+1 are loaded during step t-1
        // and stored to the idle LDS buffer at the top of step t, so neither that load nor the dosage
        // prefetch is waited for in the step that issued it.
        for (int64_t bp = b0; bp < b1; bp += RB) {
            #pragma unroll
            for (int u = 0; u < PER; ++u)
                if (bon[u]) {
                    *reinterpret_cast<u32x4 *>(&btile[buf ^ 1][threadIdx.x + u * NT]) = bstage[u];
                    if (FP6) *reinterpret_cast<u32x2 *>(&btile2[buf ^ 1][threadIdx.x + u * NT]) = bstage2[u];
                }
            #pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int64_t bn = (bp + RB + q < last) ? bp + RB + q : last;
                #pragma unroll
                for (int c = 0; c < CT; ++c) { if (MODE != 2) anext[q][c] = ld_stream(ap[c] + bn * 64); else anext[q][c] = acur[q][c]; }
            }
            #pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int64_t b2 = (bp + 2 * RB + bq_[u] < last) ? bp + 2 * RB + bq_[u] : last;
                bstage[u] = *reinterpret_cast<const u32x4 *>(bsrc[u] + (2 * b2) * 64);
                if (FP6) bstage2[u] = *reinterpret_cast<const u32x2 *>(bsrc2[u] + (2 * b2) * 64);
            }
            __builtin_amdgcn_sched_barrier(0);      // keep the prefetch loads ahead of the MFMA section
            // (block q, operand v) items in sequence; the digit fragments of item i+1 are read from LDS
            // before the MFMAs of item i are issued so the LDS latency hides behind the matrix pipe
            uint4 bfr[2][2];
            uint2 bfr2[2][2];
            bfr[0][0] = btile[buf][lane];
            bfr[0][1] = btile[buf][64 + lane];
            if (FP6) { bfr2[0][0] = btile2[buf][lane]; bfr2[0][1] = btile2[buf][64 + lane]; }
            #pragma unroll
            for (int i = 0; i < RB * NR; ++i) {
                const int q = i / NR, v = i % NR;
                if (i + 1 < RB * NR) {
                    const int q1 = (i + 1) / NR, v1 = (i + 1) % NR;
                    bfr[(i + 1) & 1][0] = btile[buf][q1 * BLK + (v1 * 2 + 0) * 64 + lane];
                    bfr[(i + 1) & 1][1] = btile[buf][q1 * BLK + (v1 * 2 + 1) * 64 + lane];
                    if (FP6) {
                        bfr2[(i + 1) & 1][0] = btile2[buf][q1 * BLK + (v1 * 2 + 0) * 64 + lane];
                        bfr2[(i + 1) & 1][1] = btile2[buf][q1 * BLK + (v1 * 2 + 1) * 64 + lane];
                    }
                }
                const uint32_t keep = (bp + q < b1) ? 0xFFFFFFFFu : 0u;     // blocks past the slice end add zero
                // the CT tiles against one digit fragment in turn: consecutive MFMAs share the B operand and write
                // different accumulators (2 FP6 operands, CT = 4: 23.1 ms against 23.8 ms for tile-by-tile order)
                if (MODE != 1) {
                    #pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        if (FP6) acc[c][v] = mfma_fp6(acur[q][c].x & keep, acur[q][c].y & keep, bfr[i & 1][0], bfr2[i & 1][0], acc[c][v]);
                        else acc[c][v] = mfma_fp4(acur[q][c].x & keep, acur[q][c].y & keep, bfr[i & 1][0], acc[c][v]);
                    }
                    #pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        if (FP6) acc[c][v] = mfma_fp6(acur[q][c].z & keep, acur[q][c].w & keep, bfr[i & 1][1], bfr2[i & 1][1], acc[c][v]);
                        else acc[c][v] = mfma_fp4(acur[q][c].z & keep, acur[q][c].w & keep, bfr[i & 1][1], acc[c][v]);
                    }
                } else {
                    #pragma unroll
                    for (int c = 0; c < CT; ++c)
                        acc[c][v][0] += __uint_as_float((acur[q][c].x ^ acur[q][c].y ^ acur[q][c].z ^ acur[q][c].w) & keep & bfr[i & 1][0].x & bfr[i & 1][1].y);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            buf ^= 1;
            #pragma unroll
            for (int q = 0; q < RB; ++q)
                #pragma unroll
                for (int c = 0; c < CT; ++c) acur[q][c] = anext[q][c];
        }
    }
    if (cg0 >= ncg) return;
    xtv_epilogue<CT, NR>(acc, lane, cg0, ncg, split, splits, dm, scal, partial);
}

// ---- X'R with every operand through an LDS-DMA ring ---------------------------------------------------------------
// The register-staged LDS kernel above keeps ONE 128-row step of dosage tiles in flight per wave (16 KB per CU with its
// one resident workgroup of the fused shapes) and waits for it at the top of the next step.  Here nothing is loaded
// into registers: every wave copies its own CT dosage tiles and its share of the block's digit planes straight into
// LDS (global_load_lds_dwordx4, 1 KB per instruction) D steps ahead of their use, so D x (WAVES*CT + 2..3 NR) KB are
// in flight per CU and the registers hold only accumulators (AGPRs) and fragments.  Waits are counted by hand
// (s_waitcnt vmcnt(N): LDS-DMA completes in issue order); a wave's own dosage tiles need only its own wait, the shared
// digit planes the wait plus the step's one barrier.  Ring of D + 1 stages: the stage refilled in step t is the one
// last read in step t - 1.  Same arithmetic, same row slicing, same summation order as the other kernels: same bits.
// Measured at n = 500k, p = 1M (tools/sweep_dma.py, tools/probe_dma.py, profiles/r02_*): 12 residuals 34.7 ms against
// 40.0 ms register-staged; D = 2, 3, 4 and the 4 x 4 / 8 x 2 wave shapes all land within 1 % of each other because the
// pass is bound by the package power cap, not by latency or issue (1354 W, shader clock 1.71 GHz; the same MFMAs alone,
// operands in registers, take 20.0 ms at 1.63 GHz: tools/mfma_rate.hip).
typedef int i32x4v __attribute__((ext_vector_type(4)));
typedef int i32x2v __attribute__((ext_vector_type(2)));
// One ds_read_b64 (64 banks, 2 LDS cycles per wave) that the compiler may not pair with a neighbour: two plain 8-byte loads at
// constant distance become ds_read2_b64 / ds_read2st64_b64, which bank modulo 32 in 16-lane groups -- 8 cycles per instruction,
// and on the A-fragment address map (16-byte lane stride) 2-way conflicts on top: 16 LDS cycles per dosage tile instead of 4
// (round 2's SQ_LDS_BANK_CONFLICT = 8 cycles per tile in every k_xtv_dma16 shape).  Volatile on an LDS-qualified pointer keeps
// the loads apart and in the LDS address space.
typedef __attribute__((address_space(3))) const volatile i32x2v *lds_b64_ptr;
__device__ __forceinline__ i32x2v lds_read_b64(const char *p) { return *(lds_b64_ptr)(p); }

// lane i's 16 B at sbase + voff land at LDS byte address lds_dst + 16 i.  M0 is compiler-reserved: saved and restored.
template <bool NT>
__device__ __forceinline__ void glds16(uint32_t lds_dst, uint32_t voff, const void *sbase)
{
    uint32_t keep;
    if (NT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3 nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "s"(lds_dst), "v"(voff), "s"(sbase) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "s"(lds_dst), "v"(voff), "s"(sbase) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_vm_barrier()
{
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(N) : "memory");
}

template <bool FP6>
__device__ __forceinline__ f32x16 mfma4x(i32x4v a, const i32x8 &b, f32x16 acc)
{
    i32x8 aa = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
    if (FP6) return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(aa, b, acc, 4, 2, 0, 0, 0, 0);
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(aa, b, acc, 4, 4, 0, 0, 0, 0);
}
// timing probe: consumes the fragments with one VALU operation instead of an MFMA
__device__ __forceinline__ f32x16 fake4x(i32x4v a, const i32x8 &b, f32x16 acc)
{
    acc[0] += __int_as_float((a[0] ^ a[1] ^ a[2] ^ a[3]) & b[0] & b[3]);
    return acc;
}

// The feed of the ring, as one wave sees it: its own CT dosage tiles and its share of the step's NP = NR x PPO digit pieces of
// 1 KB (PPO = 2: the two `dig` halves of an FP4 operand; 3: + the `dig2` piece of an FP6 one).  A stage holds the workgroup's dosage
// tiles (wave w: CT KB at w * CT KB) and behind them the operands' pieces; issue() queues L copies, so a wait for "all but the
// newest k steps" is vmcnt(k * L).
template <int CT, int NR, int WAVES, int PPO>
struct RingFeed {
    static constexpr bool FP6 = PPO == 3;
    static constexpr int DOS = WAVES * CT * 1024;          // dosage bytes of a stage
    static constexpr int OPB = PPO * 1024;                 // digit bytes of an operand and step
    static constexpr int STAGE = DOS + NR * OPB;
    static constexpr int NP = NR * PPO;                    // digit pieces per step
    static constexpr int PW = (NP + WAVES - 1) / WAVES;    // pieces per wave (surplus slots repeat the last piece)
    static constexpr int L = CT + PW;                      // LDS-DMA instructions per wave and step
    const char *xs[CT];
    const char *dsrc[PW]; int dstep[PW]; int doff[PW];      // piece u: source, its bytes per step, place in the stage
    int lane, nb;
    uint32_t voff, lds0, mydos;
    const char *ldsb;

    __device__ __forceinline__ RingFeed(const uint4 *X, int64_t nbp, int64_t ncg, const uint4 *dig, const uint2 *dig2, int64_t dig_stride,
                                        const RowSlice &sl, int wave, int lane_, const uint4 *lds)
    {
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int64_t cg = sl.cg0 + c < ncg ? sl.cg0 + c : ncg - 1;        // idle waves redo the last group
            xs[c] = reinterpret_cast<const char *>(X) + (cg * nbp + sl.bb0) * 1024;
        }
        #pragma unroll
        for (int u = 0; u < PW; ++u) {
            const int jj = wave + u * WAVES, j = jj < NP ? jj : NP - 1;
            const int op = j / PPO, part = j - PPO * op;
            if (part < 2) {
                dsrc[u] = reinterpret_cast<const char *>(dig) + (op * dig_stride + (2 * sl.bb0 + part) * 64) * 16;
                dstep[u] = 2048; doff[u] = DOS + op * OPB + part * 1024;
            } else {
                dsrc[u] = reinterpret_cast<const char *>(dig2) + (op * dig_stride + 2 * sl.bb0 * 64) * 8;
                dstep[u] = 1024; doff[u] = DOS + op * OPB + 2048;
            }
        }
        lane = lane_; nb = sl.nb;
        voff = lane * 16;
        lds0 = (uint32_t)(uintptr_t)lds;           // low 32 bits of a generic LDS address = the byte offset M0 takes
        mydos = wave * CT * 1024;
        ldsb = reinterpret_cast<const char *>(lds);
    }
    // the copies of step ts into stage st
    __device__ __forceinline__ void issue(int ts, int st) const
    {
        const int tb = ts < nb ? ts : nb - 1;                        // past the slice end: copy the last block again
        const uint32_t base = lds0 + st * STAGE;
        #pragma unroll
        for (int c = 0; c < CT; ++c) glds16<true>(base + mydos + c * 1024, voff, xs[c] + (int64_t)tb * 1024);
        #pragma unroll
        for (int u = 0; u < PW; ++u) glds16<false>(base + doff[u], voff, dsrc[u] + (int64_t)tb * dstep[u]);
    }
    // B fragment `item` = (operand item >> 1, half item & 1) of stage st.  PLAIN: round 2's plain 8-byte load of the FP6 part
    template <bool PLAIN = false>
    __device__ __forceinline__ void read_b(int st, int item, i32x8 &b) const
    {
        const int v = item >> 1, e = item & 1;
        const char *q = ldsb + st * STAGE + DOS + v * OPB;
        const i32x4v lo = *reinterpret_cast<const i32x4v *>(q + e * 1024 + lane * 16);
        if (FP6) {
            const i32x2v hi = PLAIN ? *reinterpret_cast<const i32x2v *>(q + 2048 + e * 512 + lane * 8) : lds_read_b64(q + 2048 + e * 512 + lane * 8);
            b = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], 0, 0};
        } else b = i32x8{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
    }
};

// One step of either ring kernel: the NI fragment items of step T with the A fragments of buffer P; fills buffer P ^ 1 for step T + 1.
// Item i sits in B[(i + PB) & 1] (an odd item count: the B double buffer alternates from step to step).  The last item's MFMAs are
// issued after the barrier, behind the first fragment read of the next step.  ISSUE / READB(i): timing probes leave copies / reads out.
#define MIH_RING_STEP(P, T, ISSUE, READB, ITEM)                                                                    \
        {                                                                                                          \
            const int st_next = st + 1 == S ? 0 : st + 1, st_ld = st == 0 ? S - 1 : st - 1;                        \
            constexpr int PB = (P) * (NI & 1);                                                                     \
            if (ISSUE) feed.issue((T) + D, st_ld);                                                                 \
            _Pragma("unroll")                                                                                      \
            for (int i = 0; i < NI - 1; ++i) {                                                                     \
                if (READB(i + 1)) read_b(st, i + 1, B[(i + 1 + PB) & 1]);                                          \
                ITEM(P, i, B[(i + PB) & 1])                                                                        \
                if (i == (NI > 2 ? NI / 2 - 1 : 0)) { wait_vm<D * L - CT>(); read_dos(st_next, araw); }            \
                if (i == (NI > 2 ? NI / 2 : 0)) expand(araw, A[(P) ^ 1]);                                          \
            }                                                                                                      \
            if (NI == 1) { wait_vm<D * L - CT>(); read_dos(st_next, araw); expand(araw, A[(P) ^ 1]); }             \
            wait_vm_barrier<(D - 1) * L>();                                                                        \
            read_b(st_next, 0, B[(NI + PB) & 1]);      /* = item 0 of the next step: ((P ^ 1) * ODD) & 1 */         \
            __builtin_amdgcn_sched_barrier(0);                                                                     \
            ITEM(P, NI - 1, B[(NI - 1 + PB) & 1])                                                                  \
            st = st_next;                                                                                          \
        }

// Epilogues of the ring kernels.  The 32 x 32 accumulator tile of a (column group, operand) goes through a 4.5 KB LDS
// buffer of the wave as f32 [digit column][SNP row] (rows padded to 36 floats: conflict-free 16-B stores); lane
// (row, residual) then adds up its residual's digit columns in exactly the order of xtv_epilogue -- digit 0 upward for
// 10 columns, the xor tree for 8 / 16 / 32 -- so the bits are those of every other kernel, with `slots` LDS reads per
// output instead of 10 f64 shuffles per accumulator register.
typedef float f32x4v __attribute__((ext_vector_type(4)));
constexpr int kTileRS = 36;          // floats per digit column of the wave's tile buffer
// wgt[t] = unit * base^t < 2^58: exact in 64 bits, one rounding to f64
template <int SLOTS>
__device__ __forceinline__ void digit_weights(double (&wgt)[SLOTS], unsigned long long unit, unsigned base, int ndig)
{
    unsigned long long w = unit;
    #pragma unroll
    for (int t = 0; t < SLOTS; ++t) { wgt[t] = t < ndig ? (double)w : 0.0; w *= base; }
}
// sum_t src[t] wgt[t] over the SLOTS digit columns of one (residual, SNP row)
template <int SLOTS>
__device__ __forceinline__ double digit_sum(const float *src, const double (&wgt)[SLOTS])
{
#pragma clang fp contract(off)      // products and sums round separately, as in xtv_epilogue (there a shuffle sits between them)
    double x[SLOTS];
    #pragma unroll
    for (int t = 0; t < SLOTS; ++t) x[t] = (double)src[t * kTileRS] * wgt[t];
    if ((SLOTS & (SLOTS - 1)) == 0) {                // the xor tree of xtv_epilogue, lane 0's cone
        #pragma unroll
        for (int off = SLOTS / 2; off > 0; off >>= 1)
            #pragma unroll
            for (int t = 0; t < off; ++t) x[t] = x[t] + x[t + off];
        return x[0];
    }
    double sum = 0.0;
    #pragma unroll
    for (int t = 0; t < SLOTS; ++t) sum += x[t];
    return sum;
}
// the tile of operand v and column group cg is in `buf`: output o = (SNP row o & 31, residual o >> 5 of the operand's first nsub).
// (The callers' loop over a lane's two outputs stays in the callers: inside this function it cost k_xtv_dma four VGPRs.)
template <int SLOTS>
__device__ __forceinline__ void xtv_tile_sum(const float *buf, int o, int v, int nsub, int per_op, const double (&wgt)[SLOTS], int64_t cg,
                                             int64_t ncg, int split, int splits, const double *__restrict__ scal, double *__restrict__ partial)
{
    const int row = o & 31, sub = o >> 5;
    if (sub < nsub) {
        const double sum = digit_sum<SLOTS>(buf + sub * SLOTS * kTileRS + row, wgt);
        const int rhs = v * per_op + sub;
        if (cg < ncg)
            partial[((int64_t)rhs * splits + split) * (ncg * 32) + cg * 32 + row] = sum * scal[4 * rhs + 1];
    }
}

template <int CT, int NR, int SLOTS>
__device__ __forceinline__ void xtv_epilogue_lds_s(const f32x16 (&acc)[CT][NR], float *buf, int lane, int64_t cg0, int64_t ncg,
                                                   int split, int splits, DigitMode dm, const double *__restrict__ scal,
                                                   double *__restrict__ partial)
{
    const int col = lane & 31, hi = lane >> 5;
    double wgt[SLOTS];
    digit_weights<SLOTS>(wgt, dm.base == 49 ? 16 : 4, (unsigned)dm.base, dm.ndig);
    #pragma unroll
    for (int v = 0; v < NR; ++v) {
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
            __builtin_amdgcn_wave_barrier();
            #pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<f32x4v *>(buf + col * kTileRS + 8 * q + 4 * hi) =
                    f32x4v{acc[c][v][4 * q], acc[c][v][4 * q + 1], acc[c][v][4 * q + 2], acc[c][v][4 * q + 3]};
            __builtin_amdgcn_wave_barrier();
            #pragma unroll
            for (int k = 0; k < 2; ++k) xtv_tile_sum<SLOTS>(buf, lane + 64 * k, v, dm.per_op, dm.per_op, wgt, cg0 + c, ncg, split, splits, scal, partial);
        }
    }
}
template <int CT, int NR>
__device__ __forceinline__ void xtv_epilogue_lds(const f32x16 (&acc)[CT][NR], float *buf, int lane, int64_t cg0, int64_t ncg,
                                                 int split, int splits, DigitMode dm, const double *__restrict__ scal,
                                                 double *__restrict__ partial)
{
    if (dm.slots == 10) xtv_epilogue_lds_s<CT, NR, 10>(acc, buf, lane, cg0, ncg, split, splits, dm, scal, partial);
    else if (dm.slots == 8) xtv_epilogue_lds_s<CT, NR, 8>(acc, buf, lane, cg0, ncg, split, splits, dm, scal, partial);
    else if (dm.slots == 16) xtv_epilogue_lds_s<CT, NR, 16>(acc, buf, lane, cg0, ncg, split, splits, dm, scal, partial);
    else xtv_epilogue_lds_s<CT, NR, 32>(acc, buf, lane, cg0, ncg, split, splits, dm, scal, partial);
}

// Epilogue of the passes over the score image (score_image.hip; one residual, 28 base-4 digit columns in 32 slots).  The wave's
// column groups g0 .. g0 + ACT - 1 of its region (ng groups) sit at image positions; dm.img_col maps a position to its column of
// the matrix and the dot product goes where the 2-bit pass puts it.  ONEBIT: the tile was multiplied as the plane [g >= 1], so a
// dosage-2 entry is short by (1/2)(d_t / 2): 0.25 * (sum of d_t over the column's dosage-2 rows of the slice, k_xtv_hom) is added to
// digit column t first.  The total is the 2-bit pass's S_t, below 2^24 quarter units: the f32 addition is exact, and the
// recombination sees the 2-bit pass's numbers in its order (xtv_epilogue_lds_s<.., 32>).
template <int ACT, bool ONEBIT>
__device__ __forceinline__ void xtv_epilogue_img(f32x16 (&acc)[ACT][1], float *buf, int lane, int64_t g0, int64_t ng, int split,
                                                 DigitMode dm, const double *__restrict__ scal, double *__restrict__ partial)
{
    const int col = lane & 31, hi = lane >> 5;
    double wgt[32];
    digit_weights<32>(wgt, 4, 4u, dm.ndig);
    #pragma unroll
    for (int c = 0; c < ACT; ++c) {
        const int64_t g = g0 + c;
        if (ONEBIT && g < ng) {
            const float *e = dm.img_hom + ((int64_t)split * dm.img_p1 + g * 32) * 32 + col;
            #pragma unroll
            for (int q = 0; q < 16; ++q) acc[c][0][q] += 0.25f * e[((q & 3) + 8 * (q >> 2) + 4 * hi) * 32];
        }
        __builtin_amdgcn_wave_barrier();
        #pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<f32x4v *>(buf + col * kTileRS + 8 * q + 4 * hi) =
                f32x4v{acc[c][0][4 * q], acc[c][0][4 * q + 1], acc[c][0][4 * q + 2], acc[c][0][4 * q + 3]};
        __builtin_amdgcn_wave_barrier();
        if (lane < 32 && g < ng) {
            const int64_t j = dm.img_col[g * 32 + lane];
            if (j >= 0) partial[(int64_t)split * dm.img_pstride + j] = digit_sum<32>(buf + lane, wgt) * scal[1];
        }
    }
}

// IMG (the score image, score_image.hip; one FP4 operand): 1 -- X is the image's class-2 region, the matrix's own tile format,
// and only the epilogue differs (the column map); 2 -- X is the class-1 region: a 1 KB tile holds TWO column groups at one bit per
// genotype, a lane's dwords 0, 1 the row halves of group A and 2, 3 those of group B, so a wave owns 2 CT groups (ACT) and runs four
// MFMAs per tile and step.  The feed, the wait counts and the barrier are the same.
template <int NR, int CT, int WAVES, int D, bool FP6, int MODE = 0, int IMG = 0>      // MODE 1: no MFMAs, 2: no copies after the prologue (timing probes only)
__global__ void __launch_bounds__(WAVES * 64, 1)
k_xtv_dma(const uint4 *__restrict__ X, int64_t nbp, int64_t ncg, const uint4 *__restrict__ dig, const uint2 *__restrict__ dig2,
          int64_t dig_stride, int splits, DigitMode dm, const double *__restrict__ scal,
          double *__restrict__ partial /* [NR*per_op][splits][ncg*32] */)
{
    typedef RingFeed<CT, NR, WAVES, FP6 ? 3 : 2> Feed;
    constexpr int S = D + 1;                        // ring stages
    constexpr int STAGE = Feed::STAGE, L = Feed::L;
    constexpr int NI = 2 * NR;                      // (operand, 64-row half) items of a step
    static_assert(S * STAGE <= 160 * 1024, "LDS ring too large");
    static_assert(D * L <= 63, "vmcnt range");
    static_assert(S * STAGE >= WAVES * 32 * 36 * 4, "the epilogue buffers overlay the ring");
    static_assert(IMG == 0 || (NR == 1 && !FP6 && MODE == 0), "the score image serves the single-residual FP4 pass");
    constexpr int ACT = IMG == 2 ? 2 * CT : CT;     // column groups (accumulator tiles) of a wave
    if (dm.gate && *dm.gate != dm.gate_val) return;      // (uniform: one scalar load and a branch in front of everything)
    __shared__ uint4 lds[S * STAGE / 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RowSlice sl = row_slice<WAVES, CT>(splits, nbp, wave);

    f32x16 acc[ACT][NR];
    #pragma unroll
    for (int c = 0; c < ACT; ++c)
        #pragma unroll
        for (int v = 0; v < NR; ++v)
            #pragma unroll
            for (int g = 0; g < 16; ++g) acc[c][v][g] = 0.f;

    {
        const Feed feed(X, nbp, ncg, dig, dig2, dig_stride, sl, wave, lane, lds);
        const int nb = sl.nb;
        auto read_b = [&](int st, int item, i32x8 &b) { feed.read_b(st, item, b); };
        auto read_dos = [&](int st, i32x4v (&raw)[CT]) {
            #pragma unroll
            for (int c = 0; c < CT; ++c) raw[c] = *reinterpret_cast<const i32x4v *>(feed.ldsb + st * STAGE + feed.mydos + c * 1024 + lane * 16);
        };
        auto expand = [&](const i32x4v (&raw)[CT], i32x4v (&a)[ACT][2]) {
            if constexpr (IMG == 2) {       // dword 2 g + e: group g, row half e; element 8k + q at bit 4q + k (nibble 0001 = FP4 0.5)
                const int M = 0x11111111 & sl.amask;
                #pragma unroll
                for (int c = 0; c < CT; ++c)
                    #pragma unroll
                    for (int ge = 0; ge < 4; ++ge) {
                        const unsigned u = raw[c][ge];
                        a[2 * c + (ge >> 1)][ge & 1] = i32x4v{(int)u & M, (int)(u >> 1) & M, (int)(u >> 2) & M, (int)(u >> 3) & M};
                    }
            } else {
                const int M = 0x33333333 & sl.amask;
                #pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const unsigned x = raw[c][0], y = raw[c][1], z = raw[c][2], w = raw[c][3];
                    a[c][0] = i32x4v{(int)x & M, (int)(x >> 2) & M, (int)y & M, (int)(y >> 2) & M};
                    a[c][1] = i32x4v{(int)z & M, (int)(z >> 2) & M, (int)w & M, (int)(w >> 2) & M};
                }
            }
        };

        #pragma unroll
        for (int s = 0; s < D; ++s) feed.issue(s, s);
        i32x4v araw[CT];
        i32x4v A[2][ACT][2];
        i32x8 B[2];
        wait_vm_barrier<(D - 1) * L>();
        read_dos(0, araw);
        read_b(0, 0, B[0]);
        expand(araw, A[0]);
        int st = 0;
        // item (operand v, 64-row half e): the CT tiles' half e against the operand's fragment of that half
#define MIH_MM(a_, b_, c_) (MODE == 1 ? fake4x(a_, b_, c_) : mfma4x<FP6>(a_, b_, c_))
#define MIH_DMA_ITEM(P, I, BB)                                                                                     \
            _Pragma("unroll")                                                                                      \
            for (int c = 0; c < ACT; ++c) acc[c][(I) >> 1] = MIH_MM(A[P][c][(I) & 1], BB, acc[c][(I) >> 1]);
#define MIH_ALL(i_) true
        for (int t = 0; t < nb; t += 2) {
            MIH_RING_STEP(0, t, MODE != 2, MIH_ALL, MIH_DMA_ITEM)
            if (t + 1 < nb) MIH_RING_STEP(1, t + 1, MODE != 2, MIH_ALL, MIH_DMA_ITEM)
        }
#undef MIH_ALL
#undef MIH_DMA_ITEM
#undef MIH_MM
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the look-ahead copies have landed, every wave is done with the ring
    }
    if (sl.cg0 >= ncg) return;
    float *buf = reinterpret_cast<float *>(lds) + wave * (32 * 36);
    if constexpr (IMG == 1) xtv_epilogue_img<ACT, false>(acc, buf, lane, sl.cg0, ncg, sl.split, dm, scal, partial);
    else if constexpr (IMG == 2) xtv_epilogue_img<ACT, true>(acc, buf, lane, 2 * sl.cg0, dm.img_p1 / 32, sl.split, dm, scal, partial);
    else xtv_epilogue_lds<CT, NR>(acc, buf, lane, sl.cg0, ncg, sl.split, splits, dm, scal, partial);
}

// The same pass on v_mfma_f32_16x16x128_f8f6f4.  Under the package power cap the chip holds a higher clock on the
// 16x16x128 form of the instruction (half the accumulator traffic per multiply-add): the same multiply-adds, operands in
// registers, take 16.0 ms against 20.0 ms for 32x32x64 on dosage-like x digit-like data (tools/mfma_rate.hip).  A tile
// (32 SNPs x 128 rows) becomes two A fragments (16 SNPs each, all 128 rows: lane (r, kq) reads the 8 bytes of row group
// (e, h) = (kq & 1, kq >> 1) of SNP r from the LDS image -- the row-group order is free as long as both operands use it),
// an operand's digit planes two B fragments of 16 columns (DigitMode::lay16 layout written by k_digits), and the four
// 16 x 16 products of a (tile, operand) accumulate over the whole 128-row block in one instruction each.
typedef float f32x4a __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4a mfma16(i32x4v a, const i32x8 &b, f32x4a acc)
{
    i32x8 aa = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aa, b, acc, 4, 2, 0, 0, 0, 0);
}

// the wave's tile buffer <- the 16 x 16 accumulators of one (column group, operand); cut: only the first 16 columns exist
__device__ __forceinline__ void xtv_store_tile16(const f32x4a (&acc)[2][2], float *buf, int lane, bool cut)
{
    const int n16 = lane & 15, rg = lane >> 4;
    #pragma unroll
    for (int a = 0; a < 2; ++a)
        #pragma unroll
        for (int b = 0; b < (cut ? 1 : 2); ++b)      // D: column 16 b + lane % 16, SNP rows 16 a + 4 (lane / 16) + (0..3)
            *reinterpret_cast<f32x4v *>(buf + (16 * b + n16) * kTileRS + 16 * a + 4 * rg) = f32x4v{acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]};
}

template <int CT, int NR, int SLOTS, int HALF>
__device__ __forceinline__ void xtv_epilogue16_s(const f32x4a (&acc)[CT][NR][2][2], float *buf, int lane, int64_t cg0, int64_t ncg,
                                                 int split, int splits, DigitMode dm, const double *__restrict__ scal,
                                                 double *__restrict__ partial)
{
    double wgt[SLOTS];
    digit_weights<SLOTS>(wgt, 16, 49u, dm.ndig);
    #pragma unroll
    for (int v = 0; v < NR; ++v) {
        const bool cut = HALF && v == NR - 1;      // the pass's last operand: only the residuals of its first 16 columns exist
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
            __builtin_amdgcn_wave_barrier();
            xtv_store_tile16(acc[c][v], buf, lane, cut);
            __builtin_amdgcn_wave_barrier();
            #pragma unroll
            for (int k = 0; k < 2; ++k) xtv_tile_sum<SLOTS>(buf, lane + 64 * k, v, cut ? 16 / SLOTS : dm.per_op, dm.per_op, wgt, cg0 + c, ncg, split, splits, scal, partial);
        }
    }
}

// Flat packing (DigitMode::flat, ten-digit format): residual j of the pass owns digit columns 10 j .. 10 j + 9 counted across the
// pass's operands, so a residual may begin in operand v and end in operand v + 1.  The operands' 32 x 32 tiles go through the
// wave's LDS buffer one after the other, as above; lane (row, q) takes the q-th residual that touches operand v, adds up ITS
// columns of this tile in digit order -- starting from 0 if the residual begins here, from the running sum it left in
// `carry[row]` in the previous operand otherwise -- and either stores the finished dot product or leaves the running sum for the
// next operand.  Products first, then one addition per digit from digit 0 upward: the operations, and their order, are those
// of xtv_epilogue16_s<.., 10, ..>, so the bits are the same wherever a residual sits.
template <int CT, int NR, int HALF>
__device__ __forceinline__ void xtv_epilogue16_flat(const f32x4a (&acc)[CT][NR][2][2], float *buf, int lane, int64_t cg0, int64_t ncg,
                                                    int split, int splits, DigitMode dm, const double *__restrict__ scal,
                                                    double *__restrict__ partial)
{
#pragma clang fp contract(off)      // products and sums round separately, as in xtv_epilogue
    constexpr int RS = kTileRS, ND = 10;
    const int nres = dm.nres;
    double wgt[ND];
    {
        unsigned long long w = 16;
        #pragma unroll
        for (int t = 0; t < ND; ++t) { wgt[t] = (double)w; w *= 49u; }
    }
    double *carry = reinterpret_cast<double *>(buf + 32 * RS);       // [32 SNP rows], behind the tile
    #pragma unroll
    for (int c = 0; c < CT; ++c) {
        #pragma unroll
        for (int v = 0; v < NR; ++v) {
            const bool cut = HALF && v == NR - 1;      // the pass's last operand: only its first 16 columns exist
            __builtin_amdgcn_wave_barrier();
            xtv_store_tile16(acc[c][v], buf, lane, cut);
            __builtin_amdgcn_wave_barrier();
            const int jlo = (32 * v) / ND, jhi = (32 * v + 31) / ND;       // residuals with a column in [32 v, 32 v + 32)
            #pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int o = lane + 64 * k, row = o & 31, j = jlo + (o >> 5);
                if (j <= jhi && j < nres) {
                    const int c0 = ND * j - 32 * v;                // column of digit 0 in this tile (negative: it began in the previous one)
                    const int tf = c0 < 0 ? -c0 : 0, tl = c0 + ND - 1 > 31 ? 31 - c0 : ND - 1;
                    double sum = tf == 0 ? 0.0 : carry[row];
                    #pragma unroll
                    for (int t = 0; t < ND; ++t)
                        if (t >= tf && t <= tl) {
                            const double x = (double)buf[(c0 + t) * RS + row] * wgt[t];
                            sum += x;
                        }
                    if (tl == ND - 1) {
                        if (cg0 + c < ncg)
                            partial[((int64_t)j * splits + split) * (ncg * 32) + (cg0 + c) * 32 + row] = sum * scal[4 * j + 1];
                    } else carry[row] = sum;           // (read in round k = 0 of the next operand; written here in a later round or after it)
                }
            }
        }
    }
}

// HALF = 1: the second 16-column fragment of the pass's LAST operand holds no residual (1 residual of 10 digits, or 2 of 8,
// in that operand: m = 3 j + 1 residuals in a pass) and its multiply-adds are left out -- 2 NR - 1 fragment items a step.
template <int NR, int CT, int WAVES, int D, int MODE = 0, int HALF = 0>       // MODE 3: timing probe, the odd 16-column fragments are skipped (result is NOT X'R); MODE 4: round 2's plain 8-byte LDS loads, which the compiler pairs into ds_read2_b64 (A/B for the bank-conflict fix; same result)
__global__ void __launch_bounds__(WAVES * 64, 1)
k_xtv_dma16(const uint4 *__restrict__ X, int64_t nbp, int64_t ncg, const uint4 *__restrict__ dig, const uint2 *__restrict__ dig2,
            int64_t dig_stride, int splits, DigitMode dm, const double *__restrict__ scal,
            double *__restrict__ partial /* [NR*per_op][splits][ncg*32] */)
{
    typedef RingFeed<CT, NR, WAVES, 3> Feed;
    constexpr int S = D + 1;
    constexpr int STAGE = Feed::STAGE, L = Feed::L;
    constexpr int NI = 2 * NR - HALF;               // (operand, 16-column half) items of a step
    static_assert(S * STAGE <= 160 * 1024, "LDS ring too large");
    static_assert(D * L <= 63, "vmcnt range");
    static_assert(S * STAGE >= WAVES * (32 * 36 + 64) * 4, "the epilogue buffers overlay the ring");
    static_assert(HALF == 0 || MODE == 0, "probes run on full operands");
    __shared__ uint4 lds[S * STAGE / 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RowSlice sl = row_slice<WAVES, CT>(splits, nbp, wave);

    f32x4a acc[CT][NR][2][2];
    #pragma unroll
    for (int c = 0; c < CT; ++c)
        #pragma unroll
        for (int v = 0; v < NR; ++v)
            #pragma unroll
            for (int q = 0; q < 4; ++q)
                #pragma unroll
                for (int g = 0; g < 4; ++g) acc[c][v][q >> 1][q & 1][g] = 0.f;
    {
        const Feed feed(X, nbp, ncg, dig, dig2, dig_stride, sl, wave, lane, lds);
        const int nb = sl.nb;
        // A fragment of SNP half a: the 8 bytes of row group (e, h) = (kq & 1, kq >> 1) of SNP 16 a + lane % 16
        const int kq = lane >> 4;
        const uint32_t aoff = (32 * (kq >> 1) + (lane & 15)) * 16 + 8 * (kq & 1);

        auto read_b = [&](int st, int item, i32x8 &b) { feed.template read_b<MODE == 4>(st, item, b); };
        auto read_dos = [&](int st, i32x2v (&raw)[CT][2]) {
            #pragma unroll
            for (int c = 0; c < CT; ++c)
                #pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const char *q = feed.ldsb + st * STAGE + feed.mydos + c * 1024 + a * 256 + aoff;
                    raw[c][a] = MODE == 4 ? *reinterpret_cast<const i32x2v *>(q) : lds_read_b64(q);
                }
        };
        auto expand = [&](const i32x2v (&raw)[CT][2], i32x4v (&a)[CT][2]) {
            const int M = 0x33333333 & sl.amask;
            #pragma unroll
            for (int c = 0; c < CT; ++c)
                #pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const unsigned x = raw[c][h][0], y = raw[c][h][1];
                    a[c][h] = i32x4v{(int)x & M, (int)(x >> 2) & M, (int)y & M, (int)(y >> 2) & M};
                }
        };

        #pragma unroll
        for (int s = 0; s < D; ++s) feed.issue(s, s);
        i32x2v araw[CT][2];
        i32x4v A[2][CT][2];
        i32x8 B[2];
        wait_vm_barrier<(D - 1) * L>();
        read_dos(0, araw);
        read_b(0, 0, B[0]);
        expand(araw, A[0]);
        int st = 0;
        // item (operand v, 16-column half b): both SNP halves of the CT tiles against the operand's 16-column fragment
#define MIH_DMA16_ITEM(P, I, BB)                                                                                   \
            _Pragma("unroll")                                                                                      \
            for (int c = 0; c < CT && !(MODE == 3 && ((I) & 1)); ++c) {                                            \
                acc[c][(I) >> 1][0][(I) & 1] = mfma16(A[P][c][0], BB, acc[c][(I) >> 1][0][(I) & 1]);              \
                acc[c][(I) >> 1][1][(I) & 1] = mfma16(A[P][c][1], BB, acc[c][(I) >> 1][1][(I) & 1]);              \
            }
#define MIH_DMA16_READB(i_) (!(MODE == 3 && ((i_) & 1)))
        for (int t = 0; t < nb; t += 2) {
            MIH_RING_STEP(0, t, true, MIH_DMA16_READB, MIH_DMA16_ITEM)
            if (t + 1 < nb) MIH_RING_STEP(1, t + 1, true, MIH_DMA16_READB, MIH_DMA16_ITEM)
        }
#undef MIH_DMA16_READB
#undef MIH_DMA16_ITEM
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (sl.cg0 >= ncg) return;
    float *buf = reinterpret_cast<float *>(lds) + wave * (32 * 36 + 64);      // a 32 x 36 f32 tile + 32 running sums (flat packing)
    if (dm.flat) xtv_epilogue16_flat<CT, NR, HALF>(acc, buf, lane, sl.cg0, ncg, sl.split, splits, dm, scal, partial);
    else if (dm.slots == 10) xtv_epilogue16_s<CT, NR, 10, HALF>(acc, buf, lane, sl.cg0, ncg, sl.split, splits, dm, scal, partial);
    else xtv_epilogue16_s<CT, NR, 8, HALF>(acc, buf, lane, sl.cg0, ncg, sl.split, splits, dm, scal, partial);
}
#undef MIH_RING_STEP

// Combine slices, add the missing-entry correction, centre, scale -- for the `nres` residuals of a pass in one launch: partial,
// scal, r and out advance by one residual's stride each.  A thread keeps its column and walks the residuals (round 4; before,
// one grid row per residual read mu, sinv and the two missing-list bounds once per residual: 64 MB per residual at p = 1M and
// four slices, 40 MB now); the arithmetic of every (residual, column) is unchanged.
// (round 6) pl: the rows k_r_stats / k_res_peel took out of the fixed-point residual (peel.h) -- their terms g_ij r_i are added here in
// f64, ascending rows, behind the slices' sum; a missing genotype is stored as dosage 0 and gets its imputed value below, like the rest
__device__ __forceinline__ double xtv_finalize_col(int64_t j, const double *__restrict__ pu, int splits, int64_t pstride, double sum_r,
                                                   const double *__restrict__ ru, double m, double si, int64_t a, int64_t b,
                                                   const int32_t *__restrict__ miss_row, int center, int scale,
                                                   const double *__restrict__ pl, const uint32_t *__restrict__ X, int64_t nbp)
{
    // a NaN or +-Inf anywhere in the residual (its sum says so): the reference's floating-point mul! gives NaN or +-Inf in every column it
    // touches -- in every column of a centered matrix; the fixed point has no such value, so the answer is NaN in every column
    if (!(fabs(sum_r) <= 1.7976931348623157e308)) return __longlong_as_double(0x7ff8000000000000ll);
    double dot = 0.0;
    for (int s = 0; s < splits; ++s) dot += pu[(int64_t)s * pstride + j];
    if (pl) {
        // up to kPeelMax terms: a compensated sum (the rounding error of every addition is kept, exactly, and added at the end), so the
        // side channel costs ONE rounding of the result however many rows it carries -- a plain chain of 64 additions was 2.5 x 2^-53
        // sum_i g_ij |r_i| off when every non-zero row of a residual was peeled.  No row peeled: not an operation, not a bit.
        const int np = (int)pl[0];
        double comp = 0.0;
        for (int t = 0; t < np; ++t) {
            const int64_t i = (int64_t)pl[4 + t];
            const uint32_t g = (X[xword(nbp, j, i >> 4)] >> (2 * (int)(i & 15))) & 3u;
            const double x = (double)g * pl[4 + kPeelMax + t];          // exact
            const double s = dot + x, bb = s - dot;
            comp += (dot - (s - bb)) + (x - bb);
            dot = s;
        }
        if (np > 0 && fabs(comp) <= kMaxFinite) dot += comp;            // (a sum that overflowed stays +-Inf)
    }
    if (b > a) {
        double ms = 0.0;
        for (int64_t t = a; t < b; ++t) ms += ru[miss_row[t]];
        dot += m * ms;
    }
    if (center) dot -= m * sum_r;
    if (scale) dot *= si;
    return dot;
}
__global__ void __launch_bounds__(256)
k_xtv_finalize(const double *__restrict__ partial, int splits, int64_t pstride, int64_t p, int nres,
               const double *__restrict__ scal, const double *__restrict__ r, int64_t n,
               const double *__restrict__ mu, const double *__restrict__ sinv,
               const int64_t *__restrict__ miss_ptr, const int32_t *__restrict__ miss_row,
               int center, int scale, int impute, double *__restrict__ out,
               const int32_t *__restrict__ gate, int32_t gate_val, XtvSupportHook hook,
               const double *__restrict__ peel, const uint32_t *__restrict__ X, int64_t nbp)
{
    if (gate && *gate != gate_val) return;
    const int64_t pblocks = (p + 255) / 256;
    if ((int64_t)blockIdx.x >= pblocks) {          // the support of the current iterate (device-resident steps; nres == 1)
        const int c = *hook.cur;
        const int64_t t = ((int64_t)blockIdx.x - pblocks) * 256 + threadIdx.x;
        if (t >= *hook.cnt[c]) return;
        const int64_t j = hook.idx[c][t];
        const double m = mu[j], si = scale ? sinv[j] : 1.0;
        int64_t a = 0, b = 0;
        if (impute) { a = miss_ptr[j]; b = miss_ptr[j + 1]; }
        const double dot = xtv_finalize_col(j, partial, splits, pstride, scal[2], r, m, si, a, b, miss_row, center, scale, peel, X, nbp);
        const double av = si * dot;
        hook.gval[t] = dot; hook.A[t] = av; hook.B[t] = center ? -m * av : 0.0;
        return;
    }
    int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= p) return;
    const double m = mu[j], si = scale ? sinv[j] : 1.0;
    int64_t a = 0, b = 0;
    if (impute) { a = miss_ptr[j]; b = miss_ptr[j + 1]; }
    for (int u = 0; u < nres; ++u)
        out[(int64_t)u * p + j] = xtv_finalize_col(j, partial + (int64_t)u * splits * pstride, splits, pstride, scal[4 * u + 2],
                                                   r + (int64_t)u * n, m, si, a, b, miss_row, center, scale,
                                                   peel ? peel + (int64_t)u * kPeelStride : nullptr, X, nbp);
}
