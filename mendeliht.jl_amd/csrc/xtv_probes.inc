// xtv_probes.inc -- MEASUREMENT BUILD ONLY (-DMIH_PROBES, libmendeliht_hip_probes.so; included by xtv.hip inside namespace mih, behind xtv_kernels.h).
// Launch-shape sweeps of the ring kernels, the round-1 kernel families (register-staged k_xtv_mfma_lds; per-wave k_xtv_mfma, whose
// text lives here) kept as bit-for-bit cross-checks, and timing probes whose output is NOT X'r.  None of this is in libmendeliht_hip.so.
// The knobs are process-wide here on purpose: tools/ set them once per measurement (mih_probe_*), nothing else uses this library
// concurrently.
struct ProbeKnobs { int variant = -1, multi_variant = 0, max_nr = 4; };
static ProbeKnobs g_probe;

XtvTune xtv_tune(int digits)
{
    XtvTune t;
    t.digits = digits;
    t.variant = g_probe.variant; t.multi_variant = g_probe.multi_variant; t.max_nr = g_probe.max_nr;
    if (const char *e = getenv("MENDELIHT_XTV_MAX_OPS")) { int x = atoi(e); t.max_ops = x < 1 ? 1 : x > 6 ? 6 : x; }
    if (const char *e = getenv("MENDELIHT_XTV_SLICES")) { int v = atoi(e); if (v >= 1 && v <= kMaxSplits) t.slices = v; }
    if (const char *e = getenv("MENDELIHT_XTV_NO_HALF")) t.half = atoi(e) == 0;
    return t;
}

struct Variant { int waves, ct, splits; };
static const Variant kVariants[] = {
    {4, 2, 8},    // 0
    {4, 1, 8},    // 1
    {4, 4, 8},    // 2
    {8, 2, 8},    // 3
    {8, 1, 8},    // 4
    {4, 2, 1},    // 5: no row slicing
    {4, 1, 1},    // 6
    {4, 4, 1},    // 7
    {4, 2, 16},   // 8
    {2, 2, 8},    // 9
    {8, 4, 8},    // 10
    {4, 4, 4},    // 11
    {4, 4, 16},   // 12
    {4, 8, 8},    // 13
    {2, 4, 8},    // 14
    {8, 4, 16},   // 15
};
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

static int probe_splits(const XtvTune &tn) { return tn.variant >= 0 && tn.variant < kNumVariants ? kVariants[tn.variant].splits : 0; }

// NR right-hand sides ride the same pass: the dosage tile is loaded and expanded once and fed to NR
// MFMAs (one per residual vector's digit planes).
template <int WAVES, int CT, int NR>
__global__ void __launch_bounds__(WAVES * 64)
k_xtv_mfma(const uint4 *__restrict__ X, int64_t nbp, int64_t ncg, const uint4 *__restrict__ dig, int64_t dig_stride,
           int splits, DigitMode dm, const double *__restrict__ scal, double *__restrict__ partial /* [NR*per_op][splits][ncg*32] */)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int split = blockIdx.x % splits;
    const int64_t grp = blockIdx.x / splits;
    const int64_t cg0 = (grp * WAVES + wave) * CT;
    if (cg0 >= ncg) return;
    const int64_t bps = (nbp + splits - 1) / splits;
    const int64_t b0 = split * bps;
    const int64_t b1 = (b0 + bps < nbp) ? b0 + bps : nbp;

    f32x16 acc[CT][NR];
    #pragma unroll
    for (int c = 0; c < CT; ++c)
        #pragma unroll
        for (int v = 0; v < NR; ++v)
            #pragma unroll
            for (int g = 0; g < 16; ++g) acc[c][v][g] = 0.f;

    if (b0 < b1) {
        const uint4 *ap[CT];
        #pragma unroll
        for (int c = 0; c < CT; ++c) {
            int64_t cg = cg0 + c < ncg ? cg0 + c : ncg - 1;
            ap[c] = X + (cg * nbp) * 64 + lane;
        }
        const uint4 *bp_ = dig + lane;
        uint4 acur[CT], anext[CT], bcur[NR][2], bnext[NR][2];
        #pragma unroll
        for (int c = 0; c < CT; ++c) acur[c] = ld_stream(ap[c] + b0 * 64);
        #pragma unroll
        for (int v = 0; v < NR; ++v) { bcur[v][0] = bp_[v * dig_stride + (2 * b0) * 64]; bcur[v][1] = bp_[v * dig_stride + (2 * b0 + 1) * 64]; }
        for (int64_t bp = b0; bp < b1; ++bp) {
            const int64_t bn = (bp + 1 < b1) ? bp + 1 : bp;
            #pragma unroll
            for (int c = 0; c < CT; ++c) anext[c] = ld_stream(ap[c] + bn * 64);
            #pragma unroll
            for (int v = 0; v < NR; ++v) { bnext[v][0] = bp_[v * dig_stride + (2 * bn) * 64]; bnext[v][1] = bp_[v * dig_stride + (2 * bn + 1) * 64]; }
            #pragma unroll
            for (int c = 0; c < CT; ++c) {
                #pragma unroll
                for (int v = 0; v < NR; ++v) {
                    acc[c][v] = mfma_fp4(acur[c].x, acur[c].y, bcur[v][0], acc[c][v]);
                    acc[c][v] = mfma_fp4(acur[c].z, acur[c].w, bcur[v][1], acc[c][v]);
                }
            }
            #pragma unroll
            for (int c = 0; c < CT; ++c) acur[c] = anext[c];
            #pragma unroll
            for (int v = 0; v < NR; ++v) { bcur[v][0] = bnext[v][0]; bcur[v][1] = bnext[v][1]; }
        }
    }

    xtv_epilogue<CT, NR>(acc, lane, cg0, ncg, split, splits, dm, scal, partial);
}

template <int WAVES, int CT, int NR>
static void launch_xtv(const mih_mat *h, const uint4 *dig, int64_t dig_stride, int splits, DigitMode dm, const double *scal,
                       double *partial, hipStream_t s)
{
    int64_t groups = (h->ncg + WAVES * CT - 1) / (WAVES * CT);
    hipLaunchKernelGGL((k_xtv_mfma<WAVES, CT, NR>), dim3((unsigned)(groups * splits)), dim3(WAVES * 64), 0, s,
                       reinterpret_cast<const uint4 *>(h->X), h->nbp, h->ncg, dig, dig_stride, splits, dm, scal, partial);
}

// returns -1 when no probe shape is selected for this (format, operand count): the release dispatch runs
static int dispatch_probe(const XtvTune &tn, int nr, bool half, const mih_mat *h, const uint4 *dig, const uint2 *dig2, int64_t dig_stride,
                          int splits, DigitMode dm, const double *scal, double *partial, hipStream_t s, char *name)
{
    const int mv6 = tn.multi_variant;
    if (mv6 == 0 && tn.variant < 0) return -1;
    (void)half;
#define MIH_LDS6(NRV, ID, C, RB, W) if (nr == NRV && (mv6 == ID || ID < 0)) \
        MIH_LAUNCH((k_xtv_mfma_lds<NRV, C, RB, 0, W, true>), W, C, "k_xtv_mfma_lds<%d,%d,%d,%d,fp6>", NRV, C, RB, W)
#define MIH_DMA(NRV, ID, C, W, DD, F6, MODE) if (nr == NRV && (mv6 == ID || ID < 0)) \
        MIH_LAUNCH((k_xtv_dma<NRV, C, W, DD, F6, MODE>), W, C, "k_xtv_dma<%d,%d,%d,%d,%s%s>", NRV, C, W, DD, F6 ? "fp6" : "fp4", MODE ? ",probe" : "")
#define MIH_DMA16M(NRV, ID, C, W, DD, MODE) if (nr == NRV && mv6 == ID) \
        MIH_LAUNCH((k_xtv_dma16<NRV, C, W, DD, MODE, 0>), W, C, "k_xtv_dma16<%d,%d,%d,%d%s>", NRV, C, W, DD, MODE ? ",probe" : "")
    if (dm.base == 49 && dm.lay16) {      // ids 40..49: other shapes of the 16x16x128 ring kernel; everything else: release defaults
        MIH_DMA16M(4, 40, 4, 4, 4, 0) MIH_DMA16M(3, 40, 4, 4, 4, 0) MIH_DMA16M(2, 40, 4, 4, 4, 0) MIH_DMA16M(1, 40, 4, 4, 4, 0)
        MIH_DMA16M(4, 42, 2, 8, 3, 0) MIH_DMA16M(4, 43, 2, 8, 2, 0)
        MIH_DMA16M(4, 41, 2, 8, 4, 4) MIH_DMA16M(5, 41, 2, 8, 4, 4)       // round 2's paired LDS loads (ds_read2_b64: bank conflicts), same X'R
        MIH_DMA16M(1, 49, 2, 8, 4, 3) MIH_DMA16M(4, 49, 2, 8, 4, 3)       // timing probes: the odd fragments skipped (NOT X'r)
        MIH_DMA16M(1, 44, 2, 4, 8, 0) MIH_DMA16M(1, 45, 1, 8, 6, 0) MIH_DMA16M(1, 46, 2, 4, 6, 0) MIH_DMA16M(1, 47, 4, 4, 4, 0) MIH_DMA16M(1, 48, 2, 8, 6, 0)
        return -1;
    }
#undef MIH_DMA16M
    if (dm.base == 49) {           // FP6 digit planes in the 32-column layout: the 32x32x64 kernels
        // LDS-DMA ring kernels: tuning shapes (ids 20..), timing probes (30..: results are NOT X'R), then the defaults
        MIH_DMA(4, 20, 4, 4, 4, true, 0) MIH_DMA(4, 21, 4, 4, 3, true, 0) MIH_DMA(4, 22, 2, 8, 4, true, 0) MIH_DMA(4, 23, 2, 8, 3, true, 0)
        MIH_DMA(4, 24, 4, 4, 2, true, 0) MIH_DMA(4, 25, 2, 8, 2, true, 0)
        MIH_DMA(4, 30, 4, 4, 4, true, 1) MIH_DMA(4, 31, 4, 4, 4, true, 2) MIH_DMA(4, 32, 2, 8, 4, true, 1) MIH_DMA(4, 33, 2, 8, 4, true, 2)
        MIH_DMA(3, 20, 4, 4, 4, true, 0) MIH_DMA(3, 22, 2, 8, 4, true, 0) MIH_DMA(2, 20, 4, 4, 4, true, 0) MIH_DMA(2, 22, 2, 8, 4, true, 0)
        MIH_DMA(1, 20, 4, 4, 4, true, 0) MIH_DMA(1, 22, 2, 8, 4, true, 0) MIH_DMA(1, 26, 1, 8, 4, true, 0) MIH_DMA(1, 27, 1, 16, 4, true, 0)
        if (mv6 >= 16) {      // the 32x32x64 ring shapes of other operand counts (ids 1..15 select the register-staged LDS shapes below)
            MIH_DMA(4, -1, 4, 4, 4, true, 0) MIH_DMA(3, -1, 4, 4, 4, true, 0) MIH_DMA(2, -1, 2, 8, 4, true, 0) MIH_DMA(1, -1, 2, 8, 4, true, 0)
        }
        MIH_LDS6(4, 1, 2, 2, 8) MIH_LDS6(4, 2, 1, 4, 8) MIH_LDS6(4, 3, 2, 2, 4) MIH_LDS6(4, 4, 2, 1, 4) MIH_LDS6(4, 5, 1, 2, 8)
        MIH_LDS6(1, 10, 1, 2, 8) MIH_LDS6(1, 11, 2, 4, 8) MIH_LDS6(1, 12, 2, 2, 8) MIH_LDS6(1, 13, 4, 2, 8) MIH_LDS6(1, 14, 1, 4, 16) MIH_LDS6(1, 15, 2, 2, 16)
        // register-staged defaults (2 operands: <2,4,1,4> 22.5 ms against 23.3-26 ms for five other shapes; 3 operands: <3,2,2,4> 33.2 ms
        // against 34.5 ms for <3,2,2,8>; 4 operands: <4,2,1,8> 39.4 ms against 40.6 ms for <4,2,2,8>, same box)
        MIH_LDS6(1, -1, 1, 4, 8) MIH_LDS6(2, -1, 4, 1, 4) MIH_LDS6(3, -1, 2, 2, 4) MIH_LDS6(4, -1, 2, 1, 8)
        set_error("unsupported operand count");
        return MIH_BAD_ARG;
    }
#undef MIH_LDS6
#define MIH_LDS(NRV, ID, C, RB, MODE, W) if (nr == NRV && mv6 == ID) \
        MIH_LAUNCH((k_xtv_mfma_lds<NRV, C, RB, MODE, W>), W, C, "k_xtv_mfma_lds<%d,%d,%d,%d,fp4%s>", NRV, C, RB, W, MODE ? ",probe" : "")
    // FP4 digit planes through the LDS-DMA ring (tuning shapes)
    MIH_DMA(4, 20, 4, 4, 4, false, 0) MIH_DMA(4, 22, 2, 8, 4, false, 0) MIH_DMA(3, 20, 4, 4, 4, false, 0) MIH_DMA(2, 20, 4, 4, 4, false, 0)
    MIH_DMA(2, 22, 2, 8, 4, false, 0)
    if (tn.variant < 0) {
        MIH_DMA(1, 20, 1, 8, 6, false, 0) MIH_DMA(1, 21, 2, 8, 4, false, 0) MIH_DMA(1, 22, 1, 16, 6, false, 0) MIH_DMA(1, 23, 2, 4, 8, false, 0)
        MIH_DMA(1, 24, 4, 4, 4, false, 0) MIH_DMA(1, 25, 1, 8, 3, false, 0) MIH_DMA(1, 26, 2, 8, 6, false, 0) MIH_DMA(1, 27, 1, 8, 8, false, 0)
        MIH_DMA(1, 28, 2, 4, 12, false, 0) MIH_DMA(1, 29, 4, 4, 6, false, 0) MIH_DMA(1, 34, 2, 4, 6, false, 0) MIH_DMA(1, 35, 2, 2, 8, false, 0)
    }
    if (nr == 4 || nr == 2) {
        MIH_LDS(4, 1, 2, 1, 0, 8) MIH_LDS(4, 2, 2, 3, 0, 8) MIH_LDS(4, 3, 2, 4, 0, 8) MIH_LDS(4, 4, 1, 4, 0, 8)
        MIH_LDS(4, 5, 2, 1, 0, 4) MIH_LDS(4, 6, 2, 2, 0, 4)
        MIH_LDS(4, 7, 2, 2, 1, 8) MIH_LDS(4, 8, 2, 2, 2, 8)      // timing probes (results are NOT X'r)
        MIH_LDS(2, 1, 2, 2, 0, 8) MIH_LDS(2, 2, 4, 2, 0, 8) MIH_LDS(2, 3, 2, 4, 0, 8) MIH_LDS(2, 4, 4, 1, 0, 8)
        if (nr == 2 && mv6 == 5) { launch_xtv<4, 2, 2>(h, dig, dig_stride, splits, dm, scal, partial, s); snprintf(name, 48, "k_xtv_mfma<4,2,2>"); return MIH_OK; }   // per-wave digit loads
        return -1;             // ids that exist for other operand counts only: the release shapes
    }
    if (nr == 1 && tn.variant < 0 && mv6 >= 1 && mv6 < 16) {
        // the register-staged single-operand shapes (digit planes staged through registers once per workgroup): round 1's default
        // was <1,1,4> (17.86 ms against 18.47 ms for the per-wave-load kernels at n=500k, p=1M; tools/sweep_single_lds.py)
        MIH_LDS(1, 10, 1, 2, 0, 8) MIH_LDS(1, 11, 1, 6, 0, 8) MIH_LDS(1, 12, 1, 2, 0, 16) MIH_LDS(1, 13, 2, 4, 0, 8) MIH_LDS(1, 14, 4, 2, 0, 8)
        MIH_LDS(1, 15, 1, 4, 1, 8)                        // timing probe: loads only, no MFMAs (result is NOT X'r)
        { MIH_LDS(1, mv6, 1, 4, 0, 8) }                   // id 9 and the multi-operand ids
    }
#undef MIH_LDS
#undef MIH_DMA
    if (nr == 1 && tn.variant >= 0 && tn.variant < kNumVariants) {       // round 1's per-wave-load kernels
        const Variant v = kVariants[tn.variant];
#define MIH_CASE(W, C) if (v.waves == W && v.ct == C) { launch_xtv<W, C, 1>(h, dig, dig_stride, splits, dm, scal, partial, s); \
        snprintf(name, 48, "k_xtv_mfma<%d,%d,1>", W, C); return MIH_OK; }
        MIH_CASE(4, 1) MIH_CASE(4, 2) MIH_CASE(4, 4) MIH_CASE(8, 1) MIH_CASE(8, 2) MIH_CASE(2, 2) MIH_CASE(8, 4) MIH_CASE(4, 8) MIH_CASE(2, 4)
#undef MIH_CASE
        set_error("unknown X'r kernel variant");
        return MIH_BAD_ARG;
    }
    return -1;
}

extern "C" {
// Select the single-operand X'r kernel used by every subsequent call: -1 = library default, 0..15 = the per-wave-load shapes
// {waves, column groups, row slices}.
int mih_probe_set_xtv_variant(int variant)
{
    if (variant < -1 || variant >= kNumVariants) { set_error("variant %d out of range", variant); return MIH_BAD_ARG; }
    g_probe.variant = variant;
    return MIH_OK;
}
// Launch shape of the LDS-shared / ring kernels: 0 = release defaults; 1..15 = round-1 register-staged shapes (6 / 9: its defaults);
// 20.. = 32x32x64 ring shapes; 40.. = 16x16x128 ring shapes; 7, 8, 15, 30..33, 49 = timing probes whose output is NOT X'r.
int mih_probe_set_xtv_multi_variant(int variant)
{
    if (variant < 0 || variant > 63) { set_error("multi-RHS variant %d out of range", variant); return MIH_BAD_ARG; }
    g_probe.multi_variant = variant;
    return MIH_OK;
}
// B operands fused per pass of the register-staged kernels (1, 2 or 4)
int mih_probe_set_max_fused(int max_nr)
{
    if (max_nr != 1 && max_nr != 2 && max_nr != 4) { set_error("max_fused must be 1, 2 or 4"); return MIH_BAD_ARG; }
    g_probe.max_nr = max_nr;
    return MIH_OK;
}
}
