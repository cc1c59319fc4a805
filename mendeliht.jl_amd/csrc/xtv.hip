// xtv.hip -- out = X' r over the 2-bit genotype matrix: the hot loop of the IHT iteration.
// Replaces `mul!(v.df, Transpose(x), v.r)` (src/utilities.jl:133; SnpArrays.jl linalg_direct.jl
// `_snparray_AtX_*` kernels) and, batched, `SnpArrays.mul!(p_by_r, Transpose(sla), n_by_r)`
// (src/multivariate.jl:85).
//
//   out_j = sinv_j * ( sum_i g_ij r_i  [+ mu_j * sum_{i missing in j} r_i]  - mu_j * sum_i r_i )
//
// Why this is not a plain f64 FMA loop.  Measured on MI355X (tools/instbench.hip): a wave64
// v_fma_f64 costs 2.2 ns per SIMD and the cheapest dosage->double decode (one SDWA byte-select AND)
// 1.85 ns, so a decode+FMA kernel tops out at ~4.0 TB/s of 2-bit data (50 % of the HBM peak) with
// the memory system half idle (the round-1 VALU kernel reached 3.5 TB/s).  The dosage matrix is
// exact small-integer data, so the dot products are done EXACTLY in fixed point on the matrix pipe:
//   * a 2-bit dosage code placed in the low bits of a nibble IS the FP4 (e2m1) number g/2, so the
//     A operand of v_mfma_scale_f32_32x32x64_f8f6f4 is built with one AND per 8 dosages;
//   * r is scaled by a power of two, rounded to an integer R (|R| < 2^54) and written in a positional system
//     whose digits the pipe represents exactly -- each digit set is a complete residue system of its base, so the
//     representation exists, is unique and is found by one pass of divisions per row (DigitMode, k_digits):
//       base  4, digits {-2,-1,0,1}/2                        FP4 e2m1, 28 columns, 1 residual per B operand
//       base 13, digits {-8,-6,-4..4,6,8}/2                  FP4 e2m1, 16 columns (|R| < 2^57), 2 per operand
//       base 49, digits {-32..-18 even, -16..16, 18..32 even}/8  FP6 e2m3, 10 columns, 3 per operand
//     The digit planes of a residual are columns of the 32-column B operand, so ONE MFMA multiplies a
//     32-SNP x 64-row dosage tile with all digits of the operand's residuals.  A single fit uses base 4 (the
//     fastest single-operand pass), every fused multi-RHS context base 49 (fewest MFMAs per residual: those
//     passes are bound by the matrix pipe's power);
//   * every product is a multiple of 1/4 (FP4) or 1/16 (FP6) of magnitude <= 4 and a row slice is short enough
//     (2^22 / 2^20 / 2^18 rows) that every partial sum stays below 2^24 such units: the f32 accumulators are exact
//     and the result does not depend on summation order (bit-reproducible);
//   * the digit sums are recombined in f64 (sum_t base^t * S_t, fixed order) and rescaled by 2^-e.
// The inexact steps are the rounding of r to 2^-54 of max|r| and the few f64 operations that recombine the
// digit sums (fixed order, so bit-reproducible for a given row slicing) -- tighter than the rounding an
// n-term f64 dot product accumulates.  Per 2048 dosages: 1 MFMA (13.7 ns/SIMD) + ~8 VALU ops, far
// below the 87 ns/SIMD the HBM stream allows at 6 TB/s, so the single-operand kernel is memory-bound.
//
// Work decomposition: a wave owns CT column groups (32 SNPs each) and walks a slice of the rows in
// 128-row steps; per step it loads CT x 1 KB of dosages (one contiguous 16 B/lane wave-load per
// tile) and needs the 2 KB of digit planes for those rows.  Rows are split in `splits` slices
// (slice = blockIdx % splits: the blocks of one XCD share a slice of the digit planes in their L2);
// slice partials are combined in fixed order by the finalize kernel.  The kernels (xtv_kernels.h; same arithmetic, same bits):
//   k_xtv_dma / k_xtv_dma16      every operand through an LDS-DMA ring: the single-fit pass and the fused FP6 passes;
//   k_xtv_mfma_lds<NR,CT,RB,..>  the digit planes of a 128-row block are staged ONCE per workgroup in LDS through registers
//                                (2 - 4 FP4 operands per pass);
//   k_xtv_mfma<WAVES,CT,NR>      every wave loads its own digit planes from L2 (round 1's shapes: a cross-check of the
//                                measurement build, xtv_probes.inc).
// This file: the residual formats, the dispatch, the workspace, the pass plan and the C entry points.  The residual's statistics
// and digit planes are xtv_digits.hip, dense and 16-bit dosage matrices xtv_dense.hip.
// An operand carries one 28-digit base-4 residual, two 16-digit base-13 residuals, three 10-digit base-49 residuals,
// or four 8-digit residuals (opt-in fast modes): DigitMode.
#include "common.h"
#include "peel.h"
#include <algorithm>

namespace mih {

#include "xtv_kernels.h"

constexpr int kMaxSplits = 16;

// the signature of every 2-bit kernel (but round 1's k_xtv_mfma, which takes no `dig2`), and their launch: a workgroup of
// `waves` waves x `ct` column groups per (group of columns, row slice)
typedef void (*XtvKernel)(const uint4 *X, int64_t nbp, int64_t ncg, const uint4 *dig, const uint2 *dig2, int64_t dig_stride, int splits,
                          DigitMode dm, const double *scal, double *partial);
static void launch_xtv_kernel(XtvKernel kernel, int waves, int ct, const mih_mat *h, const uint4 *dig, const uint2 *dig2, int64_t dig_stride,
                              int splits, const DigitMode &dm, const double *scal, double *partial, hipStream_t s)
{
    const int64_t groups = (h->ncg + waves * ct - 1) / (waves * ct);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(groups * splits)), dim3(waves * 64), 0, s,
                       reinterpret_cast<const uint4 *>(h->X), h->nbp, h->ncg, dig, dig2, dig_stride, splits, dm, scal, partial);
}
// in a dispatch function: launch the instantiation KERNEL in the shape (W waves, C column groups), leave its name, done
#define MIH_LAUNCH(KERNEL, W, C, ...) { \
        launch_xtv_kernel(KERNEL, W, C, h, dig, dig2, dig_stride, splits, dm, scal, partial, s); \
        snprintf(name, 48, __VA_ARGS__); \
        return MIH_OK; }

// mih_fit_params::xtv_digits / the digits argument of mih_xtv_batched_fmt (ids = base * 100 + digits, include/mendeliht_hip.h)
static bool digit_mode(int id, DigitMode &dm)
{
    switch (id) {
    case -1:                                                  // auto (lock-step drivers): 4910, and 4908 for the residuals whose range allows it
    case 0:
    case 4910: dm = {49, 10, 3, 10, 53, 18}; return true;    // FP6, three residuals per operand, |R| < 2^54
    case 4908: dm = {49, 8, 4, 8, 42, 18}; return true;      // FP6, four per operand, |R| < 2^43 (opt-in fast mode)
    case 1316: dm = {13, 16, 2, 16, 56, 20}; return true;    // FP4, two per operand, |R| < 2^57
    case 1308: dm = {13, 8, 4, 8, 26, 20}; return true;      // FP4, four per operand, |R| < 2^27
    case 428:  dm = {4, 28, 1, 32, 53, 22}; return true;     // FP4, one per operand, |R| < 2^54
    }
    return false;
}
bool xtv_digits_valid(int digits) { DigitMode dm; return digit_mode(digits, dm); }

#ifdef MIH_PROBES
#include "xtv_probes.inc"       // launch-shape sweeps, round-1 kernel families, timing probes: measurement build only
#else
XtvTune xtv_tune(int digits) { XtvTune t; t.digits = digits; return t; }
static int dispatch_probe(const XtvTune &, int, bool, const mih_mat *, const uint4 *, const uint2 *, int64_t, int, DigitMode,
                          const double *, double *, hipStream_t, char *) { return -1; }
static int probe_splits(const XtvTune &) { return 0; }
#endif

// nr B operands per pass, each carrying per_op residuals.  The release library has ONE kernel per (format family, operand
// count):
//   FP6 planes (4910 / 4908):  k_xtv_dma16<nr,2,8,D,0,half>  -- the 16x16x128 LDS-DMA ring (12 residuals at n=500k, p=1M:
//                              28.5 ms against 34.3 ms for the 32x32x64 ring kernel and 40.0 ms register-staged)
//   FP4 planes, one operand:   k_xtv_dma<1,2,4,8,fp4>         -- the single-fit pass (17.6 ms = 88.8 % of the HBM peak)
//   FP4 planes, 2-4 operands:  k_xtv_mfma_lds<nr,..>          -- register-staged; only matrices too tall for FP6 slices
//                                                                (> 2^22 rows) or an explicit 1316 / 1308 / 428 get here
// `name` receives the dispatched kernel's name (profile records).
static int dispatch_xtv(const XtvTune &tn, int nr, bool half, const mih_mat *h, const uint4 *dig, const uint2 *dig2, int64_t dig_stride,
                        int splits, DigitMode dm, const double *scal, double *partial, hipStream_t s, char *name)
{
    {
        const int rc = dispatch_probe(tn, nr, half, h, dig, dig2, dig_stride, splits, dm, scal, partial, s, name);
        if (rc >= 0) return rc;
    }
#define MIH_DMA16(NRV, C, W, DD, HF) if (nr == NRV && (int)half == HF) \
        MIH_LAUNCH((k_xtv_dma16<NRV, C, W, DD, 0, HF>), W, C, "k_xtv_dma16<%d,%d,%d,%d%s>", NRV, C, W, DD, HF ? ",half" : "")
    if (dm.base == 49) {
        if (!dm.lay16) { set_error("FP6 digit planes need the 16-column layout"); return MIH_BAD_ARG; }
        // 5 operands = 15 residuals: 224 VGPRs, 155 KB of LDS at D = 4; 6 operands = 18 residuals: 254 VGPRs, 136 KB at D = 3
        // (ring depths 2, 3, 4 are equally fast once one step is ahead: 28.8 / 28.9 / 29.0 ms at 12 residuals)
        MIH_DMA16(6, 2, 8, 3, 1) MIH_DMA16(5, 2, 8, 4, 1) MIH_DMA16(4, 2, 8, 4, 1) MIH_DMA16(3, 2, 8, 4, 1) MIH_DMA16(2, 2, 8, 4, 1) MIH_DMA16(1, 2, 8, 4, 1)
        MIH_DMA16(6, 2, 8, 3, 0) MIH_DMA16(5, 2, 8, 4, 0) MIH_DMA16(4, 2, 8, 4, 0) MIH_DMA16(3, 2, 8, 4, 0) MIH_DMA16(2, 2, 8, 4, 0) MIH_DMA16(1, 2, 8, 4, 0)
        set_error("unsupported operand count %d", nr);
        return MIH_BAD_ARG;
    }
#undef MIH_DMA16
    if (nr == 1) MIH_LAUNCH((k_xtv_dma<1, 2, 4, 8, false, 0>), 4, 2, "k_xtv_dma<1,2,4,8,fp4>")
#define MIH_LDS(NRV, C, RB, W) if (nr == NRV) \
        MIH_LAUNCH((k_xtv_mfma_lds<NRV, C, RB, 0, W>), W, C, "k_xtv_mfma_lds<%d,%d,%d,%d,fp4>", NRV, C, RB, W)
    MIH_LDS(4, 2, 2, 8) MIH_LDS(3, 2, 2, 8) MIH_LDS(2, 4, 1, 4)
#undef MIH_LDS
#undef MIH_LAUNCH
    set_error("unsupported operand count %d", nr);
    return MIH_BAD_ARG;
}

// Row slices of the library-default kernels.  A slice should hold about 50 000 rows or more -- every (column group,
// slice) work item pays a prologue and a 16-accumulator epilogue, and short items lose to that: at n = 50 000 one
// slice runs at 87 % of the HBM peak and eight at 75 %, at n = 10 000 it is 74 % against 38 % -- but there must be
// enough workgroups to fill 256 CUs.  At n = 500 000 round 1's kernels were best with eight slices (87.0 % against 83.3 % for
// one); with the LDS-DMA ring kernels FOUR are (round 3, tools/sweep_slices*.py, alternated in one process: single-fit pass
// 17.57 ms against 17.63 ms with eight, 18 residuals 38.9-39.1 against 39.2-39.4 ms) -- and the count must divide the 8 XCDs
// (slice = blockIdx % slices; five slices: 18.76 ms).
static int auto_splits(const mih_mat *h, const XtvTune &tn)
{
    if (tn.slices >= 1 && tn.slices <= kMaxSplits) return tn.slices;       // measurement build only
    int s = 1;
    while (s < 4 && h->n >= 100000ll * s) s *= 2;
    const int64_t groups = (h->ncg + 15) / 16;                 // workgroups per slice of the widest launch shape
    while (s < 16 && groups * s < 2048 && h->nbp / (2 * s) >= 8) s *= 2;
    return s;
}

// the row slices of a pass: the rule above, at least what exact f32 accumulation needs (|g/2 * d/2| <= 1 (base 4) or 4 (base 13)
// in units of 1/4, so a row slice may hold at most 2^22 / 2^20 rows), at most one per 128-row block and `cap`; -1: too tall
static int pass_splits(const mih_mat *h, int splits, const DigitMode &dm, int cap)
{
    const int64_t need = (h->n_pad + (1ll << dm.rows_log2) - 1) >> dm.rows_log2;
    if (need > cap) return -1;
    if (splits < need) splits = (int)need;
    if (splits > h->nbp) splits = (int)h->nbp;
    if (splits > cap) splits = cap;
    return splits;
}
int xtv_default_splits(const mih_mat *h, const DigitMode &dm) { return pass_splits(h, auto_splits(h, XtvTune()), dm, kMaxSplits); }

// The single-residual pass over the matrix's score image (score_image.hip) in place of k_xtv_dma<1,2,4,8,fp4>: k_xtv_hom (the
// digit sums of the one-bit columns' dosage-2 entries), then the class-2 region with the 2-bit kernel's own code and the class-1
// region with its one-bit variant.  Same row slices, same partial[slice][column]: the finalize kernel is untouched.
static void launch_xtv_image(const ScoreImage &im, const XtvWork &w, const mih_mat *h, const uint4 *dig, const uint2 *dig2, int64_t dig_stride,
                             int splits, DigitMode dm, const double *scal, double *partial, hipStream_t s, char *name)
{
    constexpr int W = 4, C = 2;
    launch_xtv_hom(im, w.hom_u.p, w.hom.p, dm.gate, dm.gate_val, s);
    dm.img_pstride = h->ncg * 32; dm.img_p1 = im.pos1; dm.img_hom = w.hom.p;
    if (im.ncg2 > 0) {
        dm.img_col = im.col_of;
        hipLaunchKernelGGL((k_xtv_dma<1, C, W, 8, false, 0, 1>), dim3((unsigned)((im.ncg2 + W * C - 1) / (W * C) * splits)), dim3(W * 64), 0, s,
                           reinterpret_cast<const uint4 *>(im.tiles), im.nbp, im.ncg2, dig, dig2, dig_stride, splits, dm, scal, partial);
    }
    if (im.nt1 > 0) {
        dm.img_col = im.col_of + im.ncg2 * 32;
        // (one tile = two column groups per wave: twice the workgroups of half the length, a shorter tail behind the class-2 launch)
        hipLaunchKernelGGL((k_xtv_dma<1, 1, W, 8, false, 0, 2>), dim3((unsigned)((im.nt1 + W - 1) / W * splits)), dim3(W * 64), 0, s,
                           reinterpret_cast<const uint4 *>(im.tiles + (size_t)im.ncg2 * (size_t)im.nbp * 1024), im.nbp, im.nt1, dig, dig2, dig_stride,
                           splits, dm, scal, partial);
    }
    snprintf(name, 48, "k_xtv_dma_img<1,2|1,4,8,fp4>+k_xtv_hom");       // (CT = 2 over the class-2 region | 1 over the class-1 region)
}

// FP6 digit planes are written in the 16-column layout when the pass runs on the 16x16x128 kernels (always, in the release
// library; the measurement build also has 32x32x64 shapes)
static bool xtv_lay16(const DigitMode &dm, const XtvTune &tn)
{
    return dm.base == 49 && tn.variant < 0 && (tn.multi_variant == 0 || (tn.multi_variant >= 40 && tn.multi_variant < 50));
}

// Flat packing of the digit columns (DigitMode::flat): the ten-digit format on the product's 16x16x128 kernels.  Three residuals
// per operand leave 2 of 32 columns idle; packed back to back, 19 residuals fit the 192 columns of a six-operand pass instead of
// 18, 16 fit five operands instead of five and a half.  (The other launch shapes of the measurement build keep the per-operand
// layout: same bits, they are the cross-check.)
static bool xtv_flat(const DigitMode &dm, const XtvTune &tn)
{
    return xtv_lay16(dm, tn) && tn.multi_variant == 0 && dm.slots * dm.per_op < 32 && tn.max_nr >= 4;
}
// residuals a full pass of the fused kernel scores
static int xtv_pass_residuals(const DigitMode &dm, const XtvTune &tn)
{
    return xtv_flat(dm, tn) ? (tn.max_ops * 32) / dm.slots : tn.max_ops * dm.per_op;
}

static void choose_mode(const mih_mat *h, const XtvTune &tn, bool batched, DigitMode &dm)
{
    digit_mode(tn.digits, dm);
    if (tn.digits == 0 || tn.digits == -1) {
        // Library default.  The workspace of a single fit scores one residual per pass: 28 sparse base-4 digit
        // columns make the fastest single-operand pass (17.86 ms against 17.99 ms for 16 base-13 columns and
        // 18.4 ms for FP6 planes at n=500k, p=1M; tools/sweep_fp6_single.py).  Every fused multi-RHS context
        // (cv_iht, model paths, multivariate fits, init_beta, mih_xtv_batched) uses the FP6 format whatever the
        // number of residuals in a call, so results never depend on how residuals are batched.  Larger digits mean
        // shorter exact row slices (2^18 rows in base 49, 2^20 in base 13, 2^22 in base 4), so very tall matrices
        // step down.
        if (!batched) digit_mode(428, dm);
        else if (tn.variant >= 0 || h->n_pad > ((int64_t)kMaxSplits << dm.rows_log2)) digit_mode(1316, dm);
        if (h->n_pad > ((int64_t)kMaxSplits << dm.rows_log2)) digit_mode(428, dm);
    }
}

// the pass the score image serves: the 428 format on the product's kernel and row slices (xtv_work_init pins an image on this condition,
// the automatic rule builds one on it)
static bool image_pass(const DigitMode &dm, const XtvTune &tn)
{
    return dm.base == 4 && tn.variant < 0 && tn.multi_variant == 0 && tn.slices == 0;
}
bool xtv_rides_image(const mih_mat *h, const XtvTune &tn)        // ... for the workspace of a single fit (batched = false)
{
    if (h->kind != 0 || !xtv_digits_valid(tn.digits)) return false;
    DigitMode dm;
    choose_mode(h, tn, false, dm);
    return image_pass(dm, tn);
}

int xtv_lockstep_width(const mih_mat *h, const XtvTune &tn)
{
    if (h->kind != 0) return 16;
    DigitMode dm;
    choose_mode(h, tn, true, dm);
    if (xtv_lay16(dm, tn)) return 2 * xtv_pass_residuals(dm, tn);    // two lanes of one full pass each
    return 8 * dm.per_op;
}

int xtv_work_init(const mih_mat *h, XtvWork &w, int m, const XtvTune &tune, bool batched)
{
    w.tune = tune;
    if (h->kind != 0) return MIH_OK;
    if (!xtv_digits_valid(tune.digits)) { set_error("residual format must be 0 (default), -1 (auto in lock-step drivers), 4910, 4908, 1316, 1308 or 428"); return MIH_BAD_ARG; }
    int64_t nblk = h->nbp * 2;
    choose_mode(h, tune, batched, w.dm);
    w.has_alt = tune.digits == -1 && batched && w.dm.base == 49 && w.dm.ndig == 10;      // (a matrix too tall for FP6 slices stepped down: no 43-bit twin)
    w.use_alt = false;
    if (w.dm.base == 49 && tune.variant >= 0) {         // only an explicitly requested FP6 format can get here (measurement build)
        set_error("the FP6 residual formats need the default kernel (variant -1)");
        return MIH_BAD_ARG;
    }
    int ops = (m + w.dm.per_op - 1) / w.dm.per_op;
    size_t rhs_cap = (size_t)ops * w.dm.per_op;
    if (xtv_flat(w.dm, tune)) {          // flat packing: ceil(10 m' / 32) operands plus at most one partly used per pass, for any m' <= m
        const int cap = xtv_pass_residuals(w.dm, tune), npass = (m + cap - 1) / cap;
        if (npass <= kMaxFlatPasses) { ops = (m * w.dm.slots + 31) / 32 + npass; rhs_cap = (size_t)m; }
    }
    w.ops_cap = ops; w.rhs_cap = rhs_cap;
    const size_t lanes = (size_t)w.ops_cap * (size_t)nblk * 64;
    const size_t dwords = lanes * (w.dm.base == 49 ? 6 : 4);
    MIH_TRY(w.digits.alloc(dwords));
    MIH_TRY(w.partial.alloc((size_t)kMaxSplits * rhs_cap * (size_t)h->ncg * 32));
    MIH_TRY(w.scal.alloc(rhs_cap * 4 + (size_t)m * kStatBlocks * 2));
    MIH_TRY(w.stat_done.alloc(rhs_cap));
    MIH_TRY(w.peel.alloc(rhs_cap * kPeelStride));
    MIH_HIP(hipMemsetAsync(w.peel.p, 0, sizeof(double) * rhs_cap * kPeelStride, h->stream));       // (no rows peeled; the guards' running counts at zero)
    MIH_HIP(hipMemset(w.stat_done.p, 0, sizeof(unsigned) * rhs_cap));       // k_r_stats leaves its counters at zero
    MIH_HIP(hipMemsetAsync(w.digits.p, 0, sizeof(*w.digits.p) * dwords, h->stream));
    MIH_HIP(hipMemsetAsync(w.scal.p, 0, sizeof(double) * rhs_cap * 4, h->stream));
    MIH_HIP(hipStreamSynchronize(h->stream));
    w.m_cap = m; w.splits_cap = kMaxSplits;
    // a single-residual workspace in the 428 format rides the matrix's score image if it has one now, and pins it
    w.img.reset();
    if (m == 1 && image_pass(w.dm, tune)) {
        std::shared_ptr<const ScoreImage> im = score_image_of(h);
        if (im && im->nbp == h->nbp) {
            if (w.hom_u.alloc((size_t)h->n_pad) == MIH_OK && w.hom.alloc(std::max<size_t>((size_t)im->splits * (size_t)im->pos1 * 32, 1)) == MIH_OK) w.img = im;
            else { w.hom_u.release(); w.hom.release(); }          // no room for the scratch: the 2-bit pass
        }
    }
    return MIH_OK;
}

// measurement hook: how often the outlier guard (peel.h) of this workspace's residual slots has fired since the last call
// (MIH_CNT_PEELED_RESIDUALS); synchronises the stream
void xtv_count_peels(const mih_mat *h, XtvWork &w, hipStream_t s)
{
    if (!h->prof->on || !w.peel.p || w.rhs_cap == 0) return;
    // (the whole buffer in ONE plain copy, <= 20 KB: a strided hipMemcpy2DAsync of the counts alone took ~6 ms per call in a process
    // that also holds PyTorch's HIP runtime -- bench.py's host-driven A/B read 0.64 ms outside the pass instead of 0.31)
    std::vector<double> c(w.rhs_cap * kPeelStride, 0.0);
    if (hipMemcpyAsync(c.data(), w.peel.p, sizeof(double) * c.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return; }
    double total = 0.0;
    for (size_t v = 0; v < w.rhs_cap; ++v) total += c[v * kPeelStride + 3];
    h->prof->count(MIH_CNT_PEELED_RESIDUALS, (int64_t)(total - w.peels_counted));
    w.peels_counted = total;
}

// One fused pass: residuals [u0, u1) ride the nr B operands from operand t; half: the last operand's second 16-column fragment is empty.
struct XtvPass { int u0, u1, t, nr; bool half; };

// The passes that score m residuals.  Flat packing (sets dm.flat): the residuals are dealt out evenly over as few passes as hold them,
// a pass takes ceil(10 cnt / 32) operands -- never more than the per-operand layout needs.  Otherwise whole operands of per_op residuals:
// 4, 3 or 2 a pass for the register-staged kernels, up to max_ops for the 16x16x128 ring, the remainder split evenly.
static std::vector<XtvPass> plan_passes(DigitMode &dm, const XtvTune &tn, int m)
{
    std::vector<XtvPass> passes;
    if (xtv_flat(dm, tn)) {
        const int cap = xtv_pass_residuals(dm, tn), npass = (m + cap - 1) / cap;
        if (npass <= kMaxFlatPasses) {
            dm.flat = 1;
            for (int q = 0, u = 0, t = 0; q < npass; ++q) {
                const int cnt = m / npass + (q < m % npass ? 1 : 0), nr = (cnt * dm.slots + 31) / 32;
                passes.push_back({u, u + cnt, t, nr, tn.half && cnt * dm.slots - 32 * (nr - 1) <= 16});
                u += cnt; t += nr;
            }
            return passes;
        }
    }
    const int per_op = dm.per_op, nops = (m + per_op - 1) / per_op;
    for (int t = 0; t < nops;) {          // t counts B operands
        int nr = (nops - t >= 4 && nops - t != 5 && tn.max_nr >= 4) ? 4 : ((nops - t == 3 || nops - t == 5) && tn.max_nr >= 4) ? 3
                 : (nops - t >= 2 && tn.max_nr >= 2) ? 2 : 1;
        if (dm.lay16 && tn.max_nr >= 4) {          // up to max_ops operands a pass, the remainder split evenly
            const int rem = nops - t, mo = tn.max_ops, np = (rem + mo - 1) / mo;
            nr = (rem + np - 1) / np;
        }
        const int u1 = std::min((t + nr) * per_op, m);
        // residuals in the pass's last operand; if they end within its first 16 columns the second fragment is left out
        passes.push_back({t * per_op, u1, t, nr, dm.lay16 && tn.half && (u1 - (t + nr - 1) * per_op) * dm.slots <= 16});
        t += nr;
    }
    return passes;
}

int xtv_device(const mih_mat *h, XtvWork &w, const double *r_dev, int m, double *out_dev, hipStream_t s)
{
    const XtvTune &tn = w.tune;
    if (h->kind == 1) return xtv_dense_device(h, w, r_dev, m, out_dev, s);
    if (m > w.m_cap) { set_error("X'r workspace too small"); return MIH_BAD_ARG; }
    int splits = probe_splits(tn);
    const bool own_splits = splits > 0;
    if (splits <= 0) splits = auto_splits(h, tn);
    DigitMode dm = (w.use_alt && w.has_alt) ? w.dm_alt : w.dm;
    dm.lay16 = xtv_lay16(dm, tn);
    splits = pass_splits(h, splits, dm, w.splits_cap);
    if (splits < 0) { set_error("n = %lld rows needs more than %d row slices for exact accumulation", (long long)h->n, w.splits_cap); return MIH_BAD_DIM; }
    // the score image serves this call if the workspace pinned one and the pass is the library-default single-residual one on the
    // image's own row slices (otherwise the bits would differ)
    const ScoreImage *img = (w.img && m == 1 && dm.base == 4 && !own_splits && splits == w.img->splits) ? w.img.get() : nullptr;
    if (img) dm.hom_u = w.hom_u.p;
    const int64_t nblk = h->nbp * 2, pstride = h->ncg * 32;
    double *part = w.scal.p + w.rhs_cap * 4;
    dm.gate = w.gate; dm.gate_val = w.gate_val;
    if (!w.stats_done) launch_r_stats(r_dev, h->n, m, part, w.stat_done.p, dm.ebits, w.scal.p, w.gate, w.gate_val, w.peel.p, s);
    uint4 *dig_all = reinterpret_cast<uint4 *>(w.digits.p);
    uint2 *dig2_all = reinterpret_cast<uint2 *>(w.digits.p + (size_t)w.ops_cap * (size_t)nblk * 64 * 4);   // FP6 only
    const std::vector<XtvPass> passes = plan_passes(dm, tn, m);
    FlatPasses fp{};          // flat packing: pass q scores residuals u0[q] .. u0[q+1] from the operands t0[q] .. t0[q+1]
    if (dm.flat) {
        fp.npass = (int)passes.size();
        for (int q = 0; q < fp.npass; ++q) { fp.u0[q] = passes[q].u0; fp.t0[q] = passes[q].t; }
        fp.u0[fp.npass] = passes.back().u1; fp.t0[fp.npass] = passes.back().t + passes.back().nr;
    }
    // INVARIANT of the flat packing: k_digits writes only the digit columns of THIS call's m residuals; the unused tail
    // columns of a pass's last operand keep whatever an earlier call with another m left there.  That is harmless because (1) the
    // columns of the MFMA's B operand are independent -- a stale column only produces accumulator columns nobody reads -- and
    // (2) xtv_epilogue16_flat stops at j >= nres.  The lock-step lanes exercise exactly this in every cross-validation (one workspace,
    // a falling residual count from round to round, every loss checked by the tests of the full configs[3] grid),
    // and test_flat_packing_ignores_what_an_earlier_pass_left_in_the_tail_columns runs 19 residuals and then 1 .. 18 on ONE workspace.
    launch_digits(r_dev, h->n, nblk, m, dm.flat ? m : (m + dm.per_op - 1) / dm.per_op * dm.per_op, dm, w.scal.p, dig_all, dig2_all, fp,
                  (w.stats_done && m == 1) ? w.shook : XtvStatsHook(), w.peel.p, s);
    const bool hooked = !dm.flat && w.hook.cur != nullptr && m == 1;       // (device-resident steps: the support's extra workgroups)
    for (const XtvPass &ps : passes) {
        DigitMode dq = dm;
        dq.nres = dm.flat ? ps.u1 - ps.u0 : 0;
        double *partial = w.partial.p + (int64_t)ps.u0 * splits * pstride;
        PassRecord rec;
        const bool prof = prof_begin(h, s, rec);
        int rc = MIH_OK;
        if (img && ps.nr == 1) launch_xtv_image(*img, w, h, dig_all, dig2_all, nblk * 64, splits, dq, w.scal.p, partial, s, rec.kernel);
        else rc = dispatch_xtv(tn, ps.nr, ps.half, h, dig_all + (int64_t)ps.t * nblk * 64, dig2_all + (int64_t)ps.t * nblk * 64, nblk * 64,
                               splits, dq, w.scal.p + 4 * ps.u0, partial, s, rec.kernel);
        if (prof) {
            rec.residuals = ps.u1 - ps.u0; rec.operands = ps.nr; rec.stream_tag = w.stream_tag;
            prof_end(h, s, rec);
        }
        if (rc) return rc;
        hipLaunchKernelGGL(k_xtv_finalize, dim3((unsigned)((h->p + 255) / 256 + (hooked ? w.hook.blocks : 0))), dim3(256), 0, s,
                           partial, splits, pstride, h->p, ps.u1 - ps.u0, w.scal.p + 4 * ps.u0, r_dev + (int64_t)ps.u0 * h->n, h->n, h->mu, h->sinv,
                           h->miss_ptr, h->miss_row, w.raw ? 0 : h->center, w.raw ? 0 : h->scale, !w.raw && h->impute && h->total_missing > 0, out_dev + (int64_t)ps.u0 * h->p,
                           w.gate, w.gate_val, hooked ? w.hook : XtvSupportHook(), w.peel.p + (int64_t)ps.u0 * kPeelStride, h->X, h->nbp);
    }
    MIH_HIP(hipGetLastError());
    return MIH_OK;
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_xtv_algorithmic_bytes(const mih_mat *h, int m, double *bytes)
{
    if (!h || !bytes || m < 1) return MIH_BAD_ARG;
    if (h->kind == 0)
        *bytes = (double)h->p * (double)((h->n + 3) / 4) + 8.0 * m * ((double)h->n + (double)h->p) + 16.0 * (double)h->p;
    else
        *bytes = (h->Du ? 2.0 : h->Df ? 4.0 : 8.0) * (double)h->n * (double)h->p + 8.0 * m * ((double)h->n + (double)h->p);
    return MIH_OK;
}

int mih_xtv_batched_fmt(const mih_mat *h, const double *R, int m, int digits, double *OUT)
{
    if (!h || !R || !OUT || m < 1) { set_error("null/invalid argument"); return MIH_BAD_ARG; }
    MIH_HIP(hipSetDevice(h->device));
    XtvWork w;
    MIH_TRY(xtv_work_init(h, w, m, xtv_tune(digits)));
    DevBuf<double> r, out;
    MIH_TRY(r.alloc((size_t)m * h->n));
    MIH_TRY(out.alloc((size_t)m * h->p));
    MIH_HIP(hipMemcpyAsync(r.p, R, sizeof(double) * (size_t)m * h->n, hipMemcpyHostToDevice, h->stream));
    MIH_TRY(xtv_device(h, w, r.p, m, out.p, h->stream));
    MIH_HIP(hipMemcpyAsync(OUT, out.p, sizeof(double) * (size_t)m * h->p, hipMemcpyDeviceToHost, h->stream));
    MIH_HIP(hipStreamSynchronize(h->stream));
    xtv_count_peels(h, w, h->stream);
    return MIH_OK;
}

int mih_xtv_batched(const mih_mat *h, const double *R, int m, double *OUT)
{
    return mih_xtv_batched_fmt(h, R, m, 0, OUT);
}

int mih_xtv(const mih_mat *h, const double *r, double *out)
{
    return mih_xtv_batched_fmt(h, r, 1, 0, out);
}

#ifdef MIH_PROBES
// include/mendeliht_hip_probes.h: a sequence of residual counts on ONE fused-pass workspace (what a lock-step lane does)
int mih_probe_xtv_sequence(const mih_mat *h, const double *R, int mcap, const int *ms, int nms, int digits, double *OUT)
{
    if (!h || !R || !ms || !OUT || mcap < 1 || nms < 1) { set_error("null/invalid argument"); return MIH_BAD_ARG; }
    for (int i = 0; i < nms; ++i) if (ms[i] < 1 || ms[i] > mcap) { set_error("ms[%d] = %d outside 1..%d", i, ms[i], mcap); return MIH_BAD_ARG; }
    MIH_HIP(hipSetDevice(h->device));
    XtvWork w;
    MIH_TRY(xtv_work_init(h, w, mcap, xtv_tune(digits)));
    DevBuf<double> r, out;
    MIH_TRY(r.alloc((size_t)mcap * h->n));
    MIH_TRY(out.alloc((size_t)mcap * h->p));
    MIH_HIP(hipMemcpyAsync(r.p, R, sizeof(double) * (size_t)mcap * h->n, hipMemcpyHostToDevice, h->stream));
    size_t off = 0;
    for (int i = 0; i < nms; ++i) {
        MIH_TRY(xtv_device(h, w, r.p, ms[i], out.p, h->stream));
        MIH_HIP(hipMemcpyAsync(OUT + off, out.p, sizeof(double) * (size_t)ms[i] * h->p, hipMemcpyDeviceToHost, h->stream));
        MIH_HIP(hipStreamSynchronize(h->stream));
        off += (size_t)ms[i] * h->p;
    }
    return MIH_OK;
}
#endif

__global__ void k_fill_random(double *r, int64_t n, uint64_t seed)
{
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t a = (uint32_t)i * 0x9E3779B1u ^ (uint32_t)seed;
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
    uint32_t b = a * 0x85EBCA77u; b ^= b >> 13;
    r[i] = ((a & 0xFFFF) + (a >> 16) + (b & 0xFFFF) + (b >> 16)) * (1.0 / 65536.0) - 2.0;
}

__global__ void k_checksum(const double *x, int64_t p, double *out)
{
    __shared__ double red[256];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < p; i += 256) a += x[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k]; __syncthreads(); }
    if (threadIdx.x == 0) *out = red[0];
}

int mih_bench_xtv(const mih_mat *h, int digits, int m, int iters, int warmup, uint64_t seed, float *ms_per_pass, double *checksum)
{
    if (!h || iters < 1 || !ms_per_pass || m < 1) return MIH_BAD_ARG;
    MIH_HIP(hipSetDevice(h->device));
    XtvWork w;
    MIH_TRY(xtv_work_init(h, w, m, xtv_tune(digits), m > 1));       // m = 1: the single-fit workspace, like IhtVar
    DevBuf<double> r, out, cs;
    MIH_TRY(r.alloc((size_t)h->n * m));
    MIH_TRY(out.alloc((size_t)h->p * m));
    MIH_TRY(cs.alloc(1));
    hipStream_t s = h->stream;
    int rc = MIH_OK;
    hipLaunchKernelGGL(k_fill_random, dim3((unsigned)((h->n * m + 255) / 256)), dim3(256), 0, s, r.p, h->n * m, seed);
    for (int i = 0; i < warmup && !rc; ++i) rc = xtv_device(h, w, r.p, m, out.p, s);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters && !rc; ++i) rc = xtv_device(h, w, r.p, m, out.p, s);
    (void)hipEventRecord(e1, s);
    hipError_t e = hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "bench sync", __FILE__, __LINE__);
    *ms_per_pass = ms / iters;
    if (checksum) {
        hipLaunchKernelGGL(k_checksum, dim3(1), dim3(256), 0, s, out.p, h->p * m, cs.p);
        MIH_HIP(hipMemcpyAsync(checksum, cs.p, sizeof(double), hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));
    }
    return MIH_OK;
}

}  // extern "C"
