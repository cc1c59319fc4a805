/*
 * mendeliht_hip_probes.h -- extra entry points of the MEASUREMENT build (libmendeliht_hip_probes.so = the product's
 * sources compiled with -DMIH_PROBES).  Not part of the drop-in boundary and not exported by libmendeliht_hip.so:
 * tools/ and the "this switch changes nothing" tests use them to sweep launch shapes, to cross-check the product's
 * kernels bit for bit against the round-1 kernel families, to run timing probes, and to drive sequences of calls on ONE
 * workspace (mih_probe_xtv_sequence: fused X'r passes; mih_probe_xv_sequence: the cached and multi-trait X beta paths of a
 * fit), to run the GLM refit of debias! on its own (mih_probe_debias_glm) and the initialize_beta! regressions on their own
 * (mih_probe_init_beta).  The measurement build also reads
 * the MENDELIHT_* A/B environment switches (XTV_MAX_OPS, XTV_SLICES, XTV_NO_HALF, CV_LANES, CV_NO_MERGE,
 * CV_NO_INIT_SHARE, CV_NO_COOP, COOP_SPIN_US, CV_TRACE, INGEST_TRACE, INGEST_THREADS, TRACE_ETA, NO_SPIN, NO_ARENA, NO_RESERVE,
 * NO_RESIDENT, TOPK_RADIX8, XV_MULTI, RES_FORCE_ABORT_ES, DEBIAS_TRACE = the IRLS iterates of debias!'s GLM refit on stderr); the
 * product reads none
 * of them.
 * These knobs are process-wide on purpose (one measurement at a time).
 */
#ifndef MENDELIHT_HIP_PROBES_H
#define MENDELIHT_HIP_PROBES_H
#include "mendeliht_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* single-operand X'r kernel of every subsequent call: -1 = product default, 0..15 = round 1's per-wave-load shapes */
int mih_probe_set_xtv_variant(int variant);
/* launch shape of the LDS-shared / ring kernels: 0 = product defaults; 1..15 = round-1 register-staged shapes (6 / 9: its
 * defaults); 20.. = 32x32x64 ring shapes; 40.. = 16x16x128 ring shapes; 7, 8, 15, 30..33, 49 = timing probes whose output
 * is NOT X'r */
int mih_probe_set_xtv_multi_variant(int variant);
/* B operands fused per pass of the register-staged kernels (1, 2 or 4) */
int mih_probe_set_max_fused(int max_nr);
/* X'r of the first ms[i] columns of R (n x mcap, column-major) for i = 0 .. nms-1, one call after the other on ONE fused-pass
 * workspace sized for mcap residuals -- what a lock-step lane does from round to round.  OUT: the results back to back
 * (p * ms[0] doubles, then p * ms[1], ...).  For the test that a pass ignores what an earlier pass with another residual
 * count left in the unused digit columns of its last operand (flat packing: plan_passes in csrc/xtv.hip, xtv_epilogue16_flat in csrc/xtv_kernels.h). */
int mih_probe_xtv_sequence(const mih_mat *h, const double *R, int mcap, const int *ms, int nms, int digits, double *OUT);
/* X beta over a small support, ncalls products one after the other on ONE workspace (xv_work_init(h, w, max_nnz, cache_nnz):
 * its LRU column cache, its coefficient buffers) with ONE pinned upload ring sized as a fit sizes it -- the paths a fit takes
 * from step to step, which mih_xv_sparse (fresh workspace, direct kernel) never does.  Call c has nnz[c] column indices and
 * m[c] * nnz[c] coefficients (trait-major), concatenated over the calls in idx_cat / val_cat.  m[c] == 1: the single-vector
 * product with the host's copy of the indices (column cache; the direct kernel when the support outgrows it); flags[c] bit 0:
 * slot and fill lists through the pinned ring, bit 1: the coefficients are gathered from a length-p vector the entry
 * scatters them into (later duplicates of an index win) and also returned in GATHERED at the call's place in val_cat's
 * layout, bit 2: clamp to [-20, 20].  m[c] > 1 (flags[c] must be 0): the multi-trait product (MENDELIHT_XV_MULTI selects its
 * kernel).  OUT: the results back to back, m[c] * n doubles per call.  GATHERED may be null when no call gathers.  The stream
 * is not synchronised between the calls. */
int mih_probe_xv_sequence(const mih_mat *h, int64_t max_nnz, int64_t cache_nnz, int ncalls, const int64_t *nnz, const int *m,
                          const int *flags, const int64_t *idx_cat, const double *val_cat, double *OUT, double *GATHERED);
/* The GLM refit of debias! (csrc/debias.hip: debias_glm_device) on its own, unsharded, on the matrix's stream: y (n doubles on the
 * host) is refitted on the k columns idx[0 .. k) (1 <= k <= p, each in [0, p)) with distribution dist, link `link` and the NegBin r
 * nb_r; BETA receives the k coefficients in the order of idx.  GRAM0, W0, T0 (each may be null) receive what the FIRST solve
 * consumed: the (k+1) x (k+1) reduced Gram, column-major, upper triangle valid, X'W t in its last column and t'W t in its corner;
 * the n working weights and the n working responses eta + wrkresid at mustart(y).  They are filled as soon as that Gram is on the
 * host, so they are valid when the call fails in the Cholesky solve or later.  IRLS_ITERS (may be null): the iterations after the
 * first solve.  The refit's own errors (ProbitLink, X'WX not positive definite, step halving, no convergence) come back as they do
 * from a fit. */
int mih_probe_debias_glm(const mih_mat *h, const int64_t *idx, int64_t k, const double *y, int dist, int link, double nb_r,
                         double *beta, double *gram0, double *w0, double *t0, int32_t *irls_iters);
/* The p univariate regressions y_t ~ 1 + x_j of initialize_beta! (csrc/iht_var.hip: init_beta_regress_device, what every fit with
 * init_beta calls) on their own, on the matrix's stream, for m traits (1 <= m <= 32): w (n doubles on the host, each 0.0 = held out
 * or 1.0 = training row) and Y (n x m, column-major) are uploaded; N and Sy[t] = sum of Y[., t] over the training rows are summed
 * on the host in row order as a fit sums them.  BETA (m x p, plane t = trait t): the slopes clamped to [-2, 2].  The other outputs
 * (each may be null) are the intermediates: S ((1 + m) x p: row 0 = sum_train x_j, row 1 + t = sum_train x_j y_t, the fused X'R
 * pass), CNT (2p, 2-bit handles only, ignored otherwise: CNT[2j + k] = training rows of column j with dosage k + 1), SXX (p, dense
 * and dosage handles only, ignored for 2-bit ones: sum_train x_j^2), ICPT (m x p: the intercepts, or the unsolved sum y where
 * N sxx - sx^2 is not positive) and ICPT_SUM (m: the device's sum of each ICPT plane).  MIH_BAD_ARG, before any launch and with no
 * output written, for a null h, w, Y or beta, m outside 1..32, a w entry that is neither 0 nor 1, no training row, a non-finite Y. */
int mih_probe_init_beta(const mih_mat *h, const double *w, const double *Y, int m, double *S, int32_t *cnt, double *sxx,
                        double *beta, double *icpt, double *icpt_sum);
#ifdef __cplusplus
}
#endif
#endif
