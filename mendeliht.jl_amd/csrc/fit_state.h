// fit_state.h -- the declaration of one IHTVariable on the device (src/data_structures.jl:4-43): what it holds and the member functions
// fit.hip (fit_iht!, sessions) and fit_lockstep.hip (cv_iht, model paths) drive it with.  The definitions, and every kernel a step
// of the variable runs, are compiled once, in iht_var.hip.
#pragma once
#include "common.h"
#include "fit_common.h"
#include <map>
#include <memory>
#include <vector>

namespace mih {

constexpr int kMaxQ = 64;
struct QVec { double v[kMaxQ]; };

// ---- what a device-resident step (resident.inc) keeps on the device and hands to its kernels ----
constexpr int kResMaxAttempts = 8;        // attempts of a step the direct gather keeps a forecast for (later ones: histograms)
struct ResModel { int64_t cnt; uint64_t idc; double c[kMaxQ]; };
struct ResCtl {
    int32_t live_epoch;       // kernels launched with another epoch do nothing
    int32_t cur;              // model buffer of the current iterate (b at the start of a step, b0 while it runs); 1 - cur: candidate
    int32_t es;               // backtracks of the running step so far
    int32_t iter;             // steps completed (fit.jl's iteration counter)
    int32_t arm_stop, min_iter, max_step, pad0;
    int32_t nfresh[2];        // per model buffer: entries whose column is not in the cache yet
    uint32_t ctr[6];          // last-block counters (left at zero)
    double eta;               // step size of the running step before any halving
    double logl_cur, best_logl, tol, tol_stop;
    double df2[kMaxQ];        // Z'r of the last score
    uint64_t topk[4];         // two-pass select: exponent bin, remaining rank, lower-bound key, 22-bit prefix
    uint64_t thr_key[kResMaxAttempts];   // |K-th largest| of the last projection made as attempt a of a step, as a key (0: unknown), and
    double thr_eta[kResMaxAttempts];     // the step size it was made with: the direct gather's forecast for the next attempt a
    ResModel m[2], best;
    // column-sharded fit: the WHOLE model of each iterate as (global index, value) lists (check_convergence and _choose!'s count are
    // global), the shard's own candidates of the running projection
    int64_t gcnt[2], lc_cnt;
};
struct ResRecord { double logl, tol, eta; int32_t status, nbt, iter, cur; int64_t support; uint64_t seq; };      // seq is stored last
struct ResPtrs {
    ResCtl *ctl;
    int64_t *idx[3]; double *val[3];          // [0], [1]: the two iterates; [2]: the best model
    int32_t *slot[2], *fresh[2];              // cache slot of every entry; positions of the entries still to be copied in
    double *gval, *coefA, *coefB;             // df on the support; k_xv_coef's coefficients of the list about to be multiplied
    uint32_t *hist;                           // 2 x 2048 bins
    uint64_t *sel; uint32_t sel_cap;          // candidates of the select: sel[0] = count, pairs behind sel[2]
    int64_t kcap;                             // entries the lists hold
    ResRecord *rec;                           // pinned ring
    uint64_t *big;                            // k_res_select<BIG>'s scratch (kResBigScratchWords), or null
    // column-sharded fit (null / 0 otherwise)
    int64_t *gidx[2]; double *gvals[2];       // the whole model of the two iterates, global indices
    int64_t *lc_idx; double *lc_val;          // this shard's survivors of its own top-K (k_res_select_local)
    double *msg, *msgs;                       // this shard's message of the projection's all-gather, and everybody's
    int32_t world, rank; int64_t col0;
};
struct ResMat {                               // what the kernels need of the 2-bit matrix and its column cache
    const uint32_t *X; int64_t nbp, ndw, n, p;
    uint32_t *cache; int32_t slots;
    const double *mu, *sinv; int center, scale;
    const int64_t *miss_ptr; const int32_t *miss_row;
};
// a run of resident steps as its driver sees it (IhtVar::res_next): never past `limit` steps in all
struct ResRun { int64_t limit = 0, issued = 0, done = 0; int max_step = 3; };

// initialize_beta! results shared by the fits of a lock-step lane: the p univariate regressions depend on the training rows only
// (the fold), not on the model size, so the first fit of a fold computes them (two extra passes over X) and the other fits of
// that fold in the lane take them from here.  One lane = one host thread: no locking; a fit that finds an entry still being
// computed by another coroutine of its lane yields until it is ready.
struct IbShared {
    struct Entry { int state = 0; DevBuf<double> beta; std::vector<double> c; };      // state 1: being computed, 2: ready
    std::map<int, std::unique_ptr<Entry>> by_key;
};

// One IHTVariable (src/data_structures.jl:4-43), device-resident.  The base carries the column shard: comm, col0, pg.
struct IhtVar : ShardComm {
    // ---- configuration (create) ----
    std::shared_ptr<DevPool> reserve;             // very first member: the matrix's reserve outlives this variable's blocks
    Arena arena;                                  // the memory outlives every buffer carved out of it
    const mih_mat *h = nullptr;
    int64_t n = 0, p = 0; int q = 0;
    int64_t k = 0, J = 1; std::vector<int64_t> ks;
    int dist = 0, link = 0, est_r = 0; double nb_r = 1.0;
    std::vector<uint8_t> zkeep; int64_t zkeepn = 0;
    const double *y_host = nullptr, *z_host = nullptr;
    int init_beta = 0, debias = 0;
    bool long_lived = false;   // a session (set before create): its set-up may build the matrix's score image (score_image_auto)
    int (*choose_cb)(void *, int32_t, const int64_t *, int64_t, int64_t, int64_t *) = nullptr;   // mih_fit_params::choose
    void *choose_user = nullptr;
    XtvTune tune;                 // how this fit's X'r passes run (mih_fit_params::xtv_digits)
    hipStream_t s = nullptr;
    bool own_stream = true;
    bool has_weight = false, has_group = false;
    int64_t G = 0;                // groups: the largest label anywhere

    // ---- device buffers ----
    DevBuf<double> y, z, w, xb, zc, mu, r, xgk, df, full, weight, red, scal, gval, ztr;
    DevBuf<unsigned> ztr_done;
    DevBuf<uint8_t> mask;
    DevBuf<int64_t> group_dev, kgrp_dev;
    XtvWork xtv; XvWork xv; TopkWork topk;
    int nb = 0;                                   // row blocks

    // ---- host model ----
    Sparse b, b0, best_b, idx;                    // idx.val = df on the support
    std::vector<uint8_t> idc, idc0;
    std::vector<double> c, c0, best_c, df2;
    int64_t ntrain = 0;
    bool choose_fired = false;
    const uint8_t *train_cur = nullptr;
    // the step size of the NEXT step, computed speculatively at the end of a step (step_post_fused): the denominator, for which support
    bool spec_ok = false; double spec_denom = 0.0, spec_numer_snp = 0.0; std::vector<int64_t> spec_idx; std::vector<uint8_t> spec_idc;
    // initialize_beta! results of the last training mask (reused across the k of one CV fold)
    DevBuf<double> ib_beta; std::vector<double> ib_c; std::vector<uint8_t> ib_train; bool ib_valid = false;

    // ---- column shard (comm, col0, pg: ShardComm) ----
    // the WHOLE k-sparse model of the step and of the step before, global column indices, identical on every rank
    // (project_full_sharded); *_ok = false: incomplete, the step falls back to the collectives
    Sparse bg, b0g; bool bg_ok = false, b0g_ok = false;
    std::vector<int64_t> group_host;             // the local columns' labels, for the candidates' messages

    // ---- lock-step lane (mih_cv_iht; create's shared_stream / fit_stream) ----
    bool batched = false;                        // one of a lock-step batch: runs on the batch's stream and leaves the X'r pass to the batch driver
    hipEvent_t ev = nullptr;                     // orders a fit that has a stream of its own against the lane's stream around the fused pass
    // a lock-step lane's cache of the regressions, keyed by the fit's training rows (fold); null outside the lock-step drivers
    IbShared *ib_shared = nullptr; int ib_key = -1;
    // sum of y over the training rows and their count, in the order of init_pre's own loop, when the caller has them already
    // (cv_iht computes them once per fold instead of once per (fold, k) fit: two sweeps over n on the host per fit otherwise)
    bool train_sums_valid = false; int64_t train_count = 0; double train_ysum = 0.0;
    uint64_t lane_seq = 0; bool lane_queued = false;      // the step chain queued behind the lane's pass (lane_queue_step)

    // ---- staging and readback ----
    DevBuf<int64_t> sidx; DevBuf<double> sval;   // staging for support lists
    // the pinned ring new lists go through, and what sidx / sval hold on the device: a list that is already there is not sent again
    HostStage stage;
    std::vector<int64_t> dev_idx; std::vector<double> dev_val; bool dev_idx_ok = false, dev_val_ok = false;
    PinBuf<double> hpin;                          // pinned landing area of the small readbacks
    SpinFlag flag;                                // `count` doubles of a device buffer into hpin[0..count) without a stream synchronisation (readback)
    bool df2_pending = false;                     // df2 has landed in pinned memory; copied out at the next synchronisation (take_df2)

    // ---- iht_one_step! resident on the device (resident.inc) ----
    // The host-driven members stay the library's statement of the step (and serve every fit the resident chain does not: callback
    // communicators, groups, est_r, debias, dense matrices); a fit that qualifies runs its steps through res_next().  Between
    // res_begin() and res_end() the iterate lives on the device only.
    bool res_ok = false, res_active = false, res_zero_list = false;
    bool res_eligible = false;           // what res_setup found; res_ok falls to false when a res_begin declines (lists beyond the buffers) and comes back with the next fit on this variable (init_pre)
    int res_epoch = 0; uint64_t res_seq = 0; int64_t res_kcap = 0, res_iter0 = 0;
    std::vector<uint64_t> res_out;                       // sequence numbers of the steps in flight, oldest first
    DevBuf<ResCtl> rctl; DevBuf<int64_t> ridx; DevBuf<double> rval; DevBuf<int32_t> rslot; DevBuf<uint32_t> rhist; DevBuf<uint64_t> rsel; DevBuf<double> rwalk; DevBuf<uint32_t> rtick;
    bool res_big = false; DevBuf<uint64_t> rbig;            // a model beyond kResMaxList entries: k_res_select_big and its scratch
    bool res_sharded = false; DevBuf<int64_t> rgidx; DevBuf<double> rgval, rmsg; PinBuf<double> rg_h;        // column shard: whole models, messages
    int64_t rg_cnt_h[2] = {0, 0};
    PinBuf<ResCtl> rctl_h; PinBuf<ResRecord> rrec; PinBuf<int64_t> ridx_h; PinBuf<double> rval_h; PinBuf<int32_t> rslot_h;
    // the attempt slots of a series (res_enqueue_attempts): the forecast, the direct gather's failures, the backtracks of the last three steps
    int res_spec = 0, res_fast_fails = 0, res_known = 0, res_last[3] = {0, 0, 0};
    static constexpr int kResSpecCap = 2;           // slots per series beyond the first

    // ---- member functions (iht_var.hip) ----
    int debias_sharded();
    int create(const mih_mat *hh, const mih_fit_params *prm, const double *yh, const double *zh, int64_t qq,
               hipStream_t shared_stream = nullptr, double *y_shared = nullptr, double *z_shared = nullptr, hipStream_t fit_stream = nullptr);
    ~IhtVar();
    // v.k = sparsity (cross_validation.jl:110): with groups and a scalar k the projection reads k from the device
    int set_k(int64_t knew);
    int ensure_stage(int64_t nnz);
    void stage_forget() { dev_idx_ok = dev_val_ok = false; }
    int upload(const std::vector<int64_t> &ix, const std::vector<double> &vl);
    int upload_idx(const std::vector<int64_t> &ix);        // sidx only; sval keeps its content only if the list is unchanged
    QVec qvec(const std::vector<double> &v) const { QVec o; for (int l = 0; l < kMaxQ; ++l) o.v[l] = l < q ? v[l] : 0.0; return o; }
    int set_weights(const uint8_t *m, int invert);        // cv_wts from a train mask
    // update_xb! (utilities.jl:93-118)
    int update_xb();
    // update_mu! + loglikelihood; returns logl and the raw deviance
    int mu_loglik(int with_zc, double *logl, double *dev);
    // score! (utilities.jl:126-135) + df[idx] gather for the next step size
    int score();
    // xtv_digits = -1 in a lock-step driver: does the residual just formed qualify for the 43-bit format?  (GLM links only: the
    // reference's tolerance for them is 1e-4, north_star; Normal / Identity fits keep the 54-bit format.)
    bool auto_digits() const { return batched && tune.digits == -1 && dist != MIH_NORMAL; }
    int residual_rides_43_bits(bool *yes);
    int resid_only();
    int score_post();        // df is in place (own X'r pass or the batch driver's)
    int readback(const double *src_dev, size_t count);
    // the second stage of a block reduction (nv sums over the nb rows of `red`) and the way home of `count` doubles in ONE kernel
    int final_sum_home(int nv, double *out_dev, const double *src_dev, size_t count);
    void take_df2() { if (df2_pending) { for (int l = 0; l < q; ++l) df2[l] = hpin.p[hpin.n - kMaxQ + l]; df2_pending = false; } }
    int gather_df_support();
    // the caller draws, as the reference does: `for pos in sample(non_zero_idx, excess, replace=false)` (utilities.jl:453-456)
    int choose_by_caller(Sparse &sp, int64_t excess, bool with_values = true);
    int choose();
    // project the (p+q) buffer `full` to k+zkeepn and split the survivors into (SNP list, covariate values)
    int project_full(Sparse &snp, std::vector<double> &ctail, std::vector<uint8_t> &ctail_nz, bool zero_in_place = true);
    int project_full_sharded(Sparse &snp, std::vector<double> &ctail, std::vector<uint8_t> &ctail_nz);
    int group_project_sharded(double *y_dev, Sparse &mine);
    // _iht_gradstep! (utilities.jl:252-280) from base model (bb, cc) with step eta
    int gradstep(const Sparse &bb, const std::vector<double> &cc, double eta);
    // init_iht_indices! (utilities.jl:366-438), init_beta=false
    int init(const uint8_t *train);
    int init_pre(const uint8_t *train);
    int init_beta_phase(const uint8_t *train);
    int init_post();
    // iht_stepsize! (utilities.jl:722-764)
    int stepsize(double *eta);
    double save_prev(double cur, double best);        // utilities.jl:702-712
    int save_best_model();        // utilities.jl:995-1006
    double check_convergence();        // utilities.jl:953-957
    int nb_sums(int which, double rr, double *out2);
    int mle_for_r();
    // iht_one_step! (fit.jl:213-263)
    int one_step(double old_logl, int nstep, int *bt, double *new_logl);
    // everything of iht_one_step! before the X'r pass (ends with the working residual in r)
    int step_pre(double old_logl, int nstep, int *bt, double *new_logl);
    int step_post_fused();
    int step_post(double logl);
    int res_setup(const mih_fit_params *prm, int64_t kcap);
    ResPtrs res_ptrs() const;
    ResMat res_mat() const;
    // k_res_xgk / k_res_xb: workgroups of 1024 rows (64 dwords of every cached column), 68 KB of dynamic LDS
    unsigned res_wide_blocks() const { return (unsigned)((h->n_pad / 16 + 63) / 64); }
    uint64_t res_zkeep_mask() const { uint64_t m = 0; for (int l = 0; l < q; ++l) if (zkeep[l]) m |= 1ull << l; return m; }
    bool res_fix() const { return h->impute && h->total_missing > 0; }
    // Normal / identity on the plain (unsharded, no imputed entries) path: the attempts do not store xb, zc, mu (k_res_xb's `lean`);
    // res_end forms them again from the model that comes home
    bool res_lean() const { return !res_sharded && !res_fix() && dist == MIH_NORMAL && link == MIH_IDENTITY; }
    void xv_cache_forget();        // the host's map of the column cache no longer describes it (the device kept the books), or vice versa
    // the host-side iterate -> the device.  next_logl / best: the loglikelihoods fit_iht! carries (fit.jl:163-164)
    int res_begin(double next_logl, double best, int64_t iter_done, int arm_stop, const mih_fit_params *prm);
    int res_end(double *next_logl, double *best, bool handback = false);
    void res_dead_passes(int count);
    // ... of the series `behind` places before the last one queued (a series that ended without a step: its pass found phase 1)
    void res_dead_pass_at(int behind);
    int res_enqueue_support();
    int res_enqueue_front();
    int res_enqueue_attempt(uint64_t seq, int a, bool more, bool fast);
    // the shards' messages of the projection (k_res_select_local -> k_res_select_global): one ncclAllGather queued on this stream
    int res_allgather_messages(int64_t mlen);
    int res_enqueue_attempts(uint64_t seq, int a0, int max_step, bool first_slow = false);
    int res_enqueue_back();
    int res_wait(uint64_t seq, ResRecord *out);
    int res_take(const ResRecord &rec, double *next_logl, double *best, int *nbt, double *tol, bool *stepped);
    int res_next(ResRun &rr, double *next_logl, double *best, int *nbt, double *tol, bool *stepped);
    int lane_queue_step(double next_logl, double best, int64_t iter_done, const mih_fit_params *prm);
    int lane_collect_step(const mih_fit_params *prm, double *next_logl, double *best, int *nbt, double *tol, bool *stepped);
    // fit_iht! (fit.jl:145-207)
    int fit_loop(const mih_fit_params *prm, double *best_out, int64_t *iter_out, double *lt, double *tt,
                 int32_t *btt, int32_t *ntrace);
};

int check_params(const mih_mat *h, const mih_fit_params *prm, int64_t q);

}  // namespace mih
