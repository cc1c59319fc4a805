// resident.inc -- iht_one_step! (src/fit.jl:213-263) resident on the device.  Included by iht_var.hip inside namespace mih; the control
// block, the step record and the argument structs of its kernels (ResCtl, ResRecord, ResPtrs, ResMat) are declared in fit_state.h.
//
// The host-driven step of rounds 1-4 kept the k-sparse model (b, b0, best_b) as host lists, finished project_k! on the host and
// took the backtracking decision there: 26 launches and three host waits between two X'r passes.  Here the iterate, the top-k
// finish, the column-cache bookkeeping, the `old_logl > new_logl` decision of _iht_backtrack_ (utilities.jl:484) and the
// convergence test (fit.jl:197) live on the device; a step is a chain of kernels the host queues WITHOUT waiting -- it reads one
// small record per step from pinned memory, one step behind.  Every kernel of the chain is gated on ONE word, ctl->live_epoch =
// 2 * epoch + phase: a kernel runs only in the epoch it was launched for and in the phase it belongs to.  The host queues
//     [step start: X_S df_S, step size]  [attempt slot] x (1 + forecast)  [step end: residual, statistics, the X'r pass]  [step start] ...
// and the device decides what of it runs: phase 1 (opened by k_res_eta) lets the attempt slots run -- a slot does whichever attempt
// ctl->es says is due: gradient step, projection, update_xb!, loglikelihood, decision; the k_res_decide that lets a candidate
// stand flips the iterate and goes to phase 0, where the slots still queued do nothing and the step-end and step-start kernels run.
// A step that needs MORE attempts than slots were queued for it (the forecast is the last step's count: a fit near its optimum
// halves the step once in most iterations) simply stays in phase 1: the step-end kernels behind the series do nothing (the X'r pass
// among them), nor does the next step start, and the next series of slots goes on with the same step -- no host round trip, no
// work thrown away but a dozen empty launches.  The host reads one record per series (a step stood / still backtracking) and
// keeps two series queued ahead.  A fit that converged (when armed), a loglikelihood NaN / Inf, or a case the device does not
// handle (exact ties that need _choose!, survivor lists beyond the buffers, a direct gather whose forecast failed) moves the
// word to the next epoch: everything queued behind does nothing, the iterate stays as it was, and the host -- when it reads that
// record -- stops, re-queues the attempt with the histogram sweeps, or replays the step through the host-driven path.
//
// Arithmetic: every sum is formed exactly as the host-driven kernels form it (same 256-row blocks, same trees, the second-stage
// sums in k_final_sum's order, k_xv_snp_cached's column groups), so a fit gives the same bits on either path
// (tests/test_gpu_parity.py::test_resident_steps_equal_host_driven_steps).
//
//   reference                                                kernel
//   iht_stepsize! (utilities.jl:722-764)                     k_res_support, k_res_xgk (+ k_res_stepsize), k_res_eta
//   _iht_gradstep! + vectorize! (:252-280, 291-315)          k_res_grad
//   project_k! (:553-559)                                    k_res_grad (histogram 1), k_res_hist2, k_res_collect, k_res_select
//   unvectorize!, _choose! trigger (:317-354, 444-458)       k_res_select
//   update_xb!, update_mu!, loglikelihood (:93-118,74-82,9-20)  k_res_xb (+ k_res_mu)
//   _iht_backtrack_ / backtrack! (:484-486, 959-973)         k_res_decide (decision); the next attempt slot in the stream goes on
//   score! residual (:128-132)                               k_res_xb / k_res_mu (the candidate's, from the values at hand)
//   Z'r, the statistics of r (:134)                          k_res_stats (+ the second stages in k_digits); X'r = the gated pass of xtv.hip (k_digits: xtv_digits.hip)
//   save_prev! / check_convergence (:702-712, 953-957)       buffer flip in k_res_decide, best model in k_res_xgk, tol in k_res_select
// Serial tails (the second-stage sums with the step size, the decision) are one-workgroup kernels of their own, 2.5 us apiece;
// NO counter is shared by a whole grid: a last-block ticket over 1954 blocks cost 100 us (measured: same-address atomics at ~60 ns
// each, and behind every one a device-scope release that writes back the XCD's L2 -- see k_res_stats, whose tickets are four
// increments per address in a kernel that writes nothing else), and a grid barrier of a persistent kernel 16 - 60 us
// (tools/gridsync_probe.hip) -- which is why the chain is kernels and not one persistent kernel.

constexpr int kResRing = 8;               // step records in pinned host memory
constexpr int kResShardList = 1024;        // longest list the sharded select handles (its pool of candidates: kResMaxInBin)
constexpr int kResMaxList = 2048;         // longest survivor list k_res_select sorts in LDS
constexpr int kResBigList = 8192;         // ... and k_res_select<BIG> in a scratch block of device memory (round 6: models beyond ~2000 effects stay resident)
constexpr int kResBigScratchWords = 8 * kResBigList;      // 64-bit words of that block: s_idx, s_val, o_idx, o_val, t_idx, t_val, {fresh_t, o_slot}, {rank_of, -}
constexpr int kResMaxInBin = 2048;        // entries it ranks among themselves (those sharing the threshold's 22-bit prefix; all candidates of a direct gather)
enum { RES_ACCEPT = 0, RES_PENDING = 1, RES_STOP_CONVERGED = 2, RES_STOP_NAN = 3, RES_STOP_INF = 4, RES_ABORT = 5, RES_REDO_SLOW = 6 };

// The gate word: 2 * epoch + phase.  Phase 0 (between two attempts series): the kernels that end a step (residual, statistics, the
// X'r pass) and those that begin the next (X_S df_S, the step size) run; phase 1: the kernels of an attempt run -- whichever
// attempt ctl->es says it is.  k_res_eta opens phase 1, the k_res_decide that lets a candidate stand goes back to phase 0.  A
// kernel launched with attempt >= 0 belongs to an attempt slot, with attempt < 0 to a step's ends.
__host__ __device__ constexpr int res_gate_step(int epoch) { return 2 * epoch; }
__host__ __device__ constexpr int res_gate_attempt(int epoch) { return 2 * epoch + 1; }
__device__ __forceinline__ bool res_dead(const ResCtl *ctl, int epoch, int attempt)
{
    return ctl->live_epoch != (attempt >= 0 ? res_gate_attempt(epoch) : res_gate_step(epoch));
}

__device__ __forceinline__ uint64_t res_abs_key(double v) { return (uint64_t)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull; }

__device__ __forceinline__ uint64_t res_wave_min_u64(uint64_t v)
{
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint64_t o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ double res_wave_max(double v)
{
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
// k_final_sum's sums of the NV values of a row of partials, for one workgroup of 256 threads (one sweep, one tree; the same order of
// additions per value)
template <int NV>
__device__ __forceinline__ void res_final_sums(const double *__restrict__ partial, int nblocks, double (&out)[NV], double (*red)[256] /* [NV][256] */)
{
    double a[NV];
    #pragma unroll
    for (int k = 0; k < NV; ++k) a[k] = 0.0;
    // eight rows in flight, the last batch with rows switched off (the partials are cold: at 1954 blocks a thread that insisted
    // on whole batches of four was left with up to four round trips one after the other); the additions stay in block order
    for (int b = threadIdx.x; b < nblocks; b += 2048) {
        double v[8][NV];
        #pragma unroll
        for (int u = 0; u < 8; ++u)
            #pragma unroll
            for (int k = 0; k < NV; ++k) v[u][k] = (b + 256 * u < nblocks) ? partial[(int64_t)(b + 256 * u) * NV + k] : 0.0;
        #pragma unroll
        for (int u = 0; u < 8; ++u)
            if (b + 256 * u < nblocks) {
                #pragma unroll
                for (int k = 0; k < NV; ++k) a[k] += v[u][k];
            }
    }
    #pragma unroll
    for (int k = 0; k < NV; ++k) red[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            #pragma unroll
            for (int k = 0; k < NV; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    #pragma unroll
    for (int k = 0; k < NV; ++k) out[k] = red[k][0];
    __syncthreads();
}
// the step size after `es` halvings (utilities.jl:485 `η_g /= 2`: exact)
__device__ __forceinline__ double res_halved(double eta, int es) { for (int i = 0; i < es; ++i) eta /= 2; return eta; }

__device__ __forceinline__ void res_publish(ResRecord *ring, uint64_t seq, int status, double logl, double tol, double eta, int nbt, int iter,
                                            int cur, int64_t support)
{
    ResRecord *r = ring + (seq % kResRing);
    r->logl = logl; r->tol = tol; r->eta = eta; r->status = status; r->nbt = nbt; r->iter = iter; r->cur = cur; r->support = support;
    __threadfence_system();
    __hip_atomic_store(&r->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// df on the support of the current iterate and k_xv_coef's coefficients for X_S df_S (iht_stepsize!, utilities.jl:731-739)
__device__ __forceinline__ void
b_res_support(ResPtrs P, int epoch, ResMat M, const double *__restrict__ df)
{
    const ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, -1)) return;
    const int cur = ctl->cur;
    const int64_t cnt = ctl->m[cur].cnt;
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    if (t >= cnt) return;
    const int64_t j = P.idx[cur][t];
    const double v = df[j], a = (M.scale ? M.sinv[j] : 1.0) * v;
    P.gval[t] = v; P.coefA[t] = a; P.coefB[t] = M.center ? -M.mu[j] * a : 0.0;
}

// The block's 256 rows of X[:, S] * v over the cached copies of the support columns: k_xv_snp_cached's sums in its order.
// Columns that are not in the cache yet (fresh) are copied for this block's 16 dwords first; every block does that for its own
// rows, so the copy needs no launch of its own and the next product over the same list finds the columns in place.
// a word of the column cache, past this CU's vector cache (see res_xv_rows_wide: a column just copied in is read back without a fence)
__device__ __forceinline__ uint32_t res_ld_word(const uint32_t *q)
{
    return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double res_xv_rows(const ResMat &M, const int64_t *__restrict__ idx, const int32_t *__restrict__ slots,
                                              const int32_t *__restrict__ fresh, int nfresh, const double *__restrict__ A,
                                              const double *__restrict__ B, int64_t nnz, double (*part)[16][17])
{
    const int64_t ndw = M.ndw;
    if (nfresh > 0) {                                            // (uniform)
        const int64_t dwf = blockIdx.x * 16ll + (threadIdx.x & 15);
        if (dwf < ndw)
            for (int e = threadIdx.x >> 4; e < nfresh; e += 16) {
                const int t = fresh[e];
                M.cache[(int64_t)slots[t] * ndw + dwf] = M.X[xword(M.nbp, idx[t], dwf)];
            }
        __syncthreads();                                         // (no device-scope fence: see res_xv_rows_wide)
    }
    const int groups = (int)(nnz < 16 ? nnz : 16);
    const int g = threadIdx.x >> 4, d = threadIdx.x & 15;
    const int64_t dw = blockIdx.x * 16ll + d;
    const int64_t per = groups ? (nnz + groups - 1) / groups : 0;
    const int64_t t0 = g * per, t1 = (g < groups) ? (t0 + per < nnz ? t0 + per : nnz) : t0;
    double acc[16];
    #pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.0;
    double bsum = 0.0;
    if (dw < ndw) {
        int64_t t = t0;
        // four columns per batch; the words of the NEXT batch are requested before the multiply-adds of this one (the sums and
        // their order are k_xv_snp_cached's)
        uint32_t wn[4] = {0u, 0u, 0u, 0u}; double an[4] = {0.0, 0.0, 0.0, 0.0}, bn[4] = {0.0, 0.0, 0.0, 0.0};
        if (t + 4 <= t1) {
            #pragma unroll
            for (int u = 0; u < 4; ++u) { wn[u] = res_ld_word(M.cache + (int64_t)slots[t + u] * ndw + dw); an[u] = A[t + u]; bn[u] = B[t + u]; }
        }
        for (; t + 4 <= t1; t += 4) {
            uint32_t w4[4]; double a4[4];
            #pragma unroll
            for (int u = 0; u < 4; ++u) { w4[u] = wn[u]; a4[u] = an[u]; bsum += bn[u]; }
            if (t + 8 <= t1) {
                #pragma unroll
                for (int u = 0; u < 4; ++u) { wn[u] = res_ld_word(M.cache + (int64_t)slots[t + 4 + u] * ndw + dw); an[u] = A[t + 4 + u]; bn[u] = B[t + 4 + u]; }
            }
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                #pragma unroll
                for (int s = 0; s < 16; ++s) acc[s] = fma((double)((w4[u] >> (2 * s)) & 3u), a4[u], acc[s]);
            }
        }
        for (; t < t1; ++t) {
            const uint32_t w = res_ld_word(M.cache + (int64_t)slots[t] * ndw + dw);
            const double a = A[t];
            bsum += B[t];
            #pragma unroll
            for (int s = 0; s < 16; ++s) acc[s] = fma((double)((w >> (2 * s)) & 3u), a, acc[s]);
        }
    }
    #pragma unroll
    for (int s = 0; s < 16; ++s) part[g][d][s] = acc[s] + bsum;
    __syncthreads();
    const int dd = threadIdx.x >> 4, s = threadIdx.x & 15;
    double a = 0.0;
    for (int gg = 0; gg < groups; ++gg) a += part[gg][dd][s];
    return a;                                                    // row 256 blockIdx.x + threadIdx.x
}

// The same product for a workgroup of 16 waves and 1024 rows (round 5, second version).  In res_xv_rows a wave holds four column
// groups of 16 dwords each, so a column's slot, its coefficients and the address of its words are per-lane values: 41 % of the
// kernel's vector instructions were that bookkeeping (counters: 7.9 M wave instructions against 4.7 M for the decode and the
// multiply-adds).  Here wave g IS column group g over 64 dwords: the list entries are wave-uniform -- scalar loads, scalar address
// arithmetic, the coefficient an SGPR operand of the multiply-add -- and a lane's only own value is its dword's offset.  Same
// sums in the same order (a group's columns in list order, + the group's constant, then the groups in order): same bits.
// `part` = [8][64][17] doubles of dynamic LDS (69 632 B: two workgroups of 16 waves per CU).
constexpr int kResWideRows = 1024;
constexpr size_t kResWideLds = sizeof(double) * 8 * 64 * 17;
__device__ __forceinline__ double res_xv_rows_wide(const ResMat &M, const int64_t *__restrict__ idx, const int32_t *__restrict__ slots,
                                                   const int32_t *__restrict__ fresh, int nfresh, const double *__restrict__ A,
                                                   const double *__restrict__ B, int64_t nnz, double *part /* [8][64][17] */)
{
    const int64_t ndw = M.ndw;
    const int d = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // (wave-uniform, and the compiler may know it)
    const int64_t dw = blockIdx.x * 64ll + d;
    if (nfresh > 0) {                                            // (uniform)
        if (dw < ndw)
            for (int e = g; e < nfresh; e += 16) {
                const int t = fresh[e];
                M.cache[(int64_t)slots[t] * ndw + dw] = M.X[xword(M.nbp, idx[t], dw)];
            }
        // (round 6) no device-scope fence here.  `__threadfence()` is a release that writes back the XCD's whole L2 (rule 6 of
        // DESIGN 3.2) -- by every wave of every workgroup, behind kernels that have just written megabytes: in a cross-validation,
        // whose short fits bring new columns in almost every step, it made this kernel 180 us per fit instead of 22
        // (tools/cv_window_trace.sh).  What is needed is less: the copies of THIS workgroup's waves must be read back by its own
        // waves.  The barrier waits for the stores (they are write-through: acknowledged by L2), and the words are read with
        // device-scope loads, which do not look at this CU's vector cache (a line of the slot's previous column may sit there).
        __syncthreads();
    }
    const int groups = (int)(nnz < 16 ? nnz : 16);
    const int64_t per = groups ? (nnz + groups - 1) / groups : 0;
    const int64_t t0 = g * per, t1 = (g < groups) ? (t0 + per < nnz ? t0 + per : nnz) : t0;
    double acc[16];
    #pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.0;
    double bsum = 0.0;
    if (dw < ndw) {
        const uint32_t *col0 = M.cache + dw;
        int64_t t = t0;
        uint32_t wn[4] = {0u, 0u, 0u, 0u};
        if (t + 4 <= t1) {
            #pragma unroll
            for (int u = 0; u < 4; ++u) wn[u] = res_ld_word(col0 + (int64_t)slots[t + u] * ndw);
        }
        for (; t + 4 <= t1; t += 4) {
            uint32_t w4[4];
            #pragma unroll
            for (int u = 0; u < 4; ++u) w4[u] = wn[u];
            if (t + 8 <= t1) {
                #pragma unroll
                for (int u = 0; u < 4; ++u) wn[u] = res_ld_word(col0 + (int64_t)slots[t + 4 + u] * ndw);
            }
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double a = A[t + u];
                bsum += B[t + u];
                #pragma unroll
                for (int s = 0; s < 16; ++s) acc[s] = fma((double)((w4[u] >> (2 * s)) & 3u), a, acc[s]);
            }
        }
        for (; t < t1; ++t) {
            const uint32_t w = res_ld_word(col0 + (int64_t)slots[t] * ndw);
            const double a = A[t];
            bsum += B[t];
            #pragma unroll
            for (int s = 0; s < 16; ++s) acc[s] = fma((double)((w >> (2 * s)) & 3u), a, acc[s]);
        }
    }
    // the groups' partial sums meet in LDS, eight groups at a time (70 KB instead of 139: TWO workgroups per CU, so that the 489
    // workgroups of n = 500 000 are all resident at once -- each walks a chain of dependent loads, gate -> lists -> words -> rows,
    // and a second round of workgroups would pay that latency again); a row's sum runs over the groups in order all the same
    double *mine = part + ((size_t)(g & 7) * 64 + d) * 17;
    const int dd = threadIdx.x >> 4, s = threadIdx.x & 15;
    double a = 0.0;
    if (g < 8) {
        #pragma unroll
        for (int u = 0; u < 16; ++u) mine[u] = acc[u] + bsum;
    }
    __syncthreads();
    for (int gg = 0; gg < (groups < 8 ? groups : 8); ++gg) a += part[((size_t)gg * 64 + dd) * 17 + s];
    if (groups > 8) {                                            // (uniform)
        __syncthreads();
        if (g >= 8) {
            #pragma unroll
            for (int u = 0; u < 16; ++u) mine[u] = acc[u] + bsum;
        }
        __syncthreads();
        for (int gg = 8; gg < groups; ++gg) a += part[((size_t)(gg - 8) * 64 + dd) * 17 + s];
    }
    return a;                                                    // row 1024 blockIdx.x + threadIdx.x
}
// block_sum (fit_common.h) for a workgroup of 1024: each quarter of 256 threads is one of the 256-row blocks the host-driven
// kernels sum over -- the same tree, the same slot of `red`
template <int NV>
__device__ __forceinline__ void res_block_sum_wide(double (&v)[NV], double *__restrict__ red, int nb)
{
    extern __shared__ double res_part[];             // the product's partials have been read (res_xv_rows_wide's caller): the same LDS again
    double (*sh)[1024] = reinterpret_cast<double (*)[1024]>(res_part);
    const int t = threadIdx.x & 255;
    __syncthreads();
    #pragma unroll
    for (int k = 0; k < NV; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) {
            #pragma unroll
            for (int k = 0; k < NV; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + st];
        }
        __syncthreads();
    }
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 8);
    if (t == 0 && blk < nb) {
        #pragma unroll
        for (int k = 0; k < NV; ++k) red[(size_t)NV * blk + k] = sh[k][threadIdx.x];
    }
}

// imputed (missing) entries of the support columns: k_xv_missing with the list and its length on the device
__device__ __forceinline__ void
b_res_missing(ResPtrs P, int epoch, int attempt, int which /* 0: current iterate, 1: candidate */, ResMat M, double *__restrict__ out)
{
    const ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    const int b = which ? 1 - ctl->cur : ctl->cur;
    const int64_t nnz = ctl->m[b].cnt;
    const int64_t *idx = P.idx[b];
    for (int64_t t = 0; t < nnz; ++t) {
        const int64_t j = idx[t];
        const int64_t a = M.miss_ptr[j], e1 = M.miss_ptr[j + 1];
        const double fix = M.mu[j] * P.coefA[t];
        for (int64_t e = a + threadIdx.x; e < e1; e += blockDim.x) out[M.miss_row[e]] += fix;
        if (e1 > a) __syncthreads();
    }
}

// iht_stepsize!'s denominator (utilities.jl:744-756): the block's share of sum ((X_S df_S + Z df2_idc) sqrt(mueta^2/var) w)^2 --
// k_stepsize_dev's terms and block sums
template <bool WIDE = false>
__device__ __forceinline__ void res_stepsize_rows(const ResPtrs &P, double xg, int64_t i, const double *__restrict__ z, const double *__restrict__ xb,
                                                  const double *__restrict__ zc, const double *__restrict__ mu, const double *__restrict__ w,
                                                  int64_t n, int q, int dist, int link, double nb_r, double *__restrict__ red)
{
    const ResCtl *ctl = P.ctl;
    const uint64_t idc = ctl->m[ctl->cur].idc;
    double v[1] = {0.0};
    if (i < n) {
        double a = 0.0;
        for (int l = 0; l < q; ++l) a += z[(int64_t)l * n + i] * (((idc >> l) & 1ull) ? ctl->df2[l] : 0.0);
        double g = xg + a;
        double sw;
        if (dist == MIH_NORMAL && link == MIH_IDENTITY) sw = w[i];      // sqrt(1 * 1 / 1) * w: the same bits without three cold vectors
        else {
            const double me = d_mueta(link, xb[i] + zc[i]);
            sw = sqrt(me * me / d_glmvar(dist, mu[i], nb_r)) * w[i];
        }
        g *= sw;
        v[0] = g * g;
    }
    if (WIDE) res_block_sum_wide<1>(v, red, (int)((n + 255) / 256));
    else block_sum<1>(v, red + blockIdx.x);
}
// ... and the step size itself, by one workgroup: the shares added in k_final_sum's order, the numerator as the host forms it
// (utilities.jl:754: the support's df in list order, then the kept covariates)
__device__ __forceinline__ void
b_res_eta(ResPtrs P, int epoch, const double *__restrict__ red, int nb, int q, const double *numer_snp /* column shard: sum over ALL shards of |df_S|^2 */)
{
#pragma clang fp contract(off)        // (the host forms numer += v * v without fused multiply-adds)
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, -1)) return;
    __shared__ double sred[1][256];
    __shared__ double sg[4096];
    const ResModel &m0 = ctl->m[ctl->cur];
    const int64_t cnt = m0.cnt;
    double dn[1];
    res_final_sums<1>(red, nb, dn, sred);
    const double denom = dn[0];
    double numer = numer_snp ? *numer_snp : 0.0;
    for (int64_t base = 0; base < (numer_snp ? 0 : cnt); base += 4096) {
        const int64_t end = base + 4096 < cnt ? base + 4096 : cnt;
        for (int64_t t = base + threadIdx.x; t < end; t += 256) sg[t - base] = P.gval[t];
        __syncthreads();
        if (threadIdx.x == 0) {                       // in list order, eight LDS reads in flight (the additions stay sequential)
            int64_t t = base;
            for (; t + 8 <= end; t += 8) {
                double g8[8];
                #pragma unroll
                for (int u = 0; u < 8; ++u) g8[u] = sg[t - base + u];
                #pragma unroll
                for (int u = 0; u < 8; ++u) numer += g8[u] * g8[u];
            }
            for (; t < end; ++t) numer += sg[t - base] * sg[t - base];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int l = 0; l < q; ++l) if ((m0.idc >> l) & 1ull) numer += ctl->df2[l] * ctl->df2[l];
        double e = numer / denom;
        if (isinf(e) || isnan(e)) e = 1e-8;
        ctl->eta = e;
        ctl->live_epoch = res_gate_attempt(epoch);          // the attempt slots queued behind are on
    }
}

// Start of a step: save_prev!'s best model (utilities.jl:702-712), X_S df_S over the cached columns and the step size.
// SPLIT: the matrix has imputed entries -- the product is stored, k_res_missing adds the imputation term, k_res_stepsize goes on.
template <bool SPLIT>
__device__ __forceinline__ void         // (eight waves per SIMD = two workgroups per CU: 64 VGPRs)
b_res_xgk(ResPtrs P, int epoch, ResMat M, const double *__restrict__ z, const double *__restrict__ xb, const double *__restrict__ zc,
          const double *__restrict__ mu, const double *__restrict__ w, int q, int dist, int link, double nb_r,
          double *__restrict__ xgk, double *__restrict__ red)
{
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, -1)) return;
    extern __shared__ double res_part[];
    const int cur = ctl->cur;
    const int64_t cnt = ctl->m[cur].cnt;
    if (blockIdx.x == 0 && ctl->logl_cur > ctl->best_logl) {       // (nobody else reads the best model while a step runs)
        for (int64_t t = threadIdx.x; t < cnt; t += 1024) { P.idx[2][t] = P.idx[cur][t]; P.val[2][t] = P.val[cur][t]; }
        if (threadIdx.x < kMaxQ) ctl->best.c[threadIdx.x] = ctl->m[cur].c[threadIdx.x];
        if (threadIdx.x == 0) { ctl->best.cnt = cnt; ctl->best.idc = ctl->m[cur].idc; ctl->best_logl = ctl->logl_cur; }
    }
    const double a = res_xv_rows_wide(M, P.idx[cur], P.slot[cur], P.fresh[cur], ctl->nfresh[cur], P.coefA, P.coefB, cnt, res_part);
    const int64_t i = blockIdx.x * 1024ll + threadIdx.x;
    if (SPLIT) { if (i < M.n) xgk[i] = a; return; }
    res_stepsize_rows<true>(P, a, i, z, xb, zc, mu, w, M.n, q, dist, link, nb_r, red);
}
__device__ __forceinline__ void
b_res_stepsize(ResPtrs P, int epoch, const double *__restrict__ xgk, const double *__restrict__ z, const double *__restrict__ xb,
               const double *__restrict__ zc, const double *__restrict__ mu, const double *__restrict__ w, int64_t n, int q,
               int dist, int link, double nb_r, double *__restrict__ red)
{
    if (res_dead(P.ctl, epoch, -1)) return;
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    res_stepsize_rows(P, i < n ? xgk[i] : 0.0, i, z, xb, zc, mu, w, n, q, dist, link, nb_r, red);
}

// k_pick11's choice among 2048 bins by ONE block (thread t owns bins 8t .. 8t+7): out[0] = bin, out[1] = the rank that remains in it
__device__ __forceinline__ void res_pick11(const uint32_t *hist, uint64_t kth, uint64_t *suf /* 257, shared */, uint64_t *out /* 2, shared */)
{
    const int t = threadIdx.x;
    uint32_t mine[8]; uint64_t own = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) { mine[j] = __hip_atomic_load(&hist[8 * t + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); own += mine[j]; }
    suf[t] = own;
    if (t == 0) suf[256] = 0;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint64_t add = (t + off < 256) ? suf[t + off] : 0;
        __syncthreads();
        suf[t] += add;
        __syncthreads();
    }
    const bool owner = (suf[t + 1] < kth && suf[t] >= kth) || (t == 0 && suf[0] < kth);
    if (owner) {
        uint64_t above = suf[t + 1];
        int bin = 8 * t;
        for (int j = 7; j >= 0; --j) { if (above + mine[j] >= kth) { bin = 8 * t + j; break; } above += mine[j]; }
        if (suf[0] < kth) { bin = 0; above = suf[0] - mine[0]; }
        out[0] = (uint64_t)bin;
        out[1] = kth > above ? kth - above : 1;
    }
    __syncthreads();
}

// The gradient step vectorized into `full` (utilities.jl:258-264, 291-315: b + eta df on the support, eta df elsewhere, prior
// weights, the covariate tail with Inf for the kept ones) and the exponent histogram of the projection's first pass.  A block owns
// a contiguous range of the vector.
// FAST (the direct gather): once the fit has settled, project_k!'s threshold in attempt a of a step is close to what it was in
// attempt a of the step before (whether it sits on a weak effect or in the noise tail, where it follows the step size).  So
// instead of locating it with two histogram sweeps the kernel gathers, while it writes `full`, every entry of at least 0.9 x that
// threshold (scaled down with the step size if that shrank) into its block's list (k_res_collect's lists); k_res_select then has
// the exact K largest among them -- if there are at least K and the lists held them all.  If not, it says so and the host
// re-queues the attempt with the histograms: a forecast that is verified, never a different result.
constexpr int kResGradBlocks = 512;
constexpr int kResCollectSlots = 32;          // entries per block list
template <bool FAST>
__device__ __forceinline__ void
b_res_grad(ResPtrs P, int epoch, int attempt, const double *__restrict__ df, const double *__restrict__ weight, int64_t p, int q, uint64_t zkeep,
           int64_t sel_len /* entries the projection selects among: p + q, or p in a column shard (the tail is judged globally) */,
           double *__restrict__ full)
{
#pragma clang fp contract(off)        // eta * df rounds before the prior weight multiplies (k_grad_full)
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    __shared__ uint32_t h[FAST ? 1 : 4][FAST ? 1 : 2048];
    __shared__ int64_t lst_idx[64]; __shared__ double lst_val[64]; __shared__ int lcnt, ccnt;
    const int cur = ctl->cur;
    const ResModel &m0 = ctl->m[cur];
    const int64_t cnt = m0.cnt;
    const int64_t *idx0 = P.idx[cur]; const double *val0 = P.val[cur];
    const double eta = res_halved(ctl->eta, ctl->es);
    if (!FAST) for (int e = threadIdx.x; e < 4 * 2048; e += 256) (&h[0][0])[e] = 0;
    if (threadIdx.x == 0) { lcnt = 0; ccnt = 0; }
    __syncthreads();
    // the forecast as a key; without one nothing qualifies and the select reports the failure
    uint64_t Lk = 0;
    if (FAST) {
        // (an attempt number that has not been seen yet borrows the forecast of the last one that has: the threshold follows the step size)
        int ai = ctl->es < kResMaxAttempts ? ctl->es : kResMaxAttempts - 1;
        while (ai > 0 && ctl->thr_key[ai] == 0) --ai;
        const uint64_t tk = ctl->thr_key[ai];
        const double te = ctl->thr_eta[ai], ratio = (te > 0.0 && eta < te) ? eta / te : 1.0;
        const double lv = 0.9 * __longlong_as_double((long long)tk) * ratio;
        Lk = (tk == 0 || !(lv > 0.0)) ? ~0ull : res_abs_key(lv);
    }
    uint64_t *cand = P.sel + kResGradBlocks + (size_t)blockIdx.x * kResCollectSlots * 2;
    const int64_t len = p + q, chunk = (len + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < len ? lo + chunk : len;
    for (int64_t t = threadIdx.x; t < cnt; t += 256) {             // the support entries of this block's range
        const int64_t j = idx0[t];
        if (j >= lo && j < hi) { const int pos = atomicAdd(&lcnt, 1); if (pos < 64) { lst_idx[pos] = j; lst_val[pos] = val0[t]; } }
    }
    __syncthreads();
    const int nl = lcnt, wave = FAST ? 0 : threadIdx.x >> 6;
    // eight entries per thread in flight (a block's range is 1954 entries at p = 10^6: a thread that fetched df one entry at a time,
    // cold after the pass, waited eight round trips)
    for (int64_t j0 = lo + threadIdx.x; j0 < hi; j0 += 8 * 256) {
        double dfv[8], wv[8];
        #pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t j = j0 + u * 256;
            dfv[u] = (j < hi && j < p) ? df[j] : 0.0;
            wv[u] = (weight && j < hi && j < p) ? weight[j] : 1.0;
        }
        #pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t j = j0 + u * 256;
            if (j >= hi) break;
            double v;
            if (j < p) {
                bool hit = false; double bv = 0.0;
                if (nl <= 64) { for (int e = 0; e < nl; ++e) if (lst_idx[e] == j) { hit = true; bv = lst_val[e]; } }
                else {                     // a dense cluster of effects: look the column up in the sorted list itself
                    int64_t a = 0, b = cnt;
                    while (a < b) { const int64_t mid = (a + b) >> 1; if (idx0[mid] < j) a = mid + 1; else b = mid; }
                    if (a < cnt && idx0[a] == j) { hit = true; bv = val0[a]; }
                }
                v = hit ? fma(eta, dfv[u], bv) : eta * dfv[u];           // BLAS.axpy!(eta, df, b) is an fma per element (k_scatter_b)
                if (weight) v = v * wv[u];
            } else {
                const int l = (int)(j - p);
                v = ((zkeep >> l) & 1ull) ? __longlong_as_double(0x7FF0000000000000ll) : fma(eta, ctl->df2[l], m0.c[l]);
            }
            if (!FAST || j >= p) full[j] = v;          // (a direct gather reads the candidates' lists, never the vector itself: 8 MB of stores per attempt less; the covariate tail is read by the sharded select)
            if (FAST) {
                if (j < sel_len && res_abs_key(v) >= Lk && v != 0.0) {
                    const int pos = atomicAdd(&ccnt, 1);
                    if (pos < kResCollectSlots) { cand[2 * pos] = (uint64_t)j; cand[2 * pos + 1] = (uint64_t)__double_as_longlong(v); }
                }
            } else if (j < sel_len) atomicAdd(&h[wave][(uint32_t)(res_abs_key(v) >> 52)], 1u);
        }
    }
    __syncthreads();
    if (FAST) { if (threadIdx.x == 0) P.sel[blockIdx.x] = (uint64_t)ccnt; return; }
    for (int b = threadIdx.x; b < 2048; b += 256) {
        const uint32_t tot = h[0][b] + h[1][b] + h[2][b] + h[3][b];
        if (tot) atomicAdd(&P.hist[b], tot);
    }
}

// project_k!, second histogram: the 11 mantissa bits below the exponent bin that holds the K-th largest magnitude.  Every block
// picks that bin from the first histogram for itself (a 2048-bin scan: ~2 us, against 2.5 us for a launch of its own or ~60 ns
// PER BLOCK for a last-block ticket); block 0 leaves the pick for the kernels behind.
constexpr int kResHistBlocks = 512;
__device__ __forceinline__ void
b_res_hist2(ResPtrs P, int epoch, int attempt, const double *__restrict__ full, int64_t len, uint64_t K)
{
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    __shared__ uint32_t h[4][2048];
    __shared__ uint64_t suf[257], pick[2];
    for (int e = threadIdx.x; e < 4 * 2048; e += 256) (&h[0][0])[e] = 0;
    res_pick11(P.hist, K, suf, pick);
    const uint64_t prefix = pick[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->topk[0] = pick[0]; ctl->topk[1] = pick[1]; }
    const int wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = blockIdx.x * 256ll + threadIdx.x;
    for (; i + 3 * stride < len; i += 4 * stride) {
        uint64_t key[4];
        #pragma unroll
        for (int u = 0; u < 4; ++u) key[u] = res_abs_key(full[i + u * stride]);
        #pragma unroll
        for (int u = 0; u < 4; ++u) if ((key[u] >> 52) == prefix) atomicAdd(&h[wave][(uint32_t)(key[u] >> 41) & 2047u], 1u);
    }
    for (; i < len; i += stride) {
        const uint64_t key = res_abs_key(full[i]);
        if ((key >> 52) == prefix) atomicAdd(&h[wave][(uint32_t)(key >> 41) & 2047u], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2048; b += 256) {
        const uint32_t tot = h[0][b] + h[1][b] + h[2][b] + h[3][b];
        if (tot) atomicAdd(&P.hist[2048 + b], tot);
    }
}

// project_k!, the gather: everything at or above the 22-bit prefix of the K-th largest magnitude.  Every block keeps its own
// short list (no counter shared by the whole grid: same-address atomics cost ~60 ns each on this chip); k_res_select reads them.
constexpr int kResCollectBlocks = 512;       // (= kResGradBlocks: the direct gather of k_res_grad<true> fills the same lists)
__device__ __forceinline__ void
b_res_collect(ResPtrs P, int epoch, int attempt, const double *__restrict__ full, int64_t len)
{
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    __shared__ int lcnt;
    __shared__ uint64_t suf[257], pick[2];
    if (threadIdx.x == 0) lcnt = 0;
    res_pick11(P.hist + 2048, ctl->topk[1], suf, pick);                // (every block for itself, as in k_res_hist2)
    const uint64_t pre = (ctl->topk[0] << 11) | pick[0], lo = pre << 41;
    if (blockIdx.x == 0) {                                             // the first histogram has served every block of k_res_hist2
        for (int b = threadIdx.x; b < 2048; b += 256) P.hist[b] = 0;
        if (threadIdx.x == 0) { ctl->topk[2] = pick[1]; ctl->topk[3] = pre; }
    }
    uint64_t *mine = P.sel + kResCollectBlocks + (size_t)blockIdx.x * kResCollectSlots * 2;
    const int64_t stride = (int64_t)gridDim.x * 256;
    // (round 6) a vector shorter than a few strides: block b takes the entries = b mod gridDim.x, so that a large model's survivors
    // spread over ALL the lists (with 256-entry runs per block the first len / 256 blocks got them all: 42 per list at K = 5000,
    // len = 30 000, and a list holds 32).  Which list an entry lands in does not matter: the select ranks them all.
    const bool spread = len < 4 * stride;
    for (int64_t i = spread ? (int64_t)threadIdx.x * gridDim.x + blockIdx.x : blockIdx.x * 256ll + threadIdx.x; i < len; i += stride) {
        const double v = full[i];
        if (res_abs_key(v) >= lo && v != 0.0) {
            const int pos = atomicAdd(&lcnt, 1);
            if (pos < kResCollectSlots) { mine[2 * pos] = (uint64_t)i; mine[2 * pos + 1] = (uint64_t)__double_as_longlong(v); }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) P.sel[blockIdx.x] = (uint64_t)lcnt;
}

// the barrier of k_res_select; BIG: its lists live in device memory, so what another wave stored before the barrier (write-through:
// acknowledged by L2 when the barrier's wait returns) must not be read from a stale line of this CU's vector cache
template <bool BIG>
__device__ __forceinline__ void res_sel_sync()
{
    __syncthreads();
    if (BIG) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
// project_k!'s exact finish, unvectorize!, the trigger of _choose!, the column-cache bookkeeping of the candidate, the coefficients of
// update_xb! and check_convergence -- one workgroup.  The survivors are the gathered entries above the threshold's 22-bit prefix
// plus, of those that share it, the ones with fewer than `rem` larger keys among them (ties at the threshold are kept:
// |x_i| >= a in utilities.jl:553-559 <=> fewer than K entries are strictly larger).
// BIG (round 6): survivor lists of up to kResBigList entries.  The same algorithm with the lists in a scratch block of device memory
// (P.big: one workgroup reads and writes it, barriers in between; the 1.9 MB stay in L2) instead of LDS, where 2048 entries fill
// 128 KB; the pool of entries that share the threshold's prefix stays in LDS (a direct gather would put ALL candidates there: the
// host does not queue one for such a model).  The reference's largest published run has k = 4678 (manuscript/UKBB_metabolomic).
template <bool BIG = false>
__device__ __forceinline__ void
b_res_select(ResPtrs P, int epoch, int attempt, int fast, uint64_t K, uint64_t seq, ResMat M, const double *__restrict__ weight, int64_t p, int q,
             uint64_t zkeep, int zkeepn, int64_t max_nonzero /* groups * (k + zkeepn), utilities.jl:447-449 */,
             int force_abort_es /* measurement build: hand the step back once it has backtracked this often (-1: never) */)
{
#pragma clang fp contract(off)
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    constexpr int kList = BIG ? kResBigList : kResMaxList, kBusy = BIG ? (2 * kResBigList + 1024) / 32 : 160;       // (the column cache holds 2 x model + 64 slots)
    __shared__ int64_t l_s_idx[BIG ? 1 : kResMaxList]; __shared__ double l_s_val[BIG ? 1 : kResMaxList];
    __shared__ uint64_t in_key[kResMaxInBin]; __shared__ int64_t in_idx[kResMaxInBin]; __shared__ uint64_t in_bits[kResMaxInBin];
    __shared__ uint32_t busy[kBusy];                // bitmap of cache slots in use by b0 and by the candidate's old columns
    __shared__ int32_t l_fresh_t[BIG ? 1 : kResMaxList];
    __shared__ int ns, nin, nfr, abort_why, nsnp_s, ncand;
    __shared__ double ct[kMaxQ]; __shared__ uint64_t cnz;
    __shared__ double red_d[16], red_n[16];
    __shared__ double c_new[kMaxQ]; __shared__ uint64_t idc_new;
    __shared__ int64_t l_o_idx[BIG ? 1 : kResMaxList]; __shared__ double l_o_val[BIG ? 1 : kResMaxList]; __shared__ int32_t l_o_slot[BIG ? 1 : kResMaxList];    // b0, staged (the searches below)
    int64_t *const s_idx = BIG ? reinterpret_cast<int64_t *>(P.big) : l_s_idx;
    double *const s_val = BIG ? reinterpret_cast<double *>(P.big + kResBigList) : l_s_val;
    int64_t *const o_idx = BIG ? reinterpret_cast<int64_t *>(P.big + 2 * kResBigList) : l_o_idx;
    double *const o_val = BIG ? reinterpret_cast<double *>(P.big + 3 * kResBigList) : l_o_val;
    int32_t *const fresh_t = BIG ? reinterpret_cast<int32_t *>(P.big + 6 * kResBigList) : l_fresh_t;
    int32_t *const o_slot = BIG ? reinterpret_cast<int32_t *>(P.big + 6 * kResBigList) + kResBigList : l_o_slot;
    const int tid = threadIdx.x;
    const int cur = ctl->cur, nw = 1 - cur;
    const ResModel &m0 = ctl->m[cur];
    const int64_t cnt0 = m0.cnt;
    // a direct gather (fast): every candidate is ranked, the K largest survive
    const uint64_t rem = fast ? K : ctl->topk[2], pre = fast ? ~0ull : ctl->topk[3];
    if (tid == 0) { ns = 0; nin = 0; nfr = 0; abort_why = 0; nsnp_s = 0; ncand = 0; cnz = 0; idc_new = 0; }
    if (tid < kMaxQ) ct[tid] = 0.0;
    for (int e = tid; e < kBusy; e += 1024) busy[e] = 0;
    res_sel_sync<BIG>();
    if ((M.slots > kBusy * 32 || cnt0 > kList || (BIG && (!P.big || fast))) && tid == 0) abort_why = 1;
    if (force_abort_es >= 0 && ctl->es >= force_abort_es && tid == 0) abort_why = 6;
    for (int64_t t = tid; t < cnt0 && t < kList; t += 1024) { o_idx[t] = P.idx[cur][t]; o_val[t] = P.val[cur][t]; o_slot[t] = P.slot[cur][t]; }
    if (!fast) for (int b = tid; b < 2048; b += 1024) P.hist[2048 + b] = 0;        // the second histogram has served every block of k_res_collect

    // the blocks' lists of k_res_collect: thread t walks list t
    for (int bl = tid; bl < kResCollectBlocks; bl += 1024) {
        const uint64_t *lst = P.sel + kResCollectBlocks + (size_t)bl * kResCollectSlots * 2;
        uint64_t first[8];                          // the list's first four entries travel with its length (one round trip instead of two:
        #pragma unroll                              // a list rarely holds more; what lies behind a short list's end is not looked at)
        for (int e = 0; e < 8; ++e) first[e] = lst[e];
        const int c = (int)P.sel[bl];
        if (c > kResCollectSlots) { abort_why = fast ? 5 : 1; continue; }  // (a benign race: the writers of one launch store the same value)
        if (fast) atomicAdd(&ncand, c);
        auto take = [&](uint64_t eidx, uint64_t bits) {
            const uint64_t key = bits & 0x7FFFFFFFFFFFFFFFull, top = key >> 41;
            if (!fast && top > pre) {
                const int pos = atomicAdd(&ns, 1);
                if (pos < kList) { s_idx[pos] = (int64_t)eidx; s_val[pos] = __longlong_as_double((long long)bits); }
            } else if (fast || top == pre) {
                const int pos = atomicAdd(&nin, 1);
                if (pos < kResMaxInBin) { in_key[pos] = key; in_idx[pos] = (int64_t)eidx; in_bits[pos] = bits; }
            }
        };
        #pragma unroll
        for (int e = 0; e < 4; ++e) if (e < c) take(first[2 * e], first[2 * e + 1]);
        for (int e = 4; e < c; ++e) take(lst[2 * e], lst[2 * e + 1]);
    }
    res_sel_sync<BIG>();
    if (!abort_why && fast && ((uint64_t)ncand < K || nin > kResMaxInBin)) { if (tid == 0) abort_why = 5; }      // the forecast did not hold
    if (!abort_why && (nin > kResMaxInBin || ns > kList)) { if (tid == 0) abort_why = 2; }
    res_sel_sync<BIG>();
    if (!abort_why) {
        // four threads per entry, each counting over a quarter of the pool (a count: any order), eight LDS reads in flight
        const int cnt_in = nin, quarter = (cnt_in + 3) >> 2;
        for (int e = tid >> 2; e < ((cnt_in + 255) & ~255); e += 256) {            // (whole waves stay in the loop for the shuffles)
            const bool on = e < cnt_in;
            const uint64_t ke = on ? in_key[e] : 0;
            const int f0 = (tid & 3) * quarter, f1 = f0 + quarter < cnt_in ? f0 + quarter : cnt_in;
            uint32_t larger = 0;
            int f = f0;
            for (; f + 8 <= f1; f += 8) {
                uint64_t k8[8];
                #pragma unroll
                for (int u = 0; u < 8; ++u) k8[u] = in_key[f + u];
                #pragma unroll
                for (int u = 0; u < 8; ++u) larger += k8[u] > ke;
            }
            for (; f < f1; ++f) larger += in_key[f] > ke;
            larger += __shfl_xor(larger, 1, 64);
            larger += __shfl_xor(larger, 2, 64);
            if (on && (tid & 3) == 0 && (uint64_t)larger < rem) {
                const int pos = atomicAdd(&ns, 1);
                if (pos < kList) { s_idx[pos] = in_idx[e]; s_val[pos] = __longlong_as_double((long long)in_bits[e]); }
            }
        }
    }
    res_sel_sync<BIG>();
    if (!abort_why && ns > kList) { if (tid == 0) abort_why = 2; }
    res_sel_sync<BIG>();
    const int nsv = ns;
    // the threshold itself (the smallest surviving magnitude, if K entries survived): the next direct gather's forecast
    __shared__ unsigned long long kmin;
    if (tid == 0) kmin = ~0ull;
    res_sel_sync<BIG>();
    {
        uint64_t km = ~0ull;
        if (!abort_why) for (int e = tid; e < nsv; e += 1024) { const uint64_t ke = res_abs_key(s_val[e]); km = ke < km ? ke : km; }
        km = res_wave_min_u64(km);                     // (one LDS atomic per wave: same-address LDS atomics serialise)
        if ((tid & 63) == 0 && km != ~0ull) atomicMin(&kmin, (unsigned long long)km);
    }
    res_sel_sync<BIG>();
    // order by index (in place: every thread ranks its entries, then all write)
    // (the pool's arrays are free by now: ranks go to in_key's memory, the ordered copy to in_idx's and in_bits's)
    int32_t *const rank_of = BIG ? reinterpret_cast<int32_t *>(P.big + 7 * kResBigList) : reinterpret_cast<int32_t *>(in_key);
    int64_t *const t_idx = BIG ? reinterpret_cast<int64_t *>(P.big + 4 * kResBigList) : in_idx;
    double *const t_val = BIG ? reinterpret_cast<double *>(P.big + 5 * kResBigList) : reinterpret_cast<double *>(in_bits);
    if (!abort_why) {
        const int quarter = (nsv + 3) >> 2;
        for (int e = tid >> 2; e < ((nsv + 255) & ~255); e += 256) {            // (whole waves stay in the loop for the shuffles)
            const bool on = e < nsv;
            const int64_t je = on ? s_idx[e] : 0;
            const int f0 = (tid & 3) * quarter, f1 = f0 + quarter < nsv ? f0 + quarter : nsv;
            int pos = 0, f = f0;
            for (; f + 8 <= f1; f += 8) {
                int64_t j8[8];
                #pragma unroll
                for (int u = 0; u < 8; ++u) j8[u] = s_idx[f + u];
                #pragma unroll
                for (int u = 0; u < 8; ++u) pos += j8[u] < je;
            }
            for (; f < f1; ++f) pos += s_idx[f] < je;
            pos += __shfl_xor(pos, 1, 64);
            pos += __shfl_xor(pos, 2, 64);
            if (on && (tid & 3) == 0) rank_of[e] = pos;
        }
    }
    res_sel_sync<BIG>();
    if (!abort_why) for (int e = tid; e < nsv; e += 1024) { const int pos = rank_of[e]; t_idx[pos] = s_idx[e]; t_val[pos] = s_val[e]; }
    res_sel_sync<BIG>();
    if (!abort_why) for (int e = tid; e < nsv; e += 1024) { const int64_t j = t_idx[e]; s_idx[e] = j; s_val[e] = t_val[e]; if (j < p) atomicAdd(&nsnp_s, 1); }
    res_sel_sync<BIG>();
    const int nsnp = nsnp_s;
    // the covariate tail (utilities.jl:264-265, 345-353) and the model of the candidate
    const double eta = res_halved(ctl->eta, ctl->es);
    if (!abort_why) {
        for (int e = nsnp + tid; e < nsv; e += 1024) { const int l = (int)(s_idx[e] - p); ct[l] = s_val[e]; atomicOr((unsigned long long *)&cnz, 1ull << l); }
    }
    res_sel_sync<BIG>();
    if (!abort_why && tid < q) {
        const double cn = fma(eta, ctl->df2[tid], m0.c[tid]);
        const double cv = ((zkeep >> tid) & 1ull) ? cn : (((cnz >> tid) & 1ull) ? ct[tid] : 0.0);
        c_new[tid] = cv;
        if (cv != 0.0) atomicOr((unsigned long long *)&idc_new, 1ull << tid);
    }
    res_sel_sync<BIG>();
    if (!abort_why && tid == 0) {
        const int64_t nz = (int64_t)nsnp - zkeepn + __popcll(idc_new);
        if (nz > max_nonzero) abort_why = 3;                       // exact ties: _choose! draws (utilities.jl:444-458) -- the host path does
        else if (nsnp > M.slots || nsnp > P.kcap) abort_why = 4;
    }
    res_sel_sync<BIG>();
    // cache slots: a column of the candidate that b0 holds keeps its slot; the others take slots neither list uses
    const int64_t *idx0 = o_idx; const double *val0 = o_val; const int32_t *slot0 = o_slot;
    int64_t *idx1 = P.idx[nw]; double *val1 = P.val[nw]; int32_t *slot1 = P.slot[nw];
    double dmax = 0.0, nbm = 0.0;
    if (!abort_why) {
        for (int64_t t = tid; t < cnt0; t += 1024) { const int32_t sl = slot0[t]; atomicOr(&busy[sl >> 5], 1u << (sl & 31)); }
        for (int e = tid; e < nsnp; e += 1024) {
            const int64_t j = s_idx[e];
            double v = s_val[e];
            if (weight) v = v / weight[j];                          // unvectorize! (utilities.jl:335-339)
            s_val[e] = v;
            int64_t a = 0, b = cnt0;
            while (a < b) { const int64_t mid = (a + b) >> 1; if (idx0[mid] < j) a = mid + 1; else b = mid; }
            double v0 = 0.0;
            if (a < cnt0 && idx0[a] == j) { slot1[e] = slot0[a]; v0 = val0[a]; }
            else { slot1[e] = -1; fresh_t[atomicAdd(&nfr, 1)] = e; }
            dmax = fmax(dmax, fabs(v - v0));
            idx1[e] = j; val1[e] = v;
            const double a_ = (M.scale ? M.sinv[j] : 1.0) * v;
            P.coefA[e] = a_; P.coefB[e] = M.center ? -M.mu[j] * a_ : 0.0;
        }
        // check_convergence (utilities.jl:953-957) over the union of the two supports
        for (int64_t t = tid; t < cnt0; t += 1024) {
            const int64_t j = idx0[t]; const double v0 = val0[t];
            nbm = fmax(nbm, fabs(v0));
            int a = 0, b = nsnp;
            while (a < b) { const int mid = (a + b) >> 1; if (s_idx[mid] < j) a = mid + 1; else b = mid; }
            if (!(a < nsnp && s_idx[a] == j)) dmax = fmax(dmax, fabs(0.0 - v0));
        }
        if (tid < q) { dmax = fmax(dmax, fabs(c_new[tid] - m0.c[tid])); nbm = fmax(nbm, fabs(m0.c[tid])); }
    }
    dmax = res_wave_max(dmax); nbm = res_wave_max(nbm);       // (maxima: any order)
    if ((tid & 63) == 0) { red_d[tid >> 6] = dmax; red_n[tid >> 6] = nbm; }
    res_sel_sync<BIG>();
    if (tid == 0) for (int wv = 1; wv < 16; ++wv) { red_d[0] = fmax(red_d[0], red_d[wv]); red_n[0] = fmax(red_n[0], red_n[wv]); }
    if (!abort_why && tid == 0) {
        const int nf = nfr;
        int sl = 0, given = 0;
        for (; given < nf && sl < M.slots; ++sl)
            if (!((busy[sl >> 5] >> (sl & 31)) & 1u)) { slot1[fresh_t[given]] = sl; ++given; }
        if (given < nf) abort_why = 4;
        else {
            for (int e = 0; e < nf; ++e) P.fresh[nw][e] = fresh_t[e];
            ctl->nfresh[nw] = nf;
            ResModel &m1 = ctl->m[nw];
            m1.cnt = nsnp; m1.idc = idc_new;
            for (int l = 0; l < kMaxQ; ++l) m1.c[l] = l < q ? c_new[l] : 0.0;
            ctl->tol = red_d[0] / (red_n[0] + 1.0);
            if (ctl->es < kResMaxAttempts) { ctl->thr_key[ctl->es] = (uint64_t)nsv >= K ? (uint64_t)kmin : 0ull; ctl->thr_eta[ctl->es] = eta; }
        }
    }
    res_sel_sync<BIG>();
    if (abort_why && tid == 0) {                 // the iterate is untouched: the host replays this step through the host-driven path --
        // or, after a direct gather whose forecast failed, this attempt with the histograms (the slots the host queues then)
        ctl->live_epoch = abort_why == 5 ? res_gate_attempt(epoch + 1) : res_gate_step(epoch + 1);
        res_publish(P.rec, seq, abort_why == 5 ? RES_REDO_SLOW : RES_ABORT, 0.0, 0.0, eta, ctl->es, ctl->iter, cur, abort_why);
    }
}

// ---- column-sharded fit: project_k! over the shards --------------------------------------------------------------------------
// (IhtVar::project_full_sharded states the rule: the K-th largest |entry| of the whole vector is the K-th largest of the union of
// every shard's own top K and the covariate tail; ties at that value are kept.)  k_res_select_local: this shard's exact top-Kloc of
// its own columns (the candidates of k_res_grad's direct gather, or of the two histogram sweeps), every local survivor kept for the
// second stage, the K largest -- by (magnitude descending, index ascending), as the host orders them -- into the message
// [count | (global index, value) x K | status].  The all-gather of the messages is queued on the fit's stream.
// k_res_select_global: the same second stage on every shard -- ANY shard's status other than 0 (a failed forecast, lists beyond the
// buffers, ties cut off at the message size) makes every shard take the same way out, so the hosts keep issuing the same
// collectives -- the threshold by rank counting over the pooled candidates and the tail, this shard's survivors, the whole model
// (global lists: check_convergence and _choose!'s count), then unvectorize!, cache slots and update_xb!'s coefficients as in
// k_res_select.
static __global__ void __launch_bounds__(1024)
k_res_select_local(ResPtrs P, int epoch, int attempt, int fast, uint64_t Kloc, uint64_t K, int32_t slots)
{
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    __shared__ uint64_t c_key[kResMaxInBin]; __shared__ int64_t c_idx[kResMaxInBin]; __shared__ uint64_t c_bits[kResMaxInBin];
    __shared__ uint8_t c_keep[kResMaxInBin];
    __shared__ int nc, ncand, status, nkeep;
    __shared__ unsigned long long kmin;
    const int tid = threadIdx.x;
    const uint64_t rem = fast ? Kloc : ctl->topk[2], pre = fast ? ~0ull : ctl->topk[3];
    if (tid == 0) { nc = 0; ncand = 0; status = 0; nkeep = 0; kmin = ~0ull; }
    __syncthreads();
    if (!fast) for (int b = tid; b < 2048; b += 1024) P.hist[2048 + b] = 0;
    for (int bl = tid; bl < kResCollectBlocks; bl += 1024) {
        const uint64_t *lst = P.sel + kResCollectBlocks + (size_t)bl * kResCollectSlots * 2;
        const int c = (int)P.sel[bl];
        if (c > kResCollectSlots) { status = fast ? 5 : 1; continue; }
        atomicAdd(&ncand, c);
        for (int e = 0; e < c; ++e) {
            const uint64_t bits = lst[2 * e + 1], key = bits & 0x7FFFFFFFFFFFFFFFull;
            const int pos = atomicAdd(&nc, 1);
            if (pos < kResMaxInBin) { c_key[pos] = key; c_idx[pos] = (int64_t)lst[2 * e]; c_bits[pos] = bits; }
        }
    }
    __syncthreads();
    if (!status && tid == 0) {
        if (fast && (uint64_t)ncand < Kloc) status = 5;               // the forecast did not hold
        else if (nc > kResMaxInBin) status = fast ? 5 : 2;
    }
    __syncthreads();
    const int ncv = status ? 0 : nc;
    // local survivors: entries above the 22-bit prefix, and of those that share it the ones with fewer than `rem` larger among them
    // (direct gather: every candidate is ranked, the Kloc largest -- and what ties with the last of them -- survive)
    for (int e = tid; e < ncv; e += 1024) {
        const uint64_t ke = c_key[e], top = ke >> 41;
        bool keep;
        if (!fast && top > pre) keep = true;
        else if (!fast && top < pre) keep = false;
        else {
            uint64_t larger = 0;
            for (int f = 0; f < ncv; ++f) larger += (fast || (c_key[f] >> 41) == pre) && c_key[f] > ke;
            keep = larger < rem;
        }
        c_keep[e] = keep;
        if (keep) atomicAdd(&nkeep, 1);
    }
    __syncthreads();
    const int nk = nkeep;
    if (!status && tid == 0) {
        const int64_t cnt0 = ctl->m[ctl->cur].cnt;
        if (nk > kResShardList || nk > P.kcap || cnt0 + nk > slots) status = 4;
    }
    __syncthreads();
    // the message: the K largest survivors by (magnitude descending, index ascending); every survivor into the local list
    const int Ki = (int)K;
    for (int t = tid; t < 2 * Ki; t += 1024) P.msg[1 + t] = (t & 1) ? 0.0 : -1.0;
    __syncthreads();
    if (!status) {
        uint64_t km = ~0ull;
        for (int e = tid; e < ncv; e += 1024) {
            if (!c_keep[e]) continue;
            const uint64_t ke = c_key[e]; const int64_t je = c_idx[e];
            km = ke < km ? ke : km;
            int pos = 0, lpos = 0;
            for (int f = 0; f < ncv; ++f) {
                if (!c_keep[f]) continue;
                pos += (c_key[f] > ke) || (c_key[f] == ke && c_idx[f] < je);
                lpos += c_idx[f] < je;
            }
            if (pos < Ki) { P.msg[1 + 2 * pos] = (double)(P.col0 + je); P.msg[2 + 2 * pos] = __longlong_as_double((long long)c_bits[e]); }
            P.lc_idx[lpos] = je; P.lc_val[lpos] = __longlong_as_double((long long)c_bits[e]);       // (ordered by index)
        }
        km = res_wave_min_u64(km);
        if ((tid & 63) == 0 && km != ~0ull) atomicMin(&kmin, (unsigned long long)km);
    }
    __syncthreads();
    if (tid == 0) {
        P.msg[0] = (double)nk;
        P.msg[1 + 2 * Ki] = (double)status;
        ctl->lc_cnt = status ? 0 : nk;
        if (!status && ctl->es < kResMaxAttempts) {
            ctl->thr_key[ctl->es] = (uint64_t)nk >= Kloc ? (uint64_t)kmin : 0ull;
            ctl->thr_eta[ctl->es] = res_halved(ctl->eta, ctl->es);
        }
    }
}

static __global__ void __launch_bounds__(1024)
k_res_select_global(ResPtrs P, int epoch, int attempt, uint64_t K, uint64_t seq, ResMat M, const double *__restrict__ full, int64_t p, int q,
                    uint64_t zkeep, int zkeepn, int64_t max_nonzero)
{
#pragma clang fp contract(off)
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    __shared__ uint64_t pk[kResMaxInBin]; __shared__ int64_t pi[kResMaxInBin]; __shared__ double pv[kResMaxInBin]; __shared__ uint8_t pkeep[kResMaxInBin];
    __shared__ int64_t s_idx[kResShardList]; __shared__ double s_val[kResShardList];
    __shared__ int64_t o_idx[kResShardList]; __shared__ double o_val[kResShardList]; __shared__ int32_t o_slot[kResShardList];
    __shared__ int64_t g_idx[kResShardList]; __shared__ double g_val[kResShardList];
    __shared__ int32_t fresh_t[kResShardList];
    __shared__ uint8_t lkeep[kResShardList];
    __shared__ uint32_t busy[160];
    __shared__ double tailv[kMaxQ], c_new[kMaxQ];
    __shared__ uint64_t cnz, idc_new;
    __shared__ int npool, ns, ng, nfr, why;
    __shared__ double red_d[16], red_n[16];
    const int tid = threadIdx.x;
    const int W = P.world, Ki = (int)K, mlen = 2 + 2 * Ki;
    const int cur = ctl->cur, nw = 1 - cur;
    const ResModel &m0 = ctl->m[cur];
    const int64_t cnt0 = m0.cnt;
    const double eta = res_halved(ctl->eta, ctl->es);
    if (tid == 0) { npool = 0; ns = 0; ng = 0; nfr = 0; why = 0; cnz = 0; idc_new = 0; }
    for (int e = tid; e < 160; e += 1024) busy[e] = 0;
    __syncthreads();
    // every shard's status: one way out for all
    for (int r = tid; r < W; r += 1024) {
        const int st = (int)P.msgs[(size_t)r * mlen + 1 + 2 * Ki];
        if (st) atomicMax(&why, st == 5 ? 5 : 1);                    // (5 only if nothing worse: an overflow needs the host-driven step)
    }
    if (tid < q) tailv[tid] = full[p + tid];
    if ((cnt0 > kResShardList || M.slots > 160 * 32 || W * Ki + q > kResMaxInBin) && tid == 0) why = 1;
    __syncthreads();
    if (!why) {
        for (int e = tid; e < W * Ki; e += 1024) {
            const int r = e / Ki, t = e - r * Ki;
            const double gi = P.msgs[(size_t)r * mlen + 1 + 2 * t];
            if (gi < 0.0) continue;
            const double v = P.msgs[(size_t)r * mlen + 2 + 2 * t];
            const int pos = atomicAdd(&npool, 1);
            pk[pos] = res_abs_key(v); pi[pos] = (int64_t)gi; pv[pos] = v;
        }
    }
    __syncthreads();
    const int np0 = npool;                                       // SNP candidates of all shards
    if (!why && tid < q) { pk[np0 + tid] = res_abs_key(tailv[tid]); pi[np0 + tid] = -1 - tid; pv[np0 + tid] = tailv[tid]; }
    __syncthreads();
    const int np = np0 + (why ? 0 : q);
    if (!why && (uint64_t)np < K && tid == 0) why = 1;           // (the host-driven step raises the reference's error)
    __syncthreads();
    // |x_i| >= a  <=>  fewer than K pooled entries are strictly larger
    if (!why) {
        for (int e = tid; e < np; e += 1024) {
            const uint64_t ke = pk[e];
            uint64_t larger = 0;
            for (int f = 0; f < np; ++f) larger += pk[f] > ke;
            pkeep[e] = larger < K;
        }
    }
    __syncthreads();
    if (!why) {
        // a shard that had more survivors than the message holds: if the smallest one it sent survives, some of its ties may be missing
        for (int r = tid; r < W; r += 1024) {
            if (P.msgs[(size_t)r * mlen] <= (double)Ki) continue;
            const double vlast = P.msgs[(size_t)r * mlen + 2 + 2 * (Ki - 1)];
            const uint64_t kl = res_abs_key(vlast);
            uint64_t larger = 0;
            for (int f = 0; f < np; ++f) larger += pk[f] > kl;
            if (larger < K) why = 1;
        }
        // this shard's survivors (its whole local list against the pooled threshold), ordered by index as k_res_select_local left them
        const int64_t lc = ctl->lc_cnt;
        for (int64_t e = tid; e < lc; e += 1024) {
            const uint64_t ke = res_abs_key(P.lc_val[e]);
            uint64_t larger = 0;
            for (int f = 0; f < np; ++f) larger += pk[f] > ke;
            lkeep[e] = larger < K;
            if (larger < K) atomicAdd(&ns, 1);
        }
        for (int e = tid; e < np0; e += 1024) if (pkeep[e]) atomicAdd(&ng, 1);
        if (tid < q && pkeep[np0 + tid]) atomicOr((unsigned long long *)&cnz, 1ull << tid);
    }
    __syncthreads();
    const int nsnp = why ? 0 : ns, ngl = why ? 0 : ng;
    if (!why && tid == 0 && (ngl > kResShardList || nsnp > kResShardList)) why = 1;
    __syncthreads();
    if (!why) {
        // positions: local survivors keep their index order; the whole model is ordered by global index
        const int64_t lc = ctl->lc_cnt;
        for (int64_t e = tid; e < lc; e += 1024) {
            if (!lkeep[e]) continue;
            int pos = 0;
            for (int64_t f = 0; f < e; ++f) pos += lkeep[f];
            s_idx[pos] = P.lc_idx[e]; s_val[pos] = P.lc_val[e];
        }
        for (int e = tid; e < np0; e += 1024) {
            if (!pkeep[e]) continue;
            int pos = 0;
            for (int f = 0; f < np0; ++f) pos += pkeep[f] && pi[f] < pi[e];
            g_idx[pos] = pi[e]; g_val[pos] = pv[e];
        }
        for (int64_t t = tid; t < cnt0; t += 1024) { o_idx[t] = P.idx[cur][t]; o_val[t] = P.val[cur][t]; o_slot[t] = P.slot[cur][t]; }
    }
    __syncthreads();
    if (!why && tid < q) {
        const double cn = fma(eta, ctl->df2[tid], m0.c[tid]);
        const double cv = ((zkeep >> tid) & 1ull) ? cn : (((cnz >> tid) & 1ull) ? tailv[tid] : 0.0);
        c_new[tid] = cv;
        if (cv != 0.0) atomicOr((unsigned long long *)&idc_new, 1ull << tid);
    }
    __syncthreads();
    if (!why && tid == 0) {
        const int64_t nz = (int64_t)ngl - zkeepn + __popcll(idc_new);       // _choose! counts the WHOLE model (utilities.jl:447-449)
        if (nz > max_nonzero) why = 3;
        else if (nsnp > M.slots || nsnp > P.kcap) why = 4;
    }
    __syncthreads();
    int64_t *idx1 = P.idx[nw]; double *val1 = P.val[nw]; int32_t *slot1 = P.slot[nw];
    double dmax = 0.0, nbm = 0.0;
    if (!why) {
        for (int64_t t = tid; t < cnt0; t += 1024) { const int32_t sl = o_slot[t]; atomicOr(&busy[sl >> 5], 1u << (sl & 31)); }
        for (int e = tid; e < nsnp; e += 1024) {
            const int64_t j = s_idx[e];
            const double v = s_val[e];
            int64_t a = 0, b = cnt0;
            while (a < b) { const int64_t mid = (a + b) >> 1; if (o_idx[mid] < j) a = mid + 1; else b = mid; }
            if (a < cnt0 && o_idx[a] == j) slot1[e] = o_slot[a];
            else { slot1[e] = -1; fresh_t[atomicAdd(&nfr, 1)] = e; }
            idx1[e] = j; val1[e] = v;
            const double a_ = (M.scale ? M.sinv[j] : 1.0) * v;
            P.coefA[e] = a_; P.coefB[e] = M.center ? -M.mu[j] * a_ : 0.0;
        }
        // check_convergence (utilities.jl:953-957) over the union of the two WHOLE models
        const int64_t g0n = ctl->gcnt[cur];
        const int64_t *g0i = P.gidx[cur]; const double *g0v = P.gvals[cur];
        for (int e = tid; e < ngl; e += 1024) {
            const int64_t j = g_idx[e];
            int64_t a = 0, b = g0n;
            while (a < b) { const int64_t mid = (a + b) >> 1; if (g0i[mid] < j) a = mid + 1; else b = mid; }
            const double v0 = (a < g0n && g0i[a] == j) ? g0v[a] : 0.0;
            dmax = fmax(dmax, fabs(g_val[e] - v0));
            P.gidx[nw][e] = j; P.gvals[nw][e] = g_val[e];
        }
        for (int64_t t = tid; t < g0n; t += 1024) {
            const int64_t j = g0i[t]; const double v0 = g0v[t];
            nbm = fmax(nbm, fabs(v0));
            int a = 0, b = ngl;
            while (a < b) { const int mid = (a + b) >> 1; if (g_idx[mid] < j) a = mid + 1; else b = mid; }
            if (!(a < ngl && g_idx[a] == j)) dmax = fmax(dmax, fabs(0.0 - v0));
        }
        if (tid < q) { dmax = fmax(dmax, fabs(c_new[tid] - m0.c[tid])); nbm = fmax(nbm, fabs(m0.c[tid])); }
    }
    dmax = res_wave_max(dmax); nbm = res_wave_max(nbm);
    if ((tid & 63) == 0) { red_d[tid >> 6] = dmax; red_n[tid >> 6] = nbm; }
    __syncthreads();
    if (tid == 0) for (int wv = 1; wv < 16; ++wv) { red_d[0] = fmax(red_d[0], red_d[wv]); red_n[0] = fmax(red_n[0], red_n[wv]); }
    if (!why && tid == 0) {
        const int nf = nfr;
        int sl = 0, given = 0;
        for (; given < nf && sl < M.slots; ++sl)
            if (!((busy[sl >> 5] >> (sl & 31)) & 1u)) { slot1[fresh_t[given]] = sl; ++given; }
        // (free slots cannot run out: k_res_select_local made sure cnt0 + its whole local list fit)
        for (int e = 0; e < nf; ++e) P.fresh[nw][e] = fresh_t[e];
        ctl->nfresh[nw] = nf;
        ResModel &m1 = ctl->m[nw];
        m1.cnt = nsnp; m1.idc = idc_new;
        for (int l = 0; l < kMaxQ; ++l) m1.c[l] = l < q ? c_new[l] : 0.0;
        ctl->gcnt[nw] = ngl;
        ctl->tol = red_d[0] / (red_n[0] + 1.0);
    }
    __syncthreads();
    if (why && tid == 0) {
        ctl->live_epoch = why == 5 ? res_gate_attempt(epoch + 1) : res_gate_step(epoch + 1);
        res_publish(P.rec, seq, why == 5 ? RES_REDO_SLOW : RES_ABORT, 0.0, 0.0, eta, ctl->es, ctl->iter, cur, why);
    }
}

// sum over the support of df^2 in list order into dst (k_sumsq_seq with the list's length on the device): the shard's share of
// iht_stepsize!'s numerator, which rides the all-reduce of X_S g_S as element n
static __global__ void k_res_sumsq(ResPtrs P, int epoch, double *__restrict__ dst)
{
    const ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, -1)) return;
    const int64_t cnt = ctl->m[ctl->cur].cnt;
    double a = 0.0;
    for (int64_t t = 0; t < cnt; ++t) a += P.gval[t] * P.gval[t];
    *dst = a;
}

// update_xb! (utilities.jl:93-118), update_mu! and the loglikelihood sums of the candidate: k_xv_snp_cached + k_zmul + k_mu_loglik
// in one sweep over the rows.  SPLIT as in k_res_xgk (k_res_missing, then k_res_mu).
template <bool WIDE = false>
__device__ __forceinline__ void res_mu_rows(const ResPtrs &P, double xbv, int64_t i, const double *__restrict__ z, const double *__restrict__ y,
                                            const double *__restrict__ w, int64_t n, int q, int dist, int link, double nb_r,
                                            double *xb, double *__restrict__ zc, double *__restrict__ mu, double *__restrict__ red,
                                            double *__restrict__ rout /* the working residual of score! for this candidate (read only if it stands) */,
                                            int lean = 0 /* Normal / identity on the plain path: nothing on the device reads xb, zc or mu before the
                                                            iterate goes home (the step-size weights are w, the residual is written here), and
                                                            res_end forms them again from the model: 12 MB of cold stores per attempt less */)
{
    const ResCtl *ctl = P.ctl;
    const int clamp = dist != MIH_NORMAL;
    const ResModel &m1 = ctl->m[1 - ctl->cur];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        if (clamp) xbv = xbv < -20.0 ? -20.0 : (xbv > 20.0 ? 20.0 : xbv);
        double a = 0.0;
        for (int l = 0; l < q; ++l) a += z[(int64_t)l * n + i] * m1.c[l];
        if (clamp) a = a < -20.0 ? -20.0 : (a > 20.0 ? 20.0 : a);
        const double eta = xbv + a;
        const double m = d_linkinv(link, eta);
        if (!lean) { xb[i] = xbv; zc[i] = a; mu[i] = m; }
        const double wt = w[i], yi = y[i];
        rout[i] = d_mueta(link, eta) / d_glmvar(dist, m, nb_r) * (yi - m) * wt;      // k_resid's expression (utilities.jl:128-132), from the values at hand
        v[0] = wt * d_devresid(dist, yi, m, nb_r);
        if (dist == MIH_GAMMA) { v[1] = wt * (log(m) + yi / m); v[3] = wt * log(yi); }
        else if (dist == MIH_INVGAUSS) v[3] = wt * log(6.283185307179586 * yi * yi * yi);
        else if (dist != MIH_NORMAL) v[1] = wt * d_loglik_obs(dist, yi, m, nb_r);
        v[2] = wt;
    }
    if (WIDE) res_block_sum_wide<4>(v, red, (int)((n + 255) / 256));
    else block_sum<4>(v, red + 4ll * blockIdx.x);
}
template <bool SPLIT>
__device__ __forceinline__ void
b_res_xb(ResPtrs P, int epoch, int attempt, ResMat M, const double *__restrict__ z, const double *__restrict__ y, const double *__restrict__ w,
         int q, int dist, int link, double nb_r, double *__restrict__ xb, double *__restrict__ zc, double *__restrict__ mu,
         double *__restrict__ red, double *__restrict__ rout, int lean)
{
    const ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    extern __shared__ double res_part[];
    const int nw = 1 - ctl->cur;
    const double a = res_xv_rows_wide(M, P.idx[nw], P.slot[nw], P.fresh[nw], ctl->nfresh[nw], P.coefA, P.coefB, ctl->m[nw].cnt, res_part);
    const int64_t i = blockIdx.x * 1024ll + threadIdx.x;
    if (SPLIT) { if (i < M.n) xb[i] = a; return; }
    res_mu_rows<true>(P, a, i, z, y, w, M.n, q, dist, link, nb_r, xb, zc, mu, red, rout, lean);
}
__device__ __forceinline__ void
b_res_mu(ResPtrs P, int epoch, int attempt, const double *src /* X_S b_S before the clamp: xb itself, or the summed shards */,
         const double *__restrict__ z, const double *__restrict__ y, const double *__restrict__ w, int64_t n,
         int q, int dist, int link, double nb_r, double *xb, double *__restrict__ zc, double *__restrict__ mu,
         double *__restrict__ red, double *__restrict__ rout)
{
    if (res_dead(P.ctl, epoch, attempt)) return;
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    res_mu_rows(P, i < n ? src[i] : 0.0, i, z, y, w, n, q, dist, link, nb_r, xb, zc, mu, red, rout);
}

// One workgroup: the loglikelihood of the candidate (utilities.jl:9-20 from the block sums, as IhtVar::mu_loglik assembles it),
// the decision of _iht_backtrack_ (utilities.jl:484: old_logl > new_logl && backtracks < max_step) and -- when the step stands --
// the flip of the iterate, the stopping rules and the step's record for the host.
__device__ __forceinline__ void
b_res_decide(ResPtrs P, int epoch, int attempt, int next_attempt_queued, uint64_t seq, const double *__restrict__ red, int nb, int64_t n, int dist)
{
#pragma clang fp contract(off)
    ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, attempt)) return;
    __shared__ double sred[4][256];
    double o[4];
    res_final_sums<4>(red, nb, o, sred);
    if (threadIdx.x != 0) return;
    double logl;
    if (dist == MIH_NORMAL) {
        const double phi = o[0] / (double)n, sd = sqrt(phi);
        logl = -(o[0] / (sd * sd) + o[2] * 1.8378770664093454835606594728112) / 2.0 - o[2] * scalar_log(sd);       // (scalar_log.h: the same bits as IhtVar::mu_loglik's on the host)
    } else if (dist == MIH_GAMMA) {
        const double phi = o[0] / (double)n, a = 1.0 / phi;
        logl = -o[2] * (lgamma(a) + a * scalar_log(phi)) - a * o[1] + (a - 1.0) * o[3];
    } else if (dist == MIH_INVGAUSS) {
        const double lam = (double)n / o[0];
        logl = 0.5 * scalar_log(lam) * o[2] - 0.5 * o[3] - 0.5 * lam * o[0];
    } else logl = o[1];
    const int es = ctl->es, cur = ctl->cur;
    const double eta = res_halved(ctl->eta, es);
    if (ctl->logl_cur > logl && es < ctl->max_step) {
        // the next attempt slot in the stream takes over: right behind, or -- this was the last slot of its series -- behind the
        // step-end and step-start kernels queued in between, which do nothing in this phase.  The host learns that the series
        // ended without a step (one record per series, whatever happened in it)
        ctl->es = es + 1;
        if (!next_attempt_queued) res_publish(P.rec, seq, RES_PENDING, logl, ctl->tol, eta, es + 1, ctl->iter, cur, ctl->m[1 - cur].cnt);
        return;
    }
    const int iter = ctl->iter + 1;
    int status = RES_ACCEPT;
    if (isnan(logl)) status = RES_STOP_NAN;
    else if (isinf(logl)) status = RES_STOP_INF;
    else if (ctl->arm_stop && iter >= ctl->min_iter && ctl->tol < ctl->tol_stop) status = RES_STOP_CONVERGED;
    ctl->cur = 1 - cur; ctl->logl_cur = logl; ctl->es = 0; ctl->iter = iter;
    ctl->nfresh[0] = 0; ctl->nfresh[1] = 0;          // (the columns of both lists are in the cache by now)
    ctl->live_epoch = res_gate_step(status == RES_ACCEPT ? epoch : epoch + 1);       // the step's end and the next one's start are on; or all is off
    res_publish(P.rec, seq, status, logl, ctl->tol, eta, es, iter, 1 - cur, ctl->m[1 - cur].cnt);
}

// ---- the kernels: each body above (b_res_*) as a launch of its own, for ONE fit --------------------------------------------------
static __global__ void __launch_bounds__(256)
k_res_support(ResPtrs P, int epoch, ResMat M, const double *__restrict__ df)
{
    b_res_support(P, epoch, M, df);
}
static __global__ void __launch_bounds__(1024)
k_res_missing(ResPtrs P, int epoch, int attempt, int which , ResMat M, double *__restrict__ out)
{
    b_res_missing(P, epoch, attempt, which, M, out);
}
static __global__ void __launch_bounds__(256)
k_res_eta(ResPtrs P, int epoch, const double *__restrict__ red, int nb, int q, const double *numer_snp)
{
    b_res_eta(P, epoch, red, nb, q, numer_snp);
}
template <bool SPLIT>
__global__ void __launch_bounds__(1024, 8)
k_res_xgk(ResPtrs P, int epoch, ResMat M, const double *__restrict__ z, const double *__restrict__ xb, const double *__restrict__ zc,
          const double *__restrict__ mu, const double *__restrict__ w, int q, int dist, int link, double nb_r,
          double *__restrict__ xgk, double *__restrict__ red)
{
    b_res_xgk<SPLIT>(P, epoch, M, z, xb, zc, mu, w, q, dist, link, nb_r, xgk, red);
}
static __global__ void __launch_bounds__(256)
k_res_stepsize(ResPtrs P, int epoch, const double *__restrict__ xgk, const double *__restrict__ z, const double *__restrict__ xb,
               const double *__restrict__ zc, const double *__restrict__ mu, const double *__restrict__ w, int64_t n, int q,
               int dist, int link, double nb_r, double *__restrict__ red)
{
    b_res_stepsize(P, epoch, xgk, z, xb, zc, mu, w, n, q, dist, link, nb_r, red);
}
template <bool FAST>
__global__ void __launch_bounds__(256)
k_res_grad(ResPtrs P, int epoch, int attempt, const double *__restrict__ df, const double *__restrict__ weight, int64_t p, int q, uint64_t zkeep,
           int64_t sel_len ,
           double *__restrict__ full)
{
    b_res_grad<FAST>(P, epoch, attempt, df, weight, p, q, zkeep, sel_len, full);
}
static __global__ void __launch_bounds__(256)
k_res_hist2(ResPtrs P, int epoch, int attempt, const double *__restrict__ full, int64_t len, uint64_t K)
{
    b_res_hist2(P, epoch, attempt, full, len, K);
}
static __global__ void __launch_bounds__(256)
k_res_collect(ResPtrs P, int epoch, int attempt, const double *__restrict__ full, int64_t len)
{
    b_res_collect(P, epoch, attempt, full, len);
}
static __global__ void __launch_bounds__(1024)
k_res_select(ResPtrs P, int epoch, int attempt, int fast, uint64_t K, uint64_t seq, ResMat M, const double *__restrict__ weight, int64_t p, int q,
             uint64_t zkeep, int zkeepn, int64_t max_nonzero ,
             int force_abort_es)
{
    b_res_select(P, epoch, attempt, fast, K, seq, M, weight, p, q, zkeep, zkeepn, max_nonzero, force_abort_es);
}
static __global__ void __launch_bounds__(1024)
k_res_select_big(ResPtrs P, int epoch, int attempt, int fast, uint64_t K, uint64_t seq, ResMat M, const double *__restrict__ weight, int64_t p, int q,
             uint64_t zkeep, int zkeepn, int64_t max_nonzero ,
             int force_abort_es)
{
    b_res_select<true>(P, epoch, attempt, fast, K, seq, M, weight, p, q, zkeep, zkeepn, max_nonzero, force_abort_es);
}
template <bool SPLIT>
__global__ void __launch_bounds__(1024, 8)
k_res_xb(ResPtrs P, int epoch, int attempt, ResMat M, const double *__restrict__ z, const double *__restrict__ y, const double *__restrict__ w,
         int q, int dist, int link, double nb_r, double *__restrict__ xb, double *__restrict__ zc, double *__restrict__ mu,
         double *__restrict__ red, double *__restrict__ rout, int lean)
{
    b_res_xb<SPLIT>(P, epoch, attempt, M, z, y, w, q, dist, link, nb_r, xb, zc, mu, red, rout, lean);
}
static __global__ void __launch_bounds__(256)
k_res_mu(ResPtrs P, int epoch, int attempt, const double *src ,
         const double *__restrict__ z, const double *__restrict__ y, const double *__restrict__ w, int64_t n,
         int q, int dist, int link, double nb_r, double *xb, double *__restrict__ zc, double *__restrict__ mu,
         double *__restrict__ red, double *__restrict__ rout)
{
    b_res_mu(P, epoch, attempt, src, z, y, w, n, q, dist, link, nb_r, xb, zc, mu, red, rout);
}
static __global__ void __launch_bounds__(256)
k_res_decide(ResPtrs P, int epoch, int attempt, int next_attempt_queued, uint64_t seq, const double *__restrict__ red, int nb, int64_t n, int dist)
{
    b_res_decide(P, epoch, attempt, next_attempt_queued, seq, red, nb, n, dist);
}

// Z'r (utilities.jl:134) and the statistics of r the fixed-point pass needs (max |r|, sum r: k_r_stats) for the iterate that stood.
// The working residual itself (utilities.jl:128-132) is written by the attempt's own sweep (res_mu_rows: y, mu, w and eta are in
// registers there), so this kernel reads r and Z only: 8 MB instead of the 32-44 MB of the first version, which formed r from
// xb, zc, y, mu, w once for the statistics and once more per covariate -- after the 125 GB pass nothing of a fit's vectors is left
// in a cache, and a sweep over cold vectors costs what its bytes cost (~3-5 TB/s: tools/sweep_probe.hip, the timestamps of round 5).
// Same partial sums, same order of additions as k_zt_r (128 strided blocks per covariate) and k_r_stats (64 strided blocks): walker
// (b, t) of k_r_stats visits rows 256 b + t + 16384 k; its even visits are walker (b, t) of k_zt_r, its odd ones walker (b + 64, t).
// The second stage of both (64 and 128 partials) is left to the kernels behind: k_digits' blocks redo the statistics' for
// themselves, its block 0 also Z'r.
// block_sum's tree over the 256 walkers of one block, by ONE wave that holds walker l, l + 64, l + 128, l + 192 in lane l: the same
// pairs in the same order (red[t] += red[t + s] for s = 128, 64, ..., 1), the result in lane 0
__device__ __forceinline__ double res_tree256_sum(double v0, double v1, double v2, double v3)
{
    double x = (v0 + v2) + (v1 + v3);              // s = 128: t + (t+128); s = 64: (t) + (t+64)
    for (int st = 32; st > 0; st >>= 1) { const double o = __shfl_down(x, st, 64); x = x + o; }      // (lanes >= st hold values nobody reads)
    return x;
}
__device__ __forceinline__ double res_tree256_max(double v0, double v1, double v2, double v3)
{
    double x = fmax(fmax(v0, v2), fmax(v1, v3));
    for (int st = 32; st > 0; st >>= 1) x = fmax(x, __shfl_down(x, st, 64));
    return x;
}
// A walk's 256 walkers are spread over FOUR single-wave workgroups (a 64-workgroup launch leaves three quarters of the chip idle);
// the wave that finishes last of its four -- a ticket per walk-block: four increments on an address of its own, nothing a whole
// grid shares -- does the block's 256-trees.  The walkers' sums go out as device-scope stores, then a device-scope RELEASE, then
// the ticket; the last wave ACQUIRES before it reads.  On this chip a device-scope release writes back the XCD's L2
// (buffer_wbl2): dear when the kernel has megabytes of dirty lines -- 768 waves doing it one after the other behind a kernel
// that also wrote r cost 45 us, which is what made the last-block tickets of the chain's first version so dear -- and cheap
// here, where nothing but these sums is written (12 us for the whole kernel).  A workgroup-scope fence is NOT enough: it compiles
// to nothing for global stores, the ticket overtook the sums now and then, and a stale partial of the step before gave Z'r a
// relative error of 1e-6 (caught by test_large_k_and_many_covariates in one run of three).
// grid (4 * kStatBlocks, ceil(q / 4)) x 64 threads: slice y takes covariates 4y .. 4y + 3 (slice 0 also the statistics).
// walk: [slices][kStatBlocks][10][256] doubles (sum, max, 2 x 4 covariate sums), tick: [slices][kStatBlocks] zeros.
constexpr int kResStatCov = 4;
static __global__ void __launch_bounds__(64)
k_res_stats(ResPtrs P, int epoch, const double *__restrict__ z, const double *__restrict__ r, int64_t n, int q,
            double *__restrict__ zpart, double *__restrict__ spart, double *__restrict__ walk, unsigned *__restrict__ tick)
{
    const ResCtl *ctl = P.ctl;
    if (res_dead(ctl, epoch, -1)) return;
    const int slice = blockIdx.y, blk = blockIdx.x >> 2, t = (blockIdx.x & 3) * 64 + threadIdx.x;      // walker t of walk-block blk
    const int l0 = slice * kResStatCov, nl = q - l0 < kResStatCov ? q - l0 : kResStatCov;
    const bool stats = slice == 0;
    const int64_t stride = 256ll * kStatBlocks;
    double mx = 0.0, sm = 0.0, za[2][kResStatCov];
    #pragma unroll
    for (int c = 0; c < kResStatCov; ++c) { za[0][c] = 0.0; za[1][c] = 0.0; }
    // sixteen rows (two rounds of eight visits: even, odd, even, ...) in flight per thread
    for (int64_t i = blk * 256ll + t; i < n; i += 16 * stride) {
        double rv[16], zv[kResStatCov][16];
        #pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int64_t iu = i + u * stride;
            const bool on = iu < n;
            rv[u] = on ? r[iu] : 0.0;
            #pragma unroll
            for (int c = 0; c < kResStatCov; ++c) zv[c][u] = (on && c < nl) ? z[(int64_t)(l0 + c) * n + iu] : 0.0;
        }
        #pragma unroll
        for (int u = 0; u < 16; ++u) if (i + u * stride < n) {
            if (stats) { mx = fmax(mx, fabs(rv[u])); sm += rv[u]; }
            #pragma unroll
            for (int c = 0; c < kResStatCov; ++c) za[u & 1][c] += zv[c][u] * rv[u];      // (sixteen visits per round: the parity of u is the parity of the visit)
        }
    }
    double *mine = walk + ((size_t)slice * kStatBlocks + blk) * 10 * 256;
    __hip_atomic_store(&mine[t], sm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&mine[256 + t], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    #pragma unroll
    for (int c = 0; c < kResStatCov; ++c) {
        __hip_atomic_store(&mine[(2 + c) * 256 + t], za[0][c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&mine[(6 + c) * 256 + t], za[1][c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    unsigned ticket = 0;
    if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(&tick[(size_t)slice * kStatBlocks + blk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __shfl(ticket, 0, 64);
    if (ticket != 3u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int l = threadIdx.x;
    auto four = [&](int plane, double (&o)[4]) {
        #pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __hip_atomic_load(&mine[plane * 256 + l + 64 * e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    double v4[4];
    if (stats) {
        four(0, v4); const double total = res_tree256_sum(v4[0], v4[1], v4[2], v4[3]);
        four(1, v4); const double top = res_tree256_max(v4[0], v4[1], v4[2], v4[3]);
        if (l == 0) { spart[blk * 2] = top; spart[blk * 2 + 1] = total; }
    }
    for (int c = 0; c < nl; ++c) {
        four(2 + c, v4); const double even = res_tree256_sum(v4[0], v4[1], v4[2], v4[3]);
        four(6 + c, v4); const double odd = res_tree256_sum(v4[0], v4[1], v4[2], v4[3]);
        if (l == 0) { zpart[(int64_t)(l0 + c) * kZtrBlocks + blk] = even; zpart[(int64_t)(l0 + c) * kZtrBlocks + blk + kStatBlocks] = odd; }
    }
    if (l == 0) tick[(size_t)slice * kStatBlocks + blk] = 0;
}

// (round 6) The outlier side channel of the fixed-point residual (peel.h) in the resident chain: ONE workgroup between k_res_stats and
// the digit kernel looks at the 64 block maxima k_res_stats left -- the same numbers, hence the same decision, as k_r_stats's last
// block in the host-driven step.  No outlier (every step of an ordinary fit): it returns after a few hundred nanoseconds of work
// and k_digits' blocks take the scale from max|r| as before; else it lists the rows that leave the fixed point and k_digits' blocks
// read the scale of the rest from its record.
static __global__ void __launch_bounds__(1024)
k_res_peel(ResPtrs P, int epoch, const double *__restrict__ r, int64_t n, const double *__restrict__ spart, double *__restrict__ pl)
{
    if (res_dead(P.ctl, epoch, -1)) return;
    const int64_t nb64 = (n + 255) / 256;
    (void)peel_decide(r, n, spart, (int)(nb64 < kStatBlocks ? nb64 : kStatBlocks), pl);
}
