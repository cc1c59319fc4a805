// assoc_sets.hip -- gene-based burden and SKAT tests of variant sets on top of the marginal association scan (mih_assoc_sets).
// tests/sets_spec.py states the definitions in numpy; include/mendeliht_hip.h has them in full.
//
// Per set the tests need the joint covariance of the members' scores under the null model, K = X~'WX~ - (L^-1 b)(L^-1 b)': a
// weighted Gram matrix of up to 128 decoded columns, adjusted for the covariates.  The pass runs after the scan's finish, whose
// S = [U | b], V and Linv it reads on the device:
//   k_assoc_set_u     u_j = L^-1 b_j of every entry, in the order of k_assoc_var
//   k_assoc_set_gram  one workgroup per set: the members (entries that are not degenerate, omega > 0), their x~ decoded chunk by
//                     chunk into LDS, C = X~'WX~ on the f64 matrix cores
//   k_assoc_set_k     K from C and u (diagonal: the scan's V), mirrored; T, S and Q of the set
//   k_assoc_set_eig   the eigenvalues of M = diag(omega) K diag(omega): parallel-order Jacobi, one workgroup per set
// and the host finishes with mixture_tail.h.  Nothing in it depends on slice_rows, on the position of a set in the list or on the
// other sets of the call: every C_jk is ONE chain of fused multiply-adds over the rows in ascending order (no split over rows, no
// atomics), everything after it has a fixed operation order with contraction off.
#include "assoc_set_eig.h"
#include "assoc_slab.h"
#include "mixture_tail.h"
#include <cmath>
#include <limits>

namespace mih {

typedef double set_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kSetChunk = 32;                    // rows of a decode chunk: eight k-steps of v_mfma_f64_16x16x4_f64
constexpr int kSetLd = kSymEigMaxOrder + 16;     // doubles between two rows of the chunk in LDS: 288 dwords = 32 banks mod 64, so the
                                                 // four row groups of a fragment read (lane >> 4) fall on the two halves of the banks
constexpr int kSetBlocksPerWave = 9;             // 8 x 9 / 2 = 36 lower-triangular 16 x 16 blocks over four waves

// ---- u ---------------------------------------------------------------------------------------------------------------------------------
// one thread per entry e: Ub[e c + k] = sum_{l <= k} Linv[k][l] b_l of column set_col[e], l ascending (k_assoc_var's expression)
__global__ void __launch_bounds__(256)
k_assoc_set_u(const double *__restrict__ S, int64_t p, int c, const double *__restrict__ Linv, const int32_t *__restrict__ set_col, int64_t nent,
              double *__restrict__ Ub)
{
#pragma clang fp contract(off)
    const int64_t e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= nent) return;
    const int64_t j = set_col[e];
    for (int k = 0; k < c; ++k) {
        double u = 0.0;
        for (int l = 0; l <= k; ++l) u = u + Linv[k * c + l] * S[(int64_t)(1 + l) * p + j];
        Ub[e * c + k] = u;
    }
}

// ---- the Gram ------------------------------------------------------------------------------------------------------------------------
// One workgroup (four waves) per set s with entries e0 .. e0 + ms.  Thread 0 lists the members in entry order (mlist[e0 + r]: the
// entry of member r; m_used[s] = m).  Then, chunk of kSetChunk rows by chunk, the members' x~ are decoded into xs[row][member]
// (members >= m of the last block and rows >= n are zero) and every wave runs its lower-triangular blocks (bi, bj), bj <= bi,
// linear index wave + 4 q, through eight MFMAs: lane l gives A[l & 15][l >> 4] = x~[row 4 kk + (l >> 4)][member 16 bi + (l & 15)]
// w[row] (ONE operand is scaled) and B[l >> 4][l & 15] = x~[same row][member 16 bj + (l & 15)], and holds
// D[(l >> 4) + 4 reg][l & 15] -- the C/D map grm.hip documents.  C_jk (j > k) goes to Kb[koff[s] + j m + k]: compact, m x m.
template <int KIND>      // 0: f64, 1: f32, 2: dosage, 3: 2-bit
__global__ void __launch_bounds__(256)
k_assoc_set_gram(ColView mt, int64_t n, const int64_t *__restrict__ set_ptr, const int32_t *__restrict__ set_col, const double *__restrict__ omega,
                 const double *__restrict__ V, const double *__restrict__ w, const int64_t *__restrict__ koff, int32_t *__restrict__ m_used,
                 int32_t *__restrict__ mlist, double *__restrict__ Kb)
{
#pragma clang fp contract(off)
    __shared__ double xs[kSetChunk * kSetLd];
    __shared__ double ws[kSetChunk];
    __shared__ int32_t mcol[kSymEigMaxOrder];
    __shared__ int sm;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t s = blockIdx.x, e0 = set_ptr[s];
    const int ms = min((int)(set_ptr[s + 1] - e0), kSymEigMaxOrder);
    if (tid == 0) {
        int m = 0;
        for (int e = 0; e < ms; ++e) {
            const int32_t col = set_col[e0 + e];
            const double v = V[col];
            if (v == v && omega[e0 + e] > 0.0) { mcol[m] = col; mlist[e0 + m] = e; ++m; }
        }
        sm = m;
        m_used[s] = m;
    }
    __syncthreads();
    const int m = sm;
    if (m == 0) return;
    const int nb = (m + 15) >> 4, nblk = nb * (nb + 1) / 2, mp = nb * 16;

    // the blocks of this wave
    int bi[kSetBlocksPerWave], bj[kSetBlocksPerWave];
    set_f64x4 acc[kSetBlocksPerWave];
    #pragma unroll
    for (int q = 0; q < kSetBlocksPerWave; ++q) {
        const int b = wv + 4 * q;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= b) ++r;
        bi[q] = r; bj[q] = b - r * (r + 1) / 2;
        acc[q] = set_f64x4{0.0, 0.0, 0.0, 0.0};
    }

    // 2-bit: thread (member tid & 127, half tid >> 7) decodes 16 rows of its member from one dword; the threads of the first half
    // walk their member's missing list with a cursor (the list is ascending)
    const int mem3 = tid & 127, hf = tid >> 7;
    SnpVals sv = {0.0, 0.0, 0.0, 0.0};
    int64_t col3 = 0, cur = 0, cend = 0;
    if (KIND == 3 && mem3 < m) {
        col3 = mcol[mem3];
        sv = snp_vals(mt, col3);
        if (hf == 0) { cur = mt.miss_ptr[col3]; cend = mt.miss_ptr[col3 + 1]; }
    }

    for (int64_t r0 = 0; r0 < n; r0 += kSetChunk) {
        __syncthreads();                                      // the previous chunk has been multiplied
        if (tid < kSetChunk) ws[tid] = r0 + tid < n ? w[r0 + tid] : 0.0;
        if (KIND == 3) {
            if (mem3 < mp) {
                const int64_t rb = r0 + 16 * hf;
                uint32_t word = 0u;
                if (mem3 < m && rb < n) word = mt.X[xword(mt.nbp, col3, rb >> 4)];
                #pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uint32_t g = (word >> (2 * k)) & 3u;
                    const double x = g == 0u ? sv.x0 : g == 1u ? sv.x1 : sv.x2;
                    xs[(16 * hf + k) * kSetLd + mem3] = (mem3 < m && rb + k < n) ? x : 0.0;
                }
            }
            __syncthreads();
            if (hf == 0 && mem3 < m)
                while (cur < cend) {
                    const int64_t row = mt.miss_row[cur];
                    if (row >= r0 + kSetChunk) break;
                    if (row >= r0 && row < n) xs[(int)(row - r0) * kSetLd + mem3] = sv.xm;
                    ++cur;
                }
        } else {
            const int row = tid & (kSetChunk - 1);
            const int64_t i = r0 + row;
            for (int mem = tid >> 5; mem < mp; mem += 8)
                xs[row * kSetLd + mem] = (mem < m && i < n) ? slab_dense_x<KIND>(mt, n, (int64_t)mcol[mem], i) : 0.0;
        }
        __syncthreads();
        #pragma unroll
        for (int kk = 0; kk < kSetChunk / 4; ++kk) {
            const int row = 4 * kk + (lane >> 4);
            const double wr = ws[row];
            const double *xr = xs + row * kSetLd + (lane & 15);
            #pragma unroll
            for (int q = 0; q < kSetBlocksPerWave; ++q)
                if (wv + 4 * q < nblk)
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[16 * bi[q]] * wr, xr[16 * bj[q]], acc[q], 0, 0, 0);
        }
    }

    double *out = Kb + koff[s];
    #pragma unroll
    for (int q = 0; q < kSetBlocksPerWave; ++q)
        if (wv + 4 * q < nblk) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * bi[q] + (lane >> 4) + 4 * r, k = 16 * bj[q] + (lane & 15);
                if (j < m && k < j) out[j * m + k] = acc[q][r];
            }
        }
}

// ---- K, T, S, Q --------------------------------------------------------------------------------------------------------------------------
// One workgroup per set.  K_jk = C_jk - sum_l u_jl u_kl (l ascending from 0.0) for j > k, written to both triangles; K_jj = V_j.
// Then rs_j = sum_k M_jk (k ascending), S = sum_j rs_j (j ascending); with a_j = omega_j U_j: T = sum_j a_j, Q = sum_j a_j a_j.
// stat[3 s ..] = T, S, Q (zeros for a set without members).
__global__ void __launch_bounds__(256)
k_assoc_set_k(const int64_t *__restrict__ set_ptr, const int32_t *__restrict__ set_col, const double *__restrict__ omega, const double *__restrict__ S,
              const double *__restrict__ V, int c, const double *__restrict__ Ub, const int64_t *__restrict__ koff, const int32_t *__restrict__ m_used,
              const int32_t *__restrict__ mlist, double *__restrict__ Kb, double *__restrict__ stat)
{
#pragma clang fp contract(off)
    __shared__ int ent[kSymEigMaxOrder];
    __shared__ double om[kSymEigMaxOrder], rs[kSymEigMaxOrder];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x, e0 = set_ptr[s];
    const int m = min(m_used[s], kSymEigMaxOrder);
    if (m <= 0) {
        if (tid < 3) stat[3 * s + tid] = 0.0;
        return;
    }
    if (tid < m) { ent[tid] = mlist[e0 + tid]; om[tid] = omega[e0 + ent[tid]]; }
    __syncthreads();
    double *K = Kb + koff[s];
    for (int idx = tid; idx < m * m; idx += 256) {
        const int j = idx / m, k = idx % m;
        if (k < j) {
            const double *uj = Ub + (e0 + ent[j]) * c, *uk = Ub + (e0 + ent[k]) * c;
            double dot = 0.0;
            for (int l = 0; l < c; ++l) dot = dot + uj[l] * uk[l];
            const double v = K[j * m + k] - dot;
            K[j * m + k] = v;
            K[k * m + j] = v;
        } else if (k == j) K[j * m + j] = V[set_col[e0 + ent[j]]];
    }
    __syncthreads();
    if (tid < m) {
        double a = 0.0;
        for (int k = 0; k < m; ++k) a = a + set_m_entry(K, m, om, tid, k);
        rs[tid] = a;
    }
    __syncthreads();
    if (tid == 0) {
        double ss = 0.0, t = 0.0, q = 0.0;
        for (int j = 0; j < m; ++j) {
            const double a = om[j] * S[set_col[e0 + ent[j]]];
            ss = ss + rs[j]; t = t + a; q = q + a * a;
        }
        stat[3 * s] = t; stat[3 * s + 1] = ss; stat[3 * s + 2] = q;
    }
}

// ---- the eigenvalues ---------------------------------------------------------------------------------------------------------------------
// One workgroup per set: the eigenvalues of M (m x m), descending, every value <= 0 set to 0, into lam[e0 ..]; NaN after m.
// The iteration is set_jacobi_eig (assoc_set_eig.h).  The matrix lives in LDS up to kSetEigLds members, in the set's slab of Mb
// (moff[s], (ms + 1)^2 doubles) beyond.
__global__ void __launch_bounds__(256)
k_assoc_set_eig(const int64_t *__restrict__ set_ptr, const double *__restrict__ omega, const int64_t *__restrict__ koff, const int64_t *__restrict__ moff,
                const int32_t *__restrict__ m_used, const int32_t *__restrict__ mlist, const double *__restrict__ Kb, double *__restrict__ Mb,
                double *__restrict__ lam)
{
#pragma clang fp contract(off)
    __shared__ double sa[kSetEigLds * (kSetEigLds + 1)];
    __shared__ double om[kSymEigMaxOrder];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x, e0 = set_ptr[s];
    const int ms = min((int)(set_ptr[s + 1] - e0), kSymEigMaxOrder);
    const int m = min(m_used[s], ms);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int i = tid; i < ms; i += 256) if (i >= m) lam[e0 + i] = nan;
    if (m <= 0) return;
    const int me = (m + 1) & ~1, lda = m <= kSetEigLds ? kSetEigLds + 1 : me;
    double *a = m <= kSetEigLds ? sa : Mb + moff[s];
    if (tid < m) om[tid] = omega[e0 + mlist[e0 + tid]];
    __syncthreads();
    const double *K = Kb + koff[s];
    double f2 = 0.0;
    for (int idx = tid; idx < me * me; idx += 256) {
        const int i = idx / me, j = idx % me;
        const double v = (i < m && j < m) ? set_m_entry(K, m, om, i, j) : 0.0;
        a[i * lda + j] = v;
        f2 = f2 + v * v;
    }
    set_jacobi_eig(a, lda, m, f2, lam + e0);
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------
int assoc_sets_check(const SetsCall &sc, int64_t p)
{
    if (sc.skato) MIH_TRY(assoc_skato_check(*sc.skato));
    if (sc.nsets < 0) { set_error("mih_assoc_sets: nsets must not be negative, got %d", (int)sc.nsets); return MIH_BAD_ARG; }
    if (!sc.set_ptr || !sc.m_used || !sc.burden_z || !sc.neglog10p_burden || !sc.skat_q || !sc.neglog10p_skat || !sc.skat_state) {
        set_error("mih_assoc_sets: null argument"); return MIH_BAD_ARG;
    }
    if (sc.set_ptr[0] != 0) { set_error("mih_assoc_sets: set_ptr must start at 0, got %lld", (long long)sc.set_ptr[0]); return MIH_BAD_ARG; }
    for (int32_t s = 0; s < sc.nsets; ++s) {
        const int64_t len = sc.set_ptr[s + 1] - sc.set_ptr[s];
        if (len < 0) { set_error("mih_assoc_sets: set_ptr decreases at set %d", (int)s + 1); return MIH_BAD_ARG; }
        if (len > kSymEigMaxOrder) {
            set_error("mih_assoc_sets: set %d has %lld entries, at most %d are supported", (int)s + 1, (long long)len, kSymEigMaxOrder);
            return MIH_BAD_ARG;
        }
    }
    const int64_t nent = sc.set_ptr[sc.nsets];
    if (nent > 0 && (!sc.set_col || !sc.omega)) { set_error("mih_assoc_sets: null argument"); return MIH_BAD_ARG; }
    for (int32_t s = 0; s < sc.nsets; ++s)
        for (int64_t e = sc.set_ptr[s]; e < sc.set_ptr[s + 1]; ++e) {
            const int64_t col = sc.set_col[e];
            if (col < 0 || col >= p) { set_error("mih_assoc_sets: set %d names column %lld, outside [0, %lld)", (int)s + 1, (long long)col, (long long)p); return MIH_BAD_ARG; }
            if (e > sc.set_ptr[s] && sc.set_col[e - 1] >= col) { set_error("mih_assoc_sets: the columns of set %d are not strictly ascending", (int)s + 1); return MIH_BAD_ARG; }
            if (!(sc.omega[e] >= 0.0) || !std::isfinite(sc.omega[e])) { set_error("mih_assoc_sets: weight %lld of set %d is negative or not finite", (long long)(e - sc.set_ptr[s]) + 1, (int)s + 1); return MIH_BAD_ARG; }
        }
    return MIH_OK;
}

// the offsets of the sets' K (ms^2 doubles each) and Jacobi slabs ((ms + 1)^2, sets of more than kSetEigLds entries only)
static void sets_offsets(const SetsCall &sc, std::vector<int64_t> &koff, std::vector<int64_t> &moff)
{
    koff.assign((size_t)sc.nsets + 1, 0); moff.assign((size_t)sc.nsets + 1, 0);
    for (int32_t s = 0; s < sc.nsets; ++s) {
        const int64_t ms = sc.set_ptr[s + 1] - sc.set_ptr[s];
        koff[(size_t)s + 1] = koff[(size_t)s] + ms * ms;
        moff[(size_t)s + 1] = moff[(size_t)s] + (ms > kSetEigLds ? (ms + 1) * (ms + 1) : 0);
    }
}

double assoc_sets_bytes(const SetsCall &sc, int c, double *resident)
{
    if (resident) *resident = 0.0;
    if (sc.nsets == 0) return 0.0;
    std::vector<int64_t> koff, moff;
    sets_offsets(sc, koff, moff);
    const double nent = (double)sc.set_ptr[sc.nsets], ns = (double)sc.nsets;
    const double res = 8.0 * ((double)koff[(size_t)sc.nsets] + (double)moff[(size_t)sc.nsets]) + (sc.skato ? assoc_skato_bytes(sc, moff[(size_t)sc.nsets]) : 0.0);
    if (resident) *resident = res;
    return res + nent * (4.0 + 8.0 + 8.0 * c + 4.0 + 8.0)             // set_col, omega, u, the member lists, lambda
         + ns * (8.0 + 8.0 + 8.0 + 4.0 + 24.0) + 64.0;                 // set_ptr, the two offsets, m_used, T / S / Q
}

int assoc_sets_run(const AssocScan &scan, const SetsCall &sc, SetsOut &out)
{
    const mih_mat *h = scan.h;
    hipStream_t s = scan.s;
    const int c = scan.c;
    const double *S = scan.S, *V = scan.V;
    const int64_t n = h->n, p = h->p, ns = sc.nsets;
    const int64_t nent = ns ? sc.set_ptr[ns] : 0;
    out.m_used.assign((size_t)ns, 0); out.state.assign((size_t)ns, 0);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out.burden_z.assign((size_t)ns, nan); out.nlp_burden.assign((size_t)ns, nan); out.skat_q.assign((size_t)ns, nan); out.nlp_skat.assign((size_t)ns, nan);
    out.lambda.assign((size_t)nent, nan);
    if (sc.skato) {
        const size_t R = (size_t)sc.skato->nrho;
        out.nlp_skato.assign((size_t)ns, nan); out.skato_rho.assign((size_t)ns, nan); out.skato_state.assign((size_t)ns, 0);
        out.nlp_rho.assign((size_t)ns * R, nan); out.lambda_rho.assign((size_t)nent * (R + 1), nan);
    }
    if (ns == 0) return MIH_OK;
    std::vector<int64_t> koff, moff;
    sets_offsets(sc, koff, moff);
    const int64_t nk = koff[(size_t)ns], nm = moff[(size_t)ns];

    DevBuf<int64_t> ptr_d, koff_d, moff_d;
    DevBuf<int32_t> col_d, mused_d, mlist_d;
    DevBuf<double> om_d, Ub, Kb, Mb, stat_d, lam_d;
    MIH_TRY(ptr_d.alloc((size_t)ns + 1)); MIH_TRY(koff_d.alloc((size_t)ns + 1)); MIH_TRY(moff_d.alloc((size_t)ns + 1));
    MIH_TRY(col_d.alloc((size_t)nent)); MIH_TRY(mused_d.alloc((size_t)ns)); MIH_TRY(mlist_d.alloc((size_t)nent));
    MIH_TRY(om_d.alloc((size_t)nent)); MIH_TRY(Ub.alloc((size_t)nent * c)); MIH_TRY(Kb.alloc((size_t)nk)); MIH_TRY(Mb.alloc((size_t)nm));
    MIH_TRY(stat_d.alloc((size_t)ns * 3)); MIH_TRY(lam_d.alloc((size_t)nent));
    MIH_HIP(hipMemcpyAsync(ptr_d.p, sc.set_ptr, sizeof(int64_t) * ((size_t)ns + 1), hipMemcpyHostToDevice, s));
    MIH_HIP(hipMemcpyAsync(koff_d.p, koff.data(), sizeof(int64_t) * ((size_t)ns + 1), hipMemcpyHostToDevice, s));
    MIH_HIP(hipMemcpyAsync(moff_d.p, moff.data(), sizeof(int64_t) * ((size_t)ns + 1), hipMemcpyHostToDevice, s));
    if (nent > 0) {
        MIH_HIP(hipMemcpyAsync(col_d.p, sc.set_col, sizeof(int32_t) * (size_t)nent, hipMemcpyHostToDevice, s));
        MIH_HIP(hipMemcpyAsync(om_d.p, sc.omega, sizeof(double) * (size_t)nent, hipMemcpyHostToDevice, s));
        MIH_HIP(hipMemsetAsync(mlist_d.p, 0, sizeof(int32_t) * (size_t)nent, s));
        hipLaunchKernelGGL(k_assoc_set_u, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, s, S, p, c, scan.Linv, col_d.p, nent, Ub.p);
        MIH_TRY(launch_failed("k_assoc_set_u"));
    }
    const ColView mt = col_view(h);
    PassRecord pr;
    bool timed = prof_begin(h, s, pr);
    by_kind(h, [&](auto K) {
        hipLaunchKernelGGL(k_assoc_set_gram<decltype(K)::value>, dim3((unsigned)ns), dim3(256), 0, s, mt, n, ptr_d.p, col_d.p, om_d.p, V, scan.w,
                           koff_d.p, mused_d.p, mlist_d.p, Kb.p);
    });
    if (timed) { snprintf(pr.kernel, sizeof(pr.kernel), "k_assoc_set_gram"); pr.residuals = 1; pr.operands = 1; prof_end(h, s, pr); }
    MIH_TRY(launch_failed("k_assoc_set_gram"));
    hipLaunchKernelGGL(k_assoc_set_k, dim3((unsigned)ns), dim3(256), 0, s, ptr_d.p, col_d.p, om_d.p, S, V, c, Ub.p, koff_d.p, mused_d.p, mlist_d.p,
                       Kb.p, stat_d.p);
    MIH_TRY(launch_failed("k_assoc_set_k"));
    PassRecord pe;
    timed = prof_begin(h, s, pe);
    hipLaunchKernelGGL(k_assoc_set_eig, dim3((unsigned)ns), dim3(256), 0, s, ptr_d.p, om_d.p, koff_d.p, moff_d.p, mused_d.p, mlist_d.p, Kb.p, Mb.p,
                       lam_d.p);
    if (timed) { snprintf(pe.kernel, sizeof(pe.kernel), "k_assoc_set_eig"); pe.residuals = 1; pe.operands = 1; prof_end(h, s, pe); }
    MIH_TRY(launch_failed("k_assoc_set_eig"));

    std::vector<double> stat((size_t)ns * 3), Kh;
    std::vector<int32_t> mlist;
    MIH_HIP(hipMemcpyAsync(out.m_used.data(), mused_d.p, sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipMemcpyAsync(stat.data(), stat_d.p, sizeof(double) * (size_t)ns * 3, hipMemcpyDeviceToHost, s));
    if (nent > 0) MIH_HIP(hipMemcpyAsync(out.lambda.data(), lam_d.p, sizeof(double) * (size_t)nent, hipMemcpyDeviceToHost, s));
    if (sc.cov && nk > 0) {
        Kh.resize((size_t)nk); mlist.resize((size_t)nent);
        MIH_HIP(hipMemcpyAsync(Kh.data(), Kb.p, sizeof(double) * (size_t)nk, hipMemcpyDeviceToHost, s));
        MIH_HIP(hipMemcpyAsync(mlist.data(), mlist_d.p, sizeof(int32_t) * (size_t)nent, hipMemcpyDeviceToHost, s));
    }
    MIH_HIP(hipStreamSynchronize(s));

    for (int64_t k = 0; k < ns; ++k) {
        const int64_t e0 = sc.set_ptr[k];
        const int m = out.m_used[(size_t)k];
        const BurdenResult b = burden_tail(stat[(size_t)k * 3], stat[(size_t)k * 3 + 1]);
        const MixResult r = mixture_tail(m, out.lambda.data() + e0, stat[(size_t)k * 3 + 2]);
        out.burden_z[(size_t)k] = b.z; out.nlp_burden[(size_t)k] = b.neglog10p;
        out.skat_q[(size_t)k] = stat[(size_t)k * 3 + 2]; out.nlp_skat[(size_t)k] = r.neglog10p; out.state[(size_t)k] = (uint8_t)r.state;
    }
    if (sc.skato) {
        const SetsDevice dev = {s, h, ptr_d.p, koff_d.p, moff_d.p, mused_d.p, mlist_d.p, om_d.p, Kb.p, stat_d.p, nm, stat.data()};
        MIH_TRY(assoc_skato_run(dev, sc, out));
    }
    if (sc.cov) {                              // K over the entries of every set, NaN in the rows and columns of non-members
        out.cov.assign((size_t)nk, nan);
        for (int64_t k = 0; k < ns; ++k) {
            const int64_t e0 = sc.set_ptr[k], ms = sc.set_ptr[k + 1] - e0;
            const int m = out.m_used[(size_t)k];
            const double *src = Kh.data() + koff[(size_t)k];
            double *dst = out.cov.data() + koff[(size_t)k];
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) dst[(int64_t)mlist[(size_t)(e0 + i)] * ms + mlist[(size_t)(e0 + j)]] = src[i * m + j];
        }
    }
    return MIH_OK;
}

void sets_publish(const SetsCall &call, const SetsOut &out)
{
    if (call.nsets <= 0) return;
    const size_t ns = (size_t)call.nsets;
    memcpy(call.m_used, out.m_used.data(), sizeof(int32_t) * ns);
    memcpy(call.burden_z, out.burden_z.data(), sizeof(double) * ns);
    memcpy(call.neglog10p_burden, out.nlp_burden.data(), sizeof(double) * ns);
    memcpy(call.skat_q, out.skat_q.data(), sizeof(double) * ns);
    memcpy(call.neglog10p_skat, out.nlp_skat.data(), sizeof(double) * ns);
    memcpy(call.skat_state, out.state.data(), ns);
    if (call.lambda && !out.lambda.empty()) memcpy(call.lambda, out.lambda.data(), sizeof(double) * out.lambda.size());
    if (call.cov && !out.cov.empty()) memcpy(call.cov, out.cov.data(), sizeof(double) * out.cov.size());
    if (call.skato) skato_publish(call, out);
}

}  // namespace mih
