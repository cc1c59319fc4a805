// assoc_skato.hip -- SKAT-O, the optimal combination of the burden and the SKAT test of a variant set, on top of the set pass
// (mih_assoc_sets_skato).  tests/skato_spec.py states the definitions in numpy; skato_tail.h has the host step and the integrand,
// include/mendeliht_hip.h the contract in full.
//
// The set pass (assoc_sets.hip) leaves per set K, the member list, omega and T, S, Q on the device.  On top of it:
//   k_assoc_set_rho    one workgroup per (set, r), r = 0 .. R: the eigenvalues of M_rho_r (r < R) or of M~ = M - rs rs' / S (r = R),
//                      formed entry by entry from M, rs and S and decomposed by the Jacobi of k_assoc_set_eig (assoc_set_eig.h);
//                      the workgroup of r = R also gives rs' rs and rs' M~ rs
//   host               skato_prepare: the R tails, p_min, the quantiles, tau, mu, kfac, u0 of every set
//   k_assoc_set_skato  one workgroup per set that has an integral: lambda~ in LDS, thread t evaluates term t (its node's
//                      saddlepoint root by mixture_tail's iteration, log S~ + log phi + log weight), a fixed log-sum-exp tree
//   host               skato_finish: the tail beyond u0, SKAT's clamp, the states
// Every value has a fixed operation order: nothing depends on slice_rows, on the position of a set or on the other sets.
#include "assoc.h"
#include "assoc_set_eig.h"
#include "skato_tail.h"
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>

namespace mih {

// ---- the eigenvalues of M_rho and M~ -------------------------------------------------------------------------------------------------
// lam_rho[r nent + e0 ..]: the eigenvalues of matrix r of set s = blockIdx.x, r = blockIdx.y; NaN after m.  With c = sqrt(1 - rho),
// d = (sqrt((1 - rho) + m rho) - c) / m:  M_rho[j, k] = ((c c) M_jk + (c d) (rs_j + rs_k)) + (d d) S for j >= k, mirrored -- at rho = 0,
// c = 1 and d = 0 exactly and the matrix is M itself;  M~[j, k] = M_jk - (rs_j rs_k) / S.  rs_j = sum_k M_jk, k ascending
// (k_assoc_set_k's).  aux[2 s ..] = rs' rs, rs' M~ rs (j ascending; the inner sum_k M~_jk rs_k with k ascending), by r = R.
// A set of more than kSetEigLds members has R + 1 slabs in Mb: matrix r at (R + 1) moff[s] + r (moff[s + 1] - moff[s]).
__global__ void __launch_bounds__(256)
k_assoc_set_rho(const int64_t *__restrict__ set_ptr, const double *__restrict__ omega, const int64_t *__restrict__ koff, const int64_t *__restrict__ moff,
                const int32_t *__restrict__ m_used, const int32_t *__restrict__ mlist, const double *__restrict__ Kb, const double *__restrict__ stat,
                const double *__restrict__ grid, int R, int64_t nent, double *__restrict__ Mb, double *__restrict__ lam_rho, double *__restrict__ aux)
{
#pragma clang fp contract(off)
    __shared__ double sa[kSetEigLds * (kSetEigLds + 1)];
    __shared__ double om[kSymEigMaxOrder], rs[kSymEigMaxOrder], tv[kSymEigMaxOrder];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int64_t s = blockIdx.x, e0 = set_ptr[s];
    const int ms = min((int)(set_ptr[s + 1] - e0), kSymEigMaxOrder);
    const int m = min(m_used[s], ms);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double *lam = lam_rho + (int64_t)r * nent + e0;
    for (int i = tid; i < ms; i += 256) if (i >= m) lam[i] = nan;
    if (m <= 0) {
        if (r == R && tid < 2) aux[2 * s + tid] = 0.0;
        return;
    }
    const int me = (m + 1) & ~1, lda = m <= kSetEigLds ? kSetEigLds + 1 : me;
    double *a = m <= kSetEigLds ? sa : Mb + (int64_t)(R + 1) * moff[s] + (int64_t)r * (moff[s + 1] - moff[s]);
    if (tid < m) om[tid] = omega[e0 + mlist[e0 + tid]];
    __syncthreads();
    const double *K = Kb + koff[s];
    if (tid < m) {
        double acc = 0.0;
        for (int k = 0; k < m; ++k) acc = acc + set_m_entry(K, m, om, tid, k);
        rs[tid] = acc;
    }
    __syncthreads();
    const double S = stat[3 * s + 1];
    double cc = 0.0, cd = 0.0, dd = 0.0;
    if (r < R) {
        const double rho = grid[r], c = sqrt(1.0 - rho), d = (sqrt((1.0 - rho) + (double)m * rho) - c) / (double)m;
        cc = c * c; cd = c * d; dd = d * d;
    }
    double f2 = 0.0;
    for (int idx = tid; idx < me * me; idx += 256) {
        const int i = idx / me, j = idx % me;
        double v = 0.0;
        if (i < m && j < m) {
            const int hi = max(i, j), lo = min(i, j);
            const double mjk = set_m_entry(K, m, om, hi, lo);
            v = r < R ? (cc * mjk + cd * (rs[hi] + rs[lo])) + dd * S : mjk - (rs[hi] * rs[lo]) / S;
        }
        a[i * lda + j] = v;
        f2 = f2 + v * v;
    }
    if (r == R) {
        __syncthreads();
        if (tid < m) {
            double acc = 0.0;
            for (int k = 0; k < m; ++k) acc = acc + a[tid * lda + k] * rs[k];
            tv[tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double rr = 0.0, wt = 0.0;
            for (int j = 0; j < m; ++j) { rr = rr + rs[j] * rs[j]; wt = wt + rs[j] * tv[j]; }
            aux[2 * s] = rr; aux[2 * s + 1] = wt;
        }
    }
    set_jacobi_eig(a, lda, m, f2, lam);
}

// ---- the integral ------------------------------------------------------------------------------------------------------------------------
// Workgroup b integrates set pend[b] with the integrand G[b]: li[b] = log(2 int_0^u0 S~(delta'(u^2)) phi(u) du), thread t the term
// t of skato_tail.h, the tree in its fixed order.  lam_t: the eigenvalues of M~, laid out like set_col.
__global__ void __launch_bounds__(256)
k_assoc_set_skato(const int32_t *__restrict__ pend, const int64_t *__restrict__ set_ptr, const int32_t *__restrict__ m_used,
                  const double *__restrict__ lam_t, const SkatoIntegrand *__restrict__ G, double *__restrict__ li)
{
#pragma clang fp contract(off)
    __shared__ double lt[kSymEigMaxOrder];
    __shared__ double red[256];
    __shared__ SkatoIntegrand g;
    static_assert(sizeof(SkatoIntegrand) % 8 == 0, "copied in 8-byte words");
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, s = pend[b], e0 = set_ptr[s];
    const int m = min(m_used[s], min((int)(set_ptr[s + 1] - e0), kSymEigMaxOrder));
    if (tid < m) lt[tid] = lam_t[e0 + tid];
    if (tid < (int)(sizeof(SkatoIntegrand) / 8)) ((uint64_t *)&g)[tid] = ((const uint64_t *)(G + b))[tid];
    __syncthreads();
    red[tid] = skato_term(tid, m, lt, g);
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) red[tid] = skato_lse(red[tid], red[tid + k]);
        __syncthreads();
    }
    if (tid == 0) li[b] = skato_scale(red[0]);
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------
int assoc_skato_check(const SkatoCall &k)
{
    if (!k.neglog10p_skato || !k.skato_rho || !k.skato_state) { set_error("mih_assoc_sets_skato: null argument"); return MIH_BAD_ARG; }
    if (k.nrho < 1 || k.nrho > kSkatoMaxRho) { set_error("mih_assoc_sets_skato: 1 <= nrho <= %d grid values, got %d", kSkatoMaxRho, (int)k.nrho); return MIH_BAD_ARG; }
    if (!k.rho) {
        if (k.nrho != kSkatoDefaultRho) { set_error("mih_assoc_sets_skato: the default grid has %d values, nrho is %d", kSkatoDefaultRho, (int)k.nrho); return MIH_BAD_ARG; }
        return MIH_OK;
    }
    for (int32_t r = 0; r < k.nrho; ++r) {
        if (!(k.rho[r] >= 0.0 && k.rho[r] <= 1.0)) { set_error("mih_assoc_sets_skato: rho %d is outside [0, 1]", (int)r + 1); return MIH_BAD_ARG; }
        if (r > 0 && !(k.rho[r] > k.rho[r - 1])) { set_error("mih_assoc_sets_skato: the grid is not strictly ascending at rho %d", (int)r + 1); return MIH_BAD_ARG; }
    }
    return MIH_OK;
}

double assoc_skato_bytes(const SetsCall &sc, int64_t nslab)
{
    const double R1 = (double)sc.skato->nrho + 1.0, nent = (double)sc.set_ptr[sc.nsets], ns = (double)sc.nsets;
    return 8.0 * (R1 * (double)nslab + R1 * nent + 2.0 * ns + 16.0) + ns * (4.0 + 8.0 + (double)sizeof(SkatoIntegrand));
}

int assoc_skato_run(const SetsDevice &dev, const SetsCall &sc, SetsOut &out)
{
    const SkatoCall &k = *sc.skato;
    hipStream_t s = dev.s;
    const int R = k.nrho;
    const int64_t ns = sc.nsets, nent = sc.set_ptr[ns];
    double given[kSkatoMaxRho], grid[kSkatoMaxRho];
    for (int r = 0; r < R; ++r) { given[r] = k.rho ? k.rho[r] : kSkatoDefaultGrid[r]; grid[r] = std::fmin(given[r], kSkatoRhoCap); }

    DevBuf<double> grid_d, Mb, lam_d, aux_d;
    MIH_TRY(grid_d.alloc((size_t)R)); MIH_TRY(Mb.alloc((size_t)(dev.nslab * (R + 1)))); MIH_TRY(lam_d.alloc((size_t)(nent * (R + 1)))); MIH_TRY(aux_d.alloc((size_t)ns * 2));
    MIH_HIP(hipMemcpyAsync(grid_d.p, grid, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, s));
    PassRecord pr;
    bool timed = prof_begin(dev.h, s, pr);
    hipLaunchKernelGGL(k_assoc_set_rho, dim3((unsigned)ns, (unsigned)(R + 1)), dim3(256), 0, s, dev.set_ptr, dev.omega, dev.koff, dev.moff, dev.m_used,
                       dev.mlist, dev.Kb, dev.stat, grid_d.p, R, nent, Mb.p, lam_d.p, aux_d.p);
    if (timed) { snprintf(pr.kernel, sizeof(pr.kernel), "k_assoc_set_rho"); pr.residuals = 1; pr.operands = R + 1; prof_end(dev.h, s, pr); }
    MIH_TRY(launch_failed("k_assoc_set_rho"));
    std::vector<double> aux((size_t)ns * 2);
    MIH_HIP(hipMemcpyAsync(aux.data(), aux_d.p, sizeof(double) * aux.size(), hipMemcpyDeviceToHost, s));
    if (nent > 0) MIH_HIP(hipMemcpyAsync(out.lambda_rho.data(), lam_d.p, sizeof(double) * (size_t)(nent * (R + 1)), hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));

    // the host step: the tails, p_min and the quantiles of every set -- sets are independent, so a few host threads share them
    // (contiguous ranges; no value depends on the split); then the sets with an integral are listed in order
    std::vector<SkatoPrep> prep((size_t)ns);
    const auto prepare = [&](int64_t q0, int64_t q1) {
        int st_rho[kSkatoMaxRho];
        for (int64_t q = q0; q < q1; ++q) {
            const int64_t e0 = sc.set_ptr[q];
            const double *st = dev.stat_host + 3 * q;
            prep[(size_t)q] = skato_prepare(out.m_used[(size_t)q], R, grid, out.lambda_rho.data() + e0, nent, out.lambda_rho.data() + (int64_t)R * nent + e0,
                                            st[2], st[0], st[1], aux[(size_t)(2 * q)], aux[(size_t)(2 * q + 1)], out.nlp_skat[(size_t)q],
                                            (int)out.state[(size_t)q], out.nlp_rho.data() + q * R, st_rho);
        }
    };
    unsigned nth = std::thread::hardware_concurrency();
    nth = nth >= 16 ? 8 : (nth >= 4 ? nth / 2 : 1);
    nth = (unsigned)std::min<int64_t>(nth, std::max<int64_t>(1, ns / 64));
    if (nth <= 1) prepare(0, ns);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; ++t) th.emplace_back(prepare, ns * t / nth, ns * (t + 1) / nth);
        for (auto &t : th) t.join();
    }
    std::vector<int32_t> pend;
    std::vector<SkatoIntegrand> G;
    for (int64_t q = 0; q < ns; ++q)
        if (prep[(size_t)q].state == kSkatoIntegral) { pend.push_back((int32_t)q); G.push_back(prep[(size_t)q].g); }
    std::vector<double> li(pend.size());
    if (!pend.empty()) {
        DevBuf<int32_t> pend_d;
        DevBuf<SkatoIntegrand> G_d;
        DevBuf<double> li_d;
        MIH_TRY(pend_d.alloc(pend.size())); MIH_TRY(G_d.alloc(G.size())); MIH_TRY(li_d.alloc(li.size()));
        MIH_HIP(hipMemcpyAsync(pend_d.p, pend.data(), sizeof(int32_t) * pend.size(), hipMemcpyHostToDevice, s));
        MIH_HIP(hipMemcpyAsync(G_d.p, G.data(), sizeof(SkatoIntegrand) * G.size(), hipMemcpyHostToDevice, s));
        PassRecord pi;
        timed = prof_begin(dev.h, s, pi);
        hipLaunchKernelGGL(k_assoc_set_skato, dim3((unsigned)pend.size()), dim3(256), 0, s, pend_d.p, dev.set_ptr, dev.m_used, lam_d.p + (int64_t)R * nent,
                           G_d.p, li_d.p);
        if (timed) { snprintf(pi.kernel, sizeof(pi.kernel), "k_assoc_set_skato"); pi.residuals = 1; pi.operands = 1; prof_end(dev.h, s, pi); }
        MIH_TRY(launch_failed("k_assoc_set_skato"));
        MIH_HIP(hipMemcpyAsync(li.data(), li_d.p, sizeof(double) * li.size(), hipMemcpyDeviceToHost, s));
        MIH_HIP(hipStreamSynchronize(s));
    }
    for (size_t b = 0; b < pend.size(); ++b) skato_finish(prep[(size_t)pend[b]], li[b], nullptr);
    for (int64_t q = 0; q < ns; ++q) {
        const SkatoPrep &p = prep[(size_t)q];
        out.nlp_skato[(size_t)q] = p.neglog10p; out.skato_state[(size_t)q] = (uint8_t)p.state;
        out.skato_rho[(size_t)q] = p.rho >= 0 ? given[p.rho] : std::numeric_limits<double>::quiet_NaN();
    }
    return MIH_OK;
}

void skato_publish(const SetsCall &call, const SetsOut &out)
{
    const SkatoCall &k = *call.skato;
    const size_t ns = (size_t)call.nsets;
    memcpy(k.neglog10p_skato, out.nlp_skato.data(), sizeof(double) * ns);
    memcpy(k.skato_rho, out.skato_rho.data(), sizeof(double) * ns);
    memcpy(k.skato_state, out.skato_state.data(), ns);
    if (k.neglog10p_rho && !out.nlp_rho.empty()) memcpy(k.neglog10p_rho, out.nlp_rho.data(), sizeof(double) * out.nlp_rho.size());
    if (k.lambda_rho && !out.lambda_rho.empty()) memcpy(k.lambda_rho, out.lambda_rho.data(), sizeof(double) * out.lambda_rho.size());
}

}  // namespace mih
