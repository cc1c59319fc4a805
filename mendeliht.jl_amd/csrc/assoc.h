// assoc.h -- where the driver of the association scan (assoc.hip) and its passes meet (assoc_spa.hip: the selection and the
// saddlepoint pass, assoc_firth.hip: the Firth pass, assoc_sets.hip: the set pass, assoc_skato.hip: SKAT-O on top of it): the view of a handle's columns and the one
// dispatch on its kind, what each entry point adds to a call and what each pass hands back, and what the plain scan leaves for
// the passes.  The device code the kernels share is assoc_slab.h.
#pragma once
#include "grm.h"
#include <algorithm>
#include <type_traits>
#include <vector>

namespace mih {

// ---- the columns of a handle, whatever its kind --------------------------------------------------------------------------------------
struct ColView {
    const double *D; const float *Df; DosageView dv;
    const uint32_t *X; int64_t nbp; const double *mu, *sinv; int center, scale, impute;
    const int64_t *miss_ptr; const int32_t *miss_row;
};
inline ColView col_view(const mih_mat *h)
{
    return ColView{h->D, h->Df, dosage_view(h), h->X, h->nbp, h->mu, h->sinv, h->center, h->scale, h->impute, h->miss_ptr, h->miss_row};
}

// f(std::integral_constant<int, KIND>()) with the KIND the kernels are instantiated by: 0 dense f64, 1 dense f32, 2 16-bit dosage,
// 3 2-bit.  A generic lambda reads it as decltype(K)::value.
template <class F>
inline void by_kind(const mih_mat *h, F &&f)
{
    if (h->kind == 0) f(std::integral_constant<int, 3>());
    else if (h->Du) f(std::integral_constant<int, 2>());
    else if (h->Df) f(std::integral_constant<int, 1>());
    else f(std::integral_constant<int, 0>());
}

// ---- what the plain scan leaves for the passes, after its finish -----------------------------------------------------------------------
// Device, on stream s: S (p x (t + c): U, then b), V (p), Linv (c x c row-major), Z (n x c), w (n, ones where the call has none),
// z (p x t).  Host: the plain scan's beta, se (p) and neglog10p (the normal values).  The passes run on one trait: t = 1.
struct AssocScan {
    const mih_mat *h; hipStream_t s; int c;
    const double *S, *V, *Linv, *Z, *w, *z;
    const double *beta, *se, *nlp;
};

// ---- the selection that the per-column solvers share -----------------------------------------------------------------------------------
constexpr int64_t kSpaSlabs = 2048;              // workgroups of a solver, each with a slab of n doubles: 8 on each of the 256 CUs

// What the solvers share of a call, all on the device but hidx: the flagged columns' indices (idx, p + 1: the count last) and
// their copy on the host, eta, mu = sigma(eta), softplus(eta), the flagged columns' alpha (nflag x c), and grid slabs of n
// doubles -- allocated once, every solver forms a column's c_i into its workgroup's slab anew.
struct AssocFlagged {
    DevBuf<int64_t> idx;
    DevBuf<double> eta, mu, sp0, alpha, slab;
    std::vector<int64_t> hidx;
    int64_t nflag = 0, grid = 0;
};

// device memory assoc_flag_run allocates at most (every column flagged), and with the saddlepoint pass's own records; the Firth
// pass's records (assoc_firth_bytes) come on top of assoc_flag_bytes.  For the memory rule of the call.
MIH_LOCAL double assoc_flag_bytes(int64_t n, int64_t p, int c);
MIH_LOCAL double assoc_spa_bytes(int64_t n, int64_t p, int c);
MIH_LOCAL double assoc_firth_bytes(int64_t p);
// The selection: the columns with a finite |z| >= cutoff.  Host: eta (n).  who: the entry point, for the error texts.
MIH_LOCAL int assoc_flag_run(const char *who, const AssocScan &sc, const double *eta_host, double cutoff, AssocFlagged &fl);

// The host half that the two solvers have in common, up to their per-column finish: rec (rec_w doubles a flagged column) and st
// (st_w words) are allocated, pick(K) -- the solver's kernel of kind K, both have one signature -- runs over the selection
// inside the measurement hook's record `name`, and both arrays come back to the host.  fl.nflag > 0.
template <class Pick>
int assoc_solver_launch(const AssocScan &sc, const AssocFlagged &fl, const char *name, int rec_w, int st_w, Pick pick,
                        std::vector<double> &hrec, std::vector<int32_t> &hst)
{
    const mih_mat *h = sc.h;
    hipStream_t s = sc.s;
    const int64_t n = h->n, p = h->p, nflag = fl.nflag;
    DevBuf<double> rec;
    DevBuf<int32_t> st;
    MIH_TRY(rec.alloc((size_t)(rec_w * nflag))); MIH_TRY(st.alloc((size_t)(st_w * nflag)));
    const ColView m = col_view(h);
    PassRecord pr;
    const bool timed = prof_begin(h, s, pr);
    by_kind(h, [&](auto K) {
        hipLaunchKernelGGL(pick(K), dim3((unsigned)fl.grid), dim3(256), 0, s, m, n, p, sc.c, fl.idx.p, nflag, fl.alpha.p, sc.Z, fl.eta.p,
                           fl.mu.p, fl.sp0.p, sc.S, sc.V, fl.slab.p, rec.p, st.p);
    });
    if (timed) { snprintf(pr.kernel, sizeof(pr.kernel), "%s", name); pr.residuals = 1; pr.operands = (int)std::min<int64_t>(nflag, 2147483647); prof_end(h, s, pr); }
    MIH_TRY(launch_failed(name));

    hrec.resize((size_t)(rec_w * nflag));
    hst.resize((size_t)(st_w * nflag));
    MIH_HIP(hipMemcpyAsync(hrec.data(), rec.p, sizeof(double) * hrec.size(), hipMemcpyDeviceToHost, s));
    MIH_HIP(hipMemcpyAsync(hst.data(), st.p, sizeof(int32_t) * hst.size(), hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    return MIH_OK;
}

// ---- the three optional passes: what the entry point adds to a call, what the pass hands back, and how it reaches the caller ---------
// Every *_run sizes and fills its *Out on the host and touches nothing of the caller's; *_publish copies it to the caller's
// arrays (an optional output may be NULL) once every pass of the call has succeeded.

// mih_assoc_score_spa (nullptr: no saddlepoint pass)
struct SpaCall { const double *eta; double cutoff; double *neglog10p_spa; uint8_t *state; double *t_hat; };
struct SpaOut {                                  // nlp, state (p), t_hat (p x 2 column-major)
    std::vector<double> nlp, t_hat;
    std::vector<uint8_t> state;
};
MIH_LOCAL int assoc_spa_run(const AssocScan &sc, const AssocFlagged &fl, SpaOut &out);
MIH_LOCAL void spa_publish(const SpaCall &call, const SpaOut &out);

// mih_assoc_score_firth (nullptr: no Firth pass); with a SpaCall beside it both passes run on one selection
struct FirthCall { const double *eta; double cutoff; double *beta, *se, *neglog10p; uint8_t *state; int32_t *evals; };
struct FirthOut {                                // all p; evals 0 where not tried
    std::vector<double> beta, se, nlp;
    std::vector<uint8_t> state;
    std::vector<int32_t> evals;
};
MIH_LOCAL int assoc_firth_run(const AssocScan &sc, const AssocFlagged &fl, FirthOut &out);
MIH_LOCAL void firth_publish(const FirthCall &call, const FirthOut &out);

// what mih_assoc_sets_skato adds to a set pass: the grid (rho = NULL: the default grid) and the SKAT-O outputs
struct SkatoCall {
    int32_t nrho; const double *rho;
    double *neglog10p_skato, *skato_rho; uint8_t *skato_state; double *neglog10p_rho, *lambda_rho;
};
// mih_assoc_sets (nullptr: no set pass); skato (nullptr: no SKAT-O) is mih_assoc_sets_skato's
struct SetsCall {
    int32_t nsets; const int64_t *set_ptr; const int32_t *set_col; const double *omega;
    int32_t *m_used; double *burden_z, *neglog10p_burden, *skat_q, *neglog10p_skat; uint8_t *skat_state; double *lambda, *cov;
    const SkatoCall *skato;
};
struct SetsOut {
    std::vector<int32_t> m_used;
    std::vector<double> burden_z, nlp_burden, skat_q, nlp_skat, lambda, cov;
    std::vector<uint8_t> state;
    std::vector<double> nlp_skato, skato_rho, nlp_rho, lambda_rho;          // SKAT-O: nsets, nsets, nsets x nrho, (nrho + 1) x entries
    std::vector<uint8_t> skato_state;
};
// MIH_OK, or MIH_BAD_ARG with the error text set: a null array, nsets < 0, a malformed set_ptr, a set of more than
// kSymEigMaxOrder entries, a column outside [0, p), columns of a set not strictly ascending, an omega negative or not finite
MIH_LOCAL int assoc_sets_check(const SetsCall &call, int64_t p);
// device memory assoc_sets_run allocates; *resident (if not null): the share of it that is per-set working storage (K and the
// Jacobi scratch of the sets of more than 64 entries)
MIH_LOCAL double assoc_sets_bytes(const SetsCall &call, int c, double *resident);
MIH_LOCAL int assoc_sets_run(const AssocScan &sc, const SetsCall &call, SetsOut &out);
MIH_LOCAL void sets_publish(const SetsCall &call, const SetsOut &out);

// The SKAT-O pass (assoc_skato.hip), run by assoc_sets_run on what the set pass left on the device (stream s): the lists, K,
// T / S / Q per set (stat), the offsets of the sets' K and Jacobi slabs, and on the host m_used, stat and the SKAT results in out.
struct SetsDevice {
    hipStream_t s; const mih_mat *h;
    const int64_t *set_ptr, *koff, *moff; const int32_t *m_used, *mlist; const double *omega, *Kb, *stat;
    int64_t nslab;                               // doubles of all Jacobi slabs of one matrix per set: moff[nsets]
    const double *stat_host;
};
MIH_LOCAL int assoc_skato_check(const SkatoCall &call);
// device memory assoc_skato_run allocates: R + 1 Jacobi slabs per large set, lambda_rho, the grid and the integrands
MIH_LOCAL double assoc_skato_bytes(const SetsCall &call, int64_t nslab);
MIH_LOCAL int assoc_skato_run(const SetsDevice &dev, const SetsCall &call, SetsOut &out);
MIH_LOCAL void skato_publish(const SetsCall &call, const SetsOut &out);

}  // namespace mih
