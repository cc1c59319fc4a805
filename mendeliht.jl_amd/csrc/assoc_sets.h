// assoc_sets.h -- what assoc_sets.hip offers the driver of the association scan (assoc.hip): the checks of a list of variant sets,
// the device memory the set pass will hold, and the pass itself (mih_assoc_sets).
#pragma once
#include "assoc_spa.h"
#include <vector>

namespace mih {

// what mih_assoc_sets adds to a call (nullptr: no set pass)
struct SetsCall {
    int32_t nsets; const int64_t *set_ptr; const int32_t *set_col; const double *omega;
    int32_t *m_used; double *burden_z, *neglog10p_burden, *skat_q, *neglog10p_skat; uint8_t *skat_state; double *lambda, *cov;
};

// the results of the pass on the host, sized and filled by assoc_sets_run; the driver copies them out when everything is there
struct SetsOut {
    std::vector<int32_t> m_used;
    std::vector<double> burden_z, nlp_burden, skat_q, nlp_skat, lambda, cov;
    std::vector<uint8_t> state;
};

// MIH_OK, or MIH_BAD_ARG with the error text set: a null array, nsets < 0, a malformed set_ptr, a set of more than
// kSymEigMaxOrder entries, a column outside [0, p), columns of a set not strictly ascending, an omega negative or not finite
MIH_LOCAL int assoc_sets_check(const SetsCall &sc, int64_t p);
// device memory assoc_sets_run allocates; *resident (if not null): the share of it that is per-set working storage (K and the
// Jacobi scratch of the sets of more than 64 entries)
MIH_LOCAL double assoc_sets_bytes(const SetsCall &sc, int c, double *resident);
// The pass, after the plain scan's finish, on stream s.  Device pointers: S (p x (1 + c): U, then b), V (p), Linv (c x c),
// w (n, ones where the call has none).
MIH_LOCAL int assoc_sets_run(const mih_mat *h, hipStream_t s, int c, const double *S, const double *V, const double *Linv, const double *w,
                             const SetsCall &sc, SetsOut &out);

}  // namespace mih
