// assoc_spa.h -- what assoc_spa.hip and assoc_firth.hip offer the driver of the association scan (assoc.hip): the selection of
// the flagged columns with what every per-column solver needs of them, the saddlepoint pass and the Firth pass.
#pragma once
#include "assoc_slab.h"
#include "firth_finish.h"
#include <vector>

namespace mih {

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
// The selection after the plain scan's finish, on stream s: the columns with a finite |z| >= cutoff.  Device pointers: S (p x
// (1 + c): U, then b), z (p), Linv (c x c).  Host: eta (n).  who: the entry point, for the error texts.
MIH_LOCAL int assoc_flag_run(const char *who, const mih_mat *h, hipStream_t s, int c, const double *S, const double *z, const double *Linv,
                             const double *eta_host, double cutoff, AssocFlagged &fl);
MIH_LOCAL SpaMat assoc_spa_mat(const mih_mat *h);
// The saddlepoint pass over the selection.  Device pointers: S, V (p), Z (n x c).  Host: nlp (p, the normal values).  out (p),
// state (p) and that (p x 2 column-major) are sized and filled here; nothing of the caller's is touched.
MIH_LOCAL int assoc_spa_run(const mih_mat *h, hipStream_t s, int c, const AssocFlagged &fl, const double *S, const double *V, const double *Z,
                            const double *nlp, std::vector<double> &out, std::vector<uint8_t> &state, std::vector<double> &that);
// The Firth pass over the selection.  Host: beta, se, nlp (p, the plain scan's).  beta_f, se_f, nlp_f (p), state (p) and evals (p,
// 0 where not tried) are sized and filled here.
MIH_LOCAL int assoc_firth_run(const mih_mat *h, hipStream_t s, int c, const AssocFlagged &fl, const double *S, const double *V, const double *Z,
                              const double *beta, const double *se, const double *nlp, std::vector<double> &beta_f, std::vector<double> &se_f,
                              std::vector<double> &nlp_f, std::vector<uint8_t> &state, std::vector<int32_t> &evals);

}  // namespace mih
