// assoc_spa.h -- what assoc_spa.hip offers the driver of the association scan (assoc.hip).
#pragma once
#include "grm.h"
#include "spa_finish.h"
#include <vector>

namespace mih {

constexpr int64_t kSpaSlabs = 2048;              // workgroups of k_assoc_spa, each with a slab of n doubles: 8 on each of the 256 CUs

// device memory assoc_spa_run allocates at most (every column flagged), for the memory rule of the call
MIH_LOCAL double assoc_spa_bytes(int64_t n, int64_t p, int c);
// The saddlepoint pass after the plain scan's finish, on stream s.  Device pointers: S (p x (1 + c): U, then b), V and z (p),
// Linv (c x c), Z (n x c).  Host: eta (n), nlp (p, the normal values).  out (p), state (p) and that (p x 2 column-major) are
// sized and filled here; nothing of the caller's is touched.
MIH_LOCAL int assoc_spa_run(const mih_mat *h, hipStream_t s, int c, const double *S, const double *V, const double *z, const double *Linv,
                            const double *Z, const double *eta_host, double cutoff, const double *nlp, std::vector<double> &out,
                            std::vector<uint8_t> &state, std::vector<double> &that);

}  // namespace mih
