// lmm_host.h -- the small host algebra of the REML null model in lmm.hip: the inverse of the c x c matrix Z'V^-1 Z, the 2 x 2
// average-information step with its halving rule, and the convergence measure.  No HIP in it: tests/lmm_host_harness.cpp
// compiles it with plain g++.
#pragma once
#include "sym_eig.h"

namespace mih {

constexpr int kLmmMaxHalvings = 60;

// Sigma = H^-1 for a symmetric positive definite H (c x c, row-major, only its lower triangle is read), through the Jacobi
// eigen-decomposition: Sigma = W D^-1 W'.  Returns the numerical rank of H (sym_eig_rank); Sigma is written only if it is c.
inline int lmm_spd_inverse(int c, const double *H, double *Sigma)
{
    std::vector<double> d((size_t)c), W((size_t)c * c);
    sym_eig_jacobi(c, H, d.data(), W.data());
    const int rank = sym_eig_rank(c, d.data());
    if (rank < c || !(d[(size_t)c - 1] > 0.0)) return std::min(rank, c - 1);
    for (int a = 0; a < c; ++a)
        for (int b = 0; b < c; ++b) {
            double s = 0.0;
            for (int k = 0; k < c; ++k) s += W[(size_t)a * c + k] * W[(size_t)b * c + k] / d[(size_t)k];
            Sigma[(size_t)a * c + b] = s;
        }
    return c;
}

// The average-information step: delta = AI^-1 score by Cramer's rule on the symmetrised AI = {a00, (a01 + a10) / 2, a11}, then
// tau' = tau + 2^-h delta with the smallest h >= 0 that keeps both components at least a tenth of their previous values.
// Returns h, or -1 when AI has no inverse with finite entries, or no h up to kLmmMaxHalvings serves (a NaN among the inputs).
inline int lmm_ai_step(const double tau[2], const double score[2], const double AI[4], double next[2])
{
    const double a00 = AI[0], a01 = 0.5 * (AI[1] + AI[2]), a11 = AI[3];
    const double det = a00 * a11 - a01 * a01;
    const double d0 = (a11 * score[0] - a01 * score[1]) / det, d1 = (a00 * score[1] - a01 * score[0]) / det;
    if (!std::isfinite(d0) || !std::isfinite(d1)) return -1;
    double scale = 1.0;
    for (int h = 0; h <= kLmmMaxHalvings; ++h, scale *= 0.5) {
        const double t0 = tau[0] + scale * d0, t1 = tau[1] + scale * d1;
        if (t0 >= 0.1 * tau[0] && t1 >= 0.1 * tau[1]) { next[0] = t0; next[1] = t1; return h; }
    }
    return -1;
}

// 2 max_i |a_i - b_i| / (|a_i| + |b_i|); 0 / 0 is no change, a NaN is the worst
inline double lmm_rel_change(const double a[2], const double b[2])
{
    double worst = 0.0;
    for (int i = 0; i < 2; ++i) {
        const double den = std::fabs(a[i]) + std::fabs(b[i]);
        const double r = den == 0.0 ? 0.0 : 2.0 * std::fabs(a[i] - b[i]) / den;
        if (r > worst || std::isnan(r)) worst = r;               // (once a NaN, it stays)
    }
    return worst;
}

}  // namespace mih
