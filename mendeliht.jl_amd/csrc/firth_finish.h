// firth_finish.h -- the scalar parts of the Firth-penalised test of the case-control scan (mih_assoc_score_firth): the control of
// the root iteration, which the device runs once per evaluation in every lane of k_assoc_firth, and the finish of a column from
// the values at the root, which the host runs.  Plain C++ with <cmath> only, so that a stand-alone harness can test both on the
// CPU (tests/firth_finish_harness.cpp).  tests/firth_spec.py states the same in numpy.
//
// The one-parameter logistic model with the covariates' effects held at the null fit has the log-likelihood beta q - K(beta), K
// the cumulant generating function of spa_finish.h.  With Jeffreys' penalty, L*(beta) = beta q - K(beta) + log(K2(beta) / K2(0)) / 2,
// and its stationarity condition is g(beta) = q with g = K1 - K3 / (2 K2): the saddlepoint equation with one correction term.
#pragma once
#include "spa_finish.h"

namespace mih {

constexpr double kFirthMinK2 = 9.094947017729282e-13;    // 2^-40: state 1 needs K2(beta_hat) >= kFirthMinK2 V

// g and its slope D = g' from the four sums of an evaluation; D is K2 where it is not finite or not > 0
MIH_SPA_HD inline void firth_g(double k1, double k2, double k3, double k4, double &g, double &D)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    g = k1 - 0.5 * (k3 / k2);
    D = k2 - 0.5 * ((k4 * k2 - k3 * k3) / (k2 * k2));
    if (!(D > 0.0) || !(D - D == 0.0)) D = k2;
}

// One evaluation of the root of g(beta) = q: spa_iter_step with k1 := g, k2 := D, s := q; an evaluation whose g - q is not
// finite ends the column as not converged (status 2).
MIH_SPA_HD inline void firth_iter_step(SpaIter &it, double k1, double k2, double k3, double k4, double q, double tol)
{
    double g, D;
    firth_g(k1, k2, k3, k4, g, D);
    const double f = g - q;
    if (!(f - f == 0.0)) { ++it.evals; it.status = 2; return; }
    spa_iter_step(it, g, D, q, tol);
}

// What the device leaves of a tried column: beta = beta_hat, K = K(beta_hat) and K2 = K2(beta_hat) from the pass at the root,
// I0 = K2 of the first evaluation (beta = 0).  status: 1 converged, 2 not.
struct FirthRoot { double beta, K, K2, I0; int status, evals; };

// A tried column.  Returns the state: 1 -- *beta, *se, *nlp are the penalised estimate, 1 / sqrt K2(beta_hat) and the chi^2_1 tail
// of the penalised likelihood ratio; 2 -- they are the plain scan's values as given.
inline int firth_column(const FirthRoot &r, double q, double V, double beta_plain, double se_plain, double nlp_plain, double *beta,
                        double *se, double *nlp)
{
    *beta = beta_plain; *se = se_plain; *nlp = nlp_plain;
    if (r.status != 1 || !std::isfinite(r.beta) || !std::isfinite(r.K2) || !(r.K2 >= kFirthMinK2 * V)) return 2;
    double dev = 2.0 * ((r.beta * q - r.K) + 0.5 * std::log(r.K2 / r.I0));
    if (!std::isfinite(dev)) return 2;
    if (dev < 0.0) dev = 0.0;
    *beta = r.beta;
    *se = 1.0 / std::sqrt(r.K2);
    *nlp = neglog10p_of_z(std::sqrt(dev));
    return 1;
}

}  // namespace mih
