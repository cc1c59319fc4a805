// spa_finish.h -- the scalar parts of the saddlepoint p-value (mih_assoc_score_spa): the control of the root iteration, which the
// device runs once per evaluation in every lane of k_assoc_spa, and the finish of a column from the values at the root, which
// the host runs.  Plain C++ with <cmath> only, so that a stand-alone harness can test both on the CPU (tests/spa_finish_harness.cpp).
// tests/spa_spec.py states the same in numpy.
#pragma once
#include "normal_tail.h"
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MIH_SPA_HD __host__ __device__
#else
#define MIH_SPA_HD
#endif

namespace mih {

constexpr double kSpaTolF = 9.313225746154785e-10;       // 2^-30: |K'(t) - s| <= kSpaTolF sqrt V
constexpr double kSpaMinK2 = 9.5367431640625e-07;        // 2^-20: a tail needs K''(t_hat) >= kSpaMinK2 V
constexpr int kSpaMaxEvals = 64;

// The root of K'(t) = s: Newton from t = 0 inside the bracket (lo, hi) of the signs of f = K'(t) - s seen so far.  A step that
// leaves the bracket (or is NaN) is replaced by the midpoint where both ends exist, by doubling (1 from t = 0) while the outer
// end is missing.  status: 0 running, 1 converged (that = t - f / K'': one more Newton step, taken as it is), 2 gave up after
// kSpaMaxEvals evaluations.
struct SpaIter { double t, lo, hi, that; int evals, status; };

MIH_SPA_HD inline void spa_iter_start(SpaIter &it)
{
    it.t = 0.0; it.lo = -HUGE_VAL; it.hi = HUGE_VAL; it.that = 0.0; it.evals = 0; it.status = 0;
}

MIH_SPA_HD inline void spa_iter_step(SpaIter &it, double k1, double k2, double s, double tol)
{
    ++it.evals;
    const double f = k1 - s;
    if (fabs(f) <= tol) { it.that = it.t - f / k2; it.status = 1; return; }
    if (it.evals == kSpaMaxEvals) { it.status = 2; return; }
    if (f < 0.0) it.lo = it.t; else it.hi = it.t;
    double tn = it.t - f / k2;
    if (!(tn > it.lo && tn < it.hi)) {
        if (f < 0.0) tn = it.hi < HUGE_VAL ? (it.t + it.hi) / 2.0 : (it.t > 0.0 ? 2.0 * it.t : 1.0);
        else tn = it.lo > -HUGE_VAL ? (it.lo + it.t) / 2.0 : (it.t < 0.0 ? 2.0 * it.t : -1.0);
    }
    it.t = tn;
}

// log Phi(-a), a >= 0, by the arithmetic of neglog10p_of_z
inline double log_phi_neg(double a)
{
    const double x = a * 0.7071067811865476 /* 1 / sqrt 2 */, ln2 = 0.6931471805599453;
    if (std::isnan(x)) return x;
    if (std::isinf(x)) return -x;
    if (x < 0.5) return std::log1p(-std::erf(x)) - ln2;
    if (x < kTailSwitch) return std::log(std::erfc(x)) - ln2;
    return log_erfc_tail(x) - ln2;
}

// What the device leaves of one tail.  status: 0 not computed (its target lies outside the range of the statistic: it
// contributes exactly 0), 1 converged (t = t_hat, K = K(t_hat), K2 = K''(t_hat)), 2 not converged.
struct SpaTail { double t, K, K2; int status, evals; };

// the log of the tail at target s; false: refused
inline bool spa_tail_log(const SpaTail &tl, double s, double V, double *logp)
{
    if (tl.status != 1 || !std::isfinite(tl.t) || !(tl.K2 >= kSpaMinK2 * V)) return false;
    const double ts = tl.t * s;
    const double w = std::copysign(std::sqrt(2.0 * (ts - tl.K)), tl.t);
    const double v = tl.t * std::sqrt(tl.K2);
    const double r = w + std::log(v / w) / w;
    if (!std::isfinite(r) || r == 0.0 || (r > 0.0) != (tl.t > 0.0)) return false;
    *logp = log_phi_neg(std::fabs(r));
    return true;
}

// -log10(exp(l0) + exp(l1)); either may be -inf (not both)
inline double spa_combine(double l0, double l1)
{
    const double m = l0 >= l1 ? l0 : l1, o = l0 >= l1 ? l1 : l0;
    return -(m + std::log1p(std::exp(o - m))) * 0.4342944819032518 /* 1 / log 10 */;
}

// A tried column: tails[0] has target +|q|, tails[1] has -|q|.  Returns the state (1: *out is the saddlepoint value, 2: a
// computed tail was refused and *out = nlp, the normal value).
inline int spa_column(const SpaTail tails[2], double q, double V, double nlp, double *out)
{
    const double aq = std::fabs(q);
    double l[2] = {-HUGE_VAL, -HUGE_VAL};
    for (int k = 0; k < 2; ++k) {
        if (tails[k].status == 0) continue;
        if (!spa_tail_log(tails[k], k == 0 ? aq : -aq, V, &l[k])) { *out = nlp; return 2; }
    }
    if (tails[0].status == 0 && tails[1].status == 0) { *out = nlp; return 2; }
    *out = spa_combine(l[0], l[1]);
    return 1;
}

}  // namespace mih
