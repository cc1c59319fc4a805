// mixture_tail.h -- the host finish of the set-based tests (mih_assoc_sets): the burden statistic from T and S, and the upper tail
// P(sum_i lambda_i chi2_1 > Q) of a positive mixture of chi-squares by the saddlepoint approximation of Kuonen (1999), with the
// root iteration, the tails and the states.  Plain C++ with <cmath> only, so that a stand-alone harness can test it on the CPU
// (tests/mixture_tail_harness.cpp).  tests/sets_spec.py states the same in numpy.
//
// lambda: m eigenvalues in descending order, none negative (the caller has set every lambda_i <= 0 to 0).  With
//     K(t) = -1/2 sum log1p(-2 lambda_i t),   K'(t) = sum lambda_i / (1 - 2 lambda_i t),   K''(t) = 2 sum (lambda_i / (1 - 2 lambda_i t))^2
// t_hat solves K'(t_hat) = Q on t < 1 / (2 lambda_1), w = sign(t_hat) sqrt(2 (t_hat Q - K(t_hat))), v = t_hat sqrt(K''(t_hat)),
// r = w + log(v / w) / w and the tail is log Phi(-r).
//
// Everything is evaluated in units of 1 / (2 lambda_1): s = 2 lambda_1 t < 1, mu_i = lambda_i / lambda_1 in [0, 1], q = Q / lambda_1,
//     g(s) = sum mu_i / (1 - mu_i s) = K' / lambda_1,     g2(s) = sum (mu_i / (1 - mu_i s))^2 = K'' / (2 lambda_1^2),
//     w^2 = s q + sum log1p(-mu_i s),                     v = s sqrt(g2 / 2)
// (all sums with i ascending from 0.0, every operation rounded by itself).  The root of f(s) = g(s) - q:
//     s = 0, lo missing, hi = 1 (the pole: f -> +inf there), no evaluations yet.  Repeat:
//     evaluate g, g2 (one evaluation); f = g - q
//     |f| <= 2^-40 q: converged; s_hat = s - f / g2 (one more Newton step, taken as it is) -- stop
//     128 evaluations made: not converged -- stop
//     f < 0: lo = s, else hi = s
//     sn = s - f / g2; if not lo < sn < hi (a NaN is not):
//         f < 0: sn = (s + hi) / 2
//         f > 0: sn = (lo + s) / 2 if lo exists, else 2 s if s < 0, else -1
//     s = sn
// (f is convex and increasing on s < 1: from the right of the root Newton descends monotonically, from the left it overshoots and
// the bracket catches it.  The last step moves s by at most 2^-40 m (1 - s), so s_hat < 1.)  t_hat = s_hat / (2 lambda_1).
//
// The states of a set, decided in this order:
//     0  m = 0, or lambda_1 is not > 0 and finite: NaN
//     2  rank one, m = 1 or lambda_2 <= 2^-40 lambda_1: the exact chi2_1 tail, neglog10p_of_z(sqrt(Q) / sqrt(lambda_1)) -- for a
//        one-variant set with omega = 1, sqrt(U U) = |U| exactly and this is the scan's own p, bit for bit
//     4  Q <= 0: the tail is 1, the value 0
//     5  the iteration did not converge: the tail of the moment-matched normal, z = (Q - sum lambda) / sqrt(2 sum lambda^2), one-sided
//     3  near the mean, w^2 < 2^-40 (|w| < 2^-20; a w^2 that rounding left negative too): the limit r = kappa_3 / 6,
//        kappa_3 = 8 sum mu^3 / (2 sum mu^2)^(3/2) the skewness (from K = k1 t + k2 t^2 / 2 + k3 t^3 / 6: w = t sqrt k2 (1 + k3 t / (3 k2)),
//        v = t sqrt k2 (1 + k3 t / (2 k2)), log(v / w) / w -> k3 / (6 k2^(3/2)))
//     1  the saddlepoint value
#pragma once
#include "normal_tail.h"
#include <cmath>
#include <cstdint>

namespace mih {

constexpr double kMixTolF = 9.094947017729282e-13;       // 2^-40: |g(s) - q| <= kMixTolF q
constexpr double kMixRankOne = 9.094947017729282e-13;    // 2^-40: lambda_2 <= kMixRankOne lambda_1 is rank one
constexpr double kMixNearMean = 9.094947017729282e-13;   // 2^-40: w^2 below this is "at the mean"
constexpr int kMixMaxEvals = 128;

// log Phi(-r) for any r, by the arithmetic of neglog10p_of_z
MIH_TAIL_FN double mix_log_phi_neg(double r)
{
    const double x = std::fabs(r) * 0.7071067811865476 /* 1 / sqrt 2 */, ln2 = 0.6931471805599453;
    if (std::isnan(x)) return x;
    if (r < 0.0) return std::isinf(x) ? 0.0 : std::log1p(-0.5 * std::erfc(x));
    if (std::isinf(x)) return -x;
    if (x < 0.5) return std::log1p(-std::erf(x)) - ln2;
    if (x < kTailSwitch) return std::log(std::erfc(x)) - ln2;
    return log_erfc_tail(x) - ln2;
}

struct MixIter { double s, lo, hi, shat; int evals, status; };      // status: 0 running, 1 converged, 2 gave up

MIH_TAIL_FN void mix_eval(int m, const double *lambda, double s, double *g, double *g2)
{
    const double l1 = lambda[0];
    double a = 0.0, b = 0.0;
    for (int i = 0; i < m; ++i) {
        const double mu = lambda[i] / l1, d = mu / (1.0 - mu * s);
        a = a + d;
        b = b + d * d;
    }
    *g = a; *g2 = b;
}

// the root iteration of the header comment; lambda[0] > 0 and finite, q > 0
MIH_TAIL_FN void mix_root(int m, const double *lambda, double q, MixIter &it)
{
    it.s = 0.0; it.lo = -HUGE_VAL; it.hi = 1.0; it.shat = std::nan(""); it.evals = 0; it.status = 0;
    const double tol = kMixTolF * q;
    for (;;) {
        double g, g2;
        mix_eval(m, lambda, it.s, &g, &g2);
        ++it.evals;
        const double f = g - q;
        if (std::fabs(f) <= tol) { it.shat = it.s - f / g2; it.status = 1; return; }
        if (it.evals == kMixMaxEvals) { it.status = 2; return; }
        if (f < 0.0) it.lo = it.s; else it.hi = it.s;
        double sn = it.s - f / g2;
        if (!(sn > it.lo && sn < it.hi)) {
            if (f < 0.0) sn = (it.s + it.hi) / 2.0;
            else sn = it.lo > -HUGE_VAL ? (it.lo + it.s) / 2.0 : (it.s < 0.0 ? 2.0 * it.s : -1.0);
        }
        it.s = sn;
    }
}

struct MixResult { double neglog10p, t_hat; int state, evals; };

// the SKAT tail of one set: lambda (m, descending, >= 0 or NaN), Q
MIH_TAIL_FN MixResult mixture_tail(int m, const double *lambda, double Q)
{
    const double nan = std::nan(""), inv_ln10 = 0.4342944819032518;
    MixResult r = {nan, nan, 0, 0};
    if (m < 1 || !(lambda[0] > 0.0) || !std::isfinite(lambda[0])) return r;
    const double l1 = lambda[0];
    if (m == 1 || lambda[1] <= kMixRankOne * l1) { r.state = 2; r.neglog10p = neglog10p_of_z(std::sqrt(Q) / std::sqrt(l1)); return r; }
    if (!(Q > 0.0)) { r.state = 4; r.neglog10p = 0.0; return r; }
    const double q = Q / l1;
    MixIter it;
    mix_root(m, lambda, q, it);
    r.evals = it.evals;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;          // sums of mu, mu^2, mu^3
    for (int i = 0; i < m; ++i) {
        const double mu = lambda[i] / l1;
        s1 = s1 + mu; s2 = s2 + mu * mu; s3 = s3 + (mu * mu) * mu;
    }
    if (it.status != 1) {
        r.state = 5;
        r.neglog10p = -mix_log_phi_neg((q - s1) / std::sqrt(2.0 * s2)) * inv_ln10;
        return r;
    }
    const double sh = it.shat;
    r.t_hat = sh / (2.0 * l1);
    double g, g2, lg = 0.0;
    mix_eval(m, lambda, sh, &g, &g2);
    for (int i = 0; i < m; ++i) lg = lg + std::log1p(-(lambda[i] / l1) * sh);
    const double w2 = sh * q + lg;
    if (!(w2 >= kMixNearMean)) {
        r.state = 3;
        r.neglog10p = -mix_log_phi_neg((8.0 * s3 / std::pow(2.0 * s2, 1.5)) / 6.0) * inv_ln10;
        return r;
    }
    const double w = std::copysign(std::sqrt(w2), sh), v = sh * std::sqrt(g2 / 2.0);
    const double rr = w + std::log(v / w) / w;
    r.state = 1;
    r.neglog10p = -mix_log_phi_neg(rr) * inv_ln10;
    return r;
}

struct BurdenResult { double z, neglog10p; };

// burden_z = T / sqrt S, NaN where S <= 0 (or is NaN); the two-sided normal tail
MIH_TAIL_FN BurdenResult burden_tail(double T, double S)
{
    BurdenResult b;
    b.z = S > 0.0 ? T / std::sqrt(S) : std::nan("");
    b.neglog10p = neglog10p_of_z(b.z);
    return b;
}

}  // namespace mih
