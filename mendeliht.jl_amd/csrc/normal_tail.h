// normal_tail.h -- the two-sided normal tail of a z statistic as -log10 p, finite far beyond where p itself underflows.
// Plain C++ with <cmath> only, so that a stand-alone harness can test it on the CPU (tests/normal_tail_harness.cpp).
#pragma once
#include <cmath>

// the tails are host code; the integrand of SKAT-O (assoc_skato.hip) evaluates them on the device as well
#ifdef __HIPCC__
#define MIH_TAIL_FN __host__ __device__ inline
#else
#define MIH_TAIL_FN inline
#endif

namespace mih {

// x >= kTailSwitch: log erfc(x) from Laplace's continued fraction
//     erfc(x) = exp(-x^2) / sqrt(pi) * 1 / (x + (1/2) / (x + 1 / (x + (3/2) / (x + 2 / (x + ...)))))
// evaluated from the bottom with a fixed number of terms: at x >= 25 term k changes the value by less than (k / (2 x^2))^k, so
// kTailTerms = 24 terms leave far less than one ulp.  erfc(25) = 8e-274 is still a normal number: below the switch libm's erfc
// is used as it is.
constexpr double kTailSwitch = 25.0;
constexpr int kTailTerms = 24;

MIH_TAIL_FN double log_erfc_tail(double x)
{
    double f = x;
    for (int k = kTailTerms; k >= 1; --k) f = x + (0.5 * k) / f;
    return -x * x - 0.5723649429247001 /* log(pi) / 2 */ - std::log(f);
}

// -log10 of p = erfc(|z| / sqrt 2), the two-sided p-value of a standard normal z.  NaN for a NaN, +inf for an infinite z.
// Small |z|: p = 1 - erf(x) is formed through log1p so that the result keeps its relative accuracy down to z = 0 (which gives 0).
MIH_TAIL_FN double neglog10p_of_z(double z)
{
    if (std::isnan(z)) return z;
    const double x = std::fabs(z) * 0.7071067811865476 /* 1 / sqrt 2 */;
    const double inv_ln10 = 0.4342944819032518;
    if (std::isinf(x)) return x;
    if (x < 0.5) return -std::log1p(-std::erf(x)) * inv_ln10;
    if (x < kTailSwitch) return -std::log(std::erfc(x)) * inv_ln10;
    return -log_erfc_tail(x) * inv_ln10;
}

}  // namespace mih
