// scalar_log.h -- log(x) of ONE scalar, the same bits on the host and on the device.
// The closed forms of the Normal, Gamma and inverse-Gaussian loglikelihood take one logarithm of a scalar per evaluation:
// IhtVar::mu_loglik on the host (the host-driven step), b_res_decide on the device (the resident step).  Each side's libm rounds
// that logarithm correctly to within an ulp, but not to the SAME double; times n, the difference is the last bit of the term and
// many ulps of a loglikelihood that has cancelled to a small number (a fit with k > n, whose loglikelihood rises through zero) --
// and `old_logl > new_logl` decides a backtrack.  So both sides call this function: the classic reduction x = 2^k (1 + f),
// sqrt(2)/2 <= 1 + f < sqrt(2), s = f / (2 + f), log(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)) with the degree-14 minimax polynomial
// R of the freely distributable fdlibm (e_log.c; error below 1 ulp), in IEEE additions, multiplications and ONE division, never
// contracted into fused operations: every operation rounds the same way wherever it runs.  Plain C++: tests/scalar_log_harness.cpp
// builds it without HIP.
#pragma once
#include <cstdint>
#include <cmath>

#if defined(__HIPCC__)
#define MIH_SCALAR_HD __host__ __device__
#else
#define MIH_SCALAR_HD
#endif

namespace mih {

MIH_SCALAR_HD inline double scalar_log(double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(x > 0.0) || x > 1.7976931348623157e308) return log(x);      // 0, negative, NaN, +Inf: -Inf, NaN, NaN, +Inf on either side
    int k = 0;
    if (x < 2.2250738585072014e-308) { x *= 18014398509481984.0; k = -54; }       // subnormal: scaled by 2^54 (exact)
    uint64_t bits;
    __builtin_memcpy(&bits, &x, sizeof(bits));
    k += (int)(bits >> 52) - 1023;
    uint64_t man = bits & 0x000FFFFFFFFFFFFFull;
    if (man >= 0x6A09E667F3BCDull) { man |= 0x3FE0000000000000ull; k += 1; }      // mantissa at or above sqrt(2): halve, [sqrt(2)/2, 1)
    else man |= 0x3FF0000000000000ull;                                            // [1, sqrt(2))
    double m;
    __builtin_memcpy(&m, &man, sizeof(m));
    const double f = m - 1.0;                                                      // exact
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    const double dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s, w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

}  // namespace mih
