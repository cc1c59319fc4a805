// sym_eig.h -- the small host algebra of the subspace iteration in pca.hip: a cyclic Jacobi eigen-solver for symmetric
// matrices up to 128 x 128 (the library links no LAPACK), the rank rule of the Gram-based orthonormalisation and the sign
// rule of the returned vectors.  No HIP in it: tests/sym_eig_harness.cpp compiles it with plain g++.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define MIH_SYM_EIG_FN __host__ __device__ inline
#else
#define MIH_SYM_EIG_FN inline
#endif

namespace mih {

constexpr int kSymEigMaxOrder = 128;
constexpr int kSymEigMaxSweeps = 60;

// A (n x n, row-major, symmetric: only its lower triangle is read) = V diag(w) V', w descending, V row-major with the
// eigenvector of w[i] in column i.  Cyclic Jacobi by rows: every rotation annihilates one off-diagonal pair exactly, and
// a sweep ends the iteration when the off-diagonal norm has fallen to u |A|_F (u = 2^-53) -- the eigenvalues are then
// within n u |A|_F of the exact ones up to a small constant, the backward error of the method.  A pair at or below
// u |A|_F / n is left alone: together such pairs are inside that norm.  Equal eigenvalues keep the order Jacobi left them
// in (a stable sort).  Returns the sweeps used, kSymEigMaxSweeps + 1 if the norm never fell; a matrix with a NaN or an
// infinity in it has no decomposition: w and V are all NaN then, with the same return value.
inline int sym_eig_jacobi(int n, const double *A, double *w, double *V)
{
    std::vector<double> a((size_t)n * n), v((size_t)n * n, 0.0);
    double fro2 = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double x = j <= i ? A[(size_t)i * n + j] : A[(size_t)j * n + i];
            a[(size_t)i * n + j] = x;
            fro2 += x * x;
        }
    for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    const double u = 1.1102230246251565e-16, fro = std::sqrt(fro2), skip = u * fro / (double)std::max(n, 1);
    if (!std::isfinite(fro)) {                                       // nothing to decompose: say so in every number returned
        std::fill(w, w + n, std::nan(""));
        std::fill(V, V + (size_t)n * n, std::nan(""));
        return kSymEigMaxSweeps + 1;
    }
    int sweeps = 0;
    for (;;) {
        double off2 = 0.0;
        for (int p = 1; p < n; ++p)
            for (int q = 0; q < p; ++q) off2 += 2.0 * a[(size_t)p * n + q] * a[(size_t)p * n + q];
        if (std::sqrt(off2) <= u * fro) break;                      // (a NaN never satisfies this)
        if (sweeps == kSymEigMaxSweeps) { ++sweeps; break; }
        ++sweeps;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (!(std::fabs(apq) > skip)) continue;
                const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::hypot(theta, 1.0));
                const double c = 1.0 / std::hypot(t, 1.0), s = t * c;
                a[(size_t)p * n + p] -= t * apq;
                a[(size_t)q * n + q] += t * apq;
                a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
                for (int r = 0; r < n; ++r) {
                    if (r != p && r != q) {
                        const double arp = a[(size_t)r * n + p], arq = a[(size_t)r * n + q];
                        a[(size_t)r * n + p] = a[(size_t)p * n + r] = c * arp - s * arq;
                        a[(size_t)r * n + q] = a[(size_t)q * n + r] = s * arp + c * arq;
                    }
                    const double vrp = v[(size_t)r * n + p], vrq = v[(size_t)r * n + q];
                    v[(size_t)r * n + p] = c * vrp - s * vrq;
                    v[(size_t)r * n + q] = s * vrp + c * vrq;
                }
            }
    }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * n + x] > a[(size_t)y * n + y]; });
    for (int i = 0; i < n; ++i) {
        w[i] = a[(size_t)order[(size_t)i] * n + order[(size_t)i]];
        for (int r = 0; r < n; ++r) V[(size_t)r * n + i] = v[(size_t)r * n + order[(size_t)i]];
    }
    return sweeps;
}

// The rank rule: of the eigenvalues d (descending) of a Gram matrix Y'Y, direction i survives if d_i > 2^-52 d_1; none
// survives a d_1 that is not positive (or not a number).  What is dropped is a numerically null direction of the block.
inline int sym_eig_rank(int n, const double *d)
{
    if (n < 1 || !(d[0] > 0.0)) return 0;
    const double floor_d = 2.220446049250313e-16 * d[0];
    int r = 0;
    while (r < n && d[r] > floor_d) ++r;
    return r;
}

// The sign rule: the entry of largest magnitude, the lowest index on a tie, is made positive.  sign_rule_better says
// whether (|x|, index i) takes the place of the best entry so far -- the one comparison the device's reduction and the
// host function below share.
MIH_SYM_EIG_FN bool sign_rule_better(double ax, int64_t i, double abest, int64_t ibest)
{
    return ax > abest || (ax == abest && i < ibest);
}

inline int64_t sign_rule_pivot(int64_t n, const double *x)
{
    int64_t ib = 0;
    double ab = -1.0;
    for (int64_t i = 0; i < n; ++i)
        if (sign_rule_better(std::fabs(x[i]), i, ab, ib)) { ab = std::fabs(x[i]); ib = i; }
    return ib;
}

inline void sign_rule_apply(int64_t n, double *x)
{
    if (n < 1 || !(x[sign_rule_pivot(n, x)] < 0.0)) return;
    for (int64_t i = 0; i < n; ++i) x[i] = -x[i];
}

}  // namespace mih
