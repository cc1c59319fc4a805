// The host algebra of the REML null model (csrc/lmm_host.h) on inputs with known answers; plain C++, no HIP.
// Prints one line per check and "all ok" at the end; the exit status is the number of failed checks.
#include "lmm_host.h"
#include <cstdio>

using namespace mih;

static int failed = 0;

static void check(bool ok, const char *what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failed;
}

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol * std::max(1.0, std::fabs(b)); }

int main()
{
    {   // the inverse of a 3 x 3 SPD matrix, against the product with the matrix
        const double H[9] = {4.0, 1.0, 0.5, 1.0, 3.0, 0.25, 0.5, 0.25, 2.0};
        double S[9];
        bool ok = lmm_spd_inverse(3, H, S) == 3;
        for (int a = 0; a < 3 && ok; ++a)
            for (int b = 0; b < 3; ++b) {
                double t = 0.0;
                for (int k = 0; k < 3; ++k) t += H[a * 3 + k] * S[k * 3 + b];
                ok = ok && std::fabs(t - (a == b ? 1.0 : 0.0)) <= 1e-14;
            }
        check(ok, "inverse of a 3 x 3 SPD matrix");
        const double one[1] = {8.0};
        double inv[1] = {0.0};
        check(lmm_spd_inverse(1, one, inv) == 1 && inv[0] == 0.125, "inverse of a 1 x 1 matrix");
    }
    {   // rank-deficient, not positive, NaN: the rank is reported and Sigma is left alone
        const double R[4] = {1.0, 2.0, 2.0, 4.0}, N[4] = {1.0, 0.0, 0.0, -1.0}, Q[4] = {1.0, std::nan(""), std::nan(""), 1.0};
        double S[4] = {-7.0, -7.0, -7.0, -7.0};
        check(lmm_spd_inverse(2, R, S) == 1 && S[0] == -7.0 && S[3] == -7.0, "a rank-one matrix reports rank 1");
        check(lmm_spd_inverse(2, N, S) < 2 && S[0] == -7.0, "an indefinite matrix is refused");
        check(lmm_spd_inverse(2, Q, S) == 0 && S[0] == -7.0, "a NaN reports rank 0");
    }
    {   // the full step: AI = [[2, 1], [1, 3]] (given unsymmetrised), score = (1, 2): delta = (0.2, 0.6)
        const double tau[2] = {1.0, 1.0}, score[2] = {1.0, 2.0}, AI[4] = {2.0, 1.5, 0.5, 3.0};
        double next[2];
        check(lmm_ai_step(tau, score, AI, next) == 0 && near(next[0], 1.2, 1e-15) && near(next[1], 1.6, 1e-15), "a full step, AI symmetrised");
    }
    {   // halving: delta = (-4, 0.5) from tau = (1, 1): h = 3 is the first with 1 - 4 / 2^h >= 0.1
        const double tau[2] = {1.0, 1.0}, score[2] = {-4.0, 0.5}, AI[4] = {1.0, 0.0, 0.0, 1.0};
        double next[2];
        check(lmm_ai_step(tau, score, AI, next) == 3 && next[0] == 0.5 && next[1] == 1.0625, "three halvings keep a tenth of tau_e");
        const double ten[2] = {10.0, 10.0}, edge[2] = {-9.0, 0.0};   // lands on a tenth exactly: accepted without halving
        check(lmm_ai_step(ten, edge, AI, next) == 0 && next[0] == 1.0 && next[1] == 10.0, "a tenth is enough");
    }
    {   // no inverse, NaN: refused, next untouched
        const double tau[2] = {1.0, 1.0}, score[2] = {1.0, 1.0}, sing[4] = {1.0, 1.0, 1.0, 1.0}, bad[4] = {1.0, 0.0, 0.0, std::nan("")};
        double next[2] = {-7.0, -7.0};
        check(lmm_ai_step(tau, score, sing, next) == -1 && next[0] == -7.0, "a singular AI is refused");
        check(lmm_ai_step(tau, score, bad, next) == -1 && next[1] == -7.0, "a NaN in AI is refused");
        const double nt[2] = {std::nan(""), 1.0}, id[4] = {1.0, 0.0, 0.0, 1.0};
        check(lmm_ai_step(nt, score, id, next) == -1 && next[0] == -7.0, "a NaN tau finds no step");
    }
    {
        const double a[2] = {1.0, 2.0}, b[2] = {1.0, 2.0}, c[2] = {3.0, 2.0}, z[2] = {0.0, 0.0}, n[2] = {std::nan(""), 1.0};
        check(lmm_rel_change(a, b) == 0.0, "no change");
        check(near(lmm_rel_change(a, c), 1.0, 1e-15), "2 |1 - 3| / (1 + 3) = 1");
        check(lmm_rel_change(z, z) == 0.0, "0 / 0 is no change");
        check(std::isnan(lmm_rel_change(n, a)), "a NaN is the worst");
    }
    std::printf(failed ? "%d failed\n" : "all ok\n", failed);
    return failed;
}
