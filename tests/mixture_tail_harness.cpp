// Stand-alone harness of csrc/mixture_tail.h: the host finish of the set-based tests -- the burden statistic from T and S, and
// the SKAT tail of a set from its eigenvalues and Q (the root iteration, the tails and the states).
// stdin, per set:  m Q T S   then m eigenvalues (descending, none negative).
// stdout per set:  state neglog10p_skat t_hat evals burden_z neglog10p_burden   (%.17g)
#include "mixture_tail.h"
#include <cstdio>
#include <vector>

using namespace mih;

int main()
{
    int m;
    double Q, T, S;
    while (scanf("%d %lf %lf %lf", &m, &Q, &T, &S) == 4) {
        if (m < 0 || m > 100000) return 2;
        std::vector<double> lam((size_t)m);
        for (int i = 0; i < m; ++i)
            if (scanf("%lf", &lam[(size_t)i]) != 1) return 2;
        const MixResult r = mixture_tail(m, lam.data(), Q);
        const BurdenResult b = burden_tail(T, S);
        printf("%d %.17g %.17g %d %.17g %.17g\n", r.state, r.neglog10p, r.t_hat, r.evals, b.z, b.neglog10p);
    }
    return 0;
}
