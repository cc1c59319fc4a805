// Stand-alone harness of csrc/skato_tail.h: the host step of SKAT-O (the tails over the grid, p_min, the quantiles, u0) and the
// integral as the device evaluates it -- the 256 terms of skato_term and the fixed log-sum-exp tree, here in one loop.
// stdin, per set:  m R Q T S rr wt neglog10p_skat skat_state   then the R grid values (already capped), R rows of m eigenvalues
//                  (those of M_rho) and the m eigenvalues of M~.
// stdout per set:  state rho neglog10p_skato neglog10p_integral u0 mu kfac   then R rows  state_rho neglog10p_rho q_rho tau_rho  (%.17g)
#include "skato_tail.h"
#include <cstdio>
#include <vector>

using namespace mih;

int main()
{
    int m, R, skat_state;
    double Q, T, S, rr, wt, nlp_skat;
    while (scanf("%d %d %lf %lf %lf %lf %lf %lf %d", &m, &R, &Q, &T, &S, &rr, &wt, &nlp_skat, &skat_state) == 9) {
        if (m < 0 || m > 128 || R < 1 || R > kSkatoMaxRho) return 2;
        std::vector<double> grid((size_t)R), lam((size_t)(R + 1) * (size_t)m), nlp_rho((size_t)R);
        std::vector<int> st_rho((size_t)R);
        for (int r = 0; r < R; ++r)
            if (scanf("%lf", &grid[(size_t)r]) != 1) return 2;
        for (size_t i = 0; i < lam.size(); ++i)
            if (scanf("%lf", &lam[i]) != 1) return 2;
        const double *lam_t = lam.data() + (size_t)R * (size_t)m;
        SkatoPrep p = skato_prepare(m, R, grid.data(), lam.data(), m, lam_t, Q, T, S, rr, wt, nlp_skat, skat_state, nlp_rho.data(), st_rho.data());
        double nlp_int = std::nan("");
        if (p.state == kSkatoIntegral) {
            double red[kSkatoPanels * kSkatoNodes];
            for (int t = 0; t < kSkatoPanels * kSkatoNodes; ++t) red[t] = skato_term(t, m, lam_t, p.g);
            for (int k = kSkatoPanels * kSkatoNodes / 2; k > 0; k >>= 1)
                for (int t = 0; t < k; ++t) red[t] = skato_lse(red[t], red[t + k]);
            skato_finish(p, skato_scale(red[0]), &nlp_int);
        }
        printf("%d %d %.17g %.17g %.17g %.17g %.17g\n", p.state, p.rho, p.neglog10p, nlp_int, p.g.u0, p.g.mu, p.g.kfac);
        for (int r = 0; r < R; ++r) printf("%d %.17g %.17g %.17g\n", st_rho[(size_t)r], nlp_rho[(size_t)r], p.g.q[r], p.g.tau[r]);
    }
    return 0;
}
