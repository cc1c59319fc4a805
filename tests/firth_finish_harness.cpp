// Stand-alone harness of csrc/firth_finish.h: the control of the Firth root iteration (firth_iter_step, which the device runs in
// every lane of k_assoc_firth) and the host's finish of a column (firth_column).  The row sums, which the device makes, are made
// here in long double, as tests/firth_spec.py makes them, so that the two can be compared closely.
// stdin, per column:  n q V beta se nlp nan_at   then n lines  c_i h_i   (nan_at: the evaluation, counted from 1, whose K1 is
// replaced by a NaN; 0 for none).   stdout per column:  state beta_firth se_firth neglog10p_firth evals   (%.17g)
#include "firth_finish.h"
#include <cstdio>
#include <vector>

using namespace mih;

struct Col {
    std::vector<long double> c, h, mu, sp0;
    long double m1 = 0;
    static void parts(long double x, long double &e, long double &r) { e = expl(-fabsl(x)); r = 1.0L / (1.0L + e); }
    void prepare()
    {
        mu.resize(c.size()); sp0.resize(c.size());
        for (size_t i = 0; i < c.size(); ++i) {
            long double e, r;
            parts(h[i], e, r);
            mu[i] = h[i] >= 0 ? r : e * r;
            sp0[i] = fmaxl(h[i], 0.0L) + log1pl(e);
            m1 += c[i] * mu[i];
        }
    }
    void k1234(double t, double k[4]) const
    {
        long double a1 = 0, a2 = 0, a3 = 0, a4 = 0;
        for (size_t i = 0; i < c.size(); ++i) {
            long double e, r;
            const long double x = h[i] + c[i] * (long double)t;
            parts(x, e, r);
            const long double er = e * r, s = er * r, d = (1.0L - e) * r, c2 = c[i] * c[i];
            a1 += c[i] * ((x >= 0 ? r : er) - mu[i]);
            a2 += c2 * s;
            a3 += (c2 * c[i]) * (s * (x >= 0 ? -d : d));
            a4 += (c2 * c2) * (s * (1.0L - 6.0L * s));
        }
        k[0] = (double)a1; k[1] = (double)a2; k[2] = (double)a3; k[3] = (double)a4;
    }
    void k02(double t, double &k0, double &k2) const
    {
        long double a = 0, b = 0;
        for (size_t i = 0; i < c.size(); ++i) {
            long double e, r;
            const long double x = h[i] + c[i] * (long double)t;
            parts(x, e, r);
            a += (fmaxl(x, 0.0L) + log1pl(e)) - sp0[i];
            b += (c[i] * c[i]) * ((e * r) * r);
        }
        k0 = (double)(a - (long double)t * m1); k2 = (double)b;
    }
};

int main()
{
    long long n;
    int nan_at;
    double q, V, beta, se, nlp;
    while (scanf("%lld %lf %lf %lf %lf %lf %d", &n, &q, &V, &beta, &se, &nlp, &nan_at) == 7) {
        if (n < 1 || n > 100000000) return 2;
        Col col;
        col.c.resize((size_t)n); col.h.resize((size_t)n);
        for (long long i = 0; i < n; ++i) {
            double c, h;
            if (scanf("%lf %lf", &c, &h) != 2) return 2;
            col.c[(size_t)i] = c; col.h[(size_t)i] = h;
        }
        col.prepare();
        const double tol = kSpaTolF * std::sqrt(V);
        FirthRoot root = {std::nan(""), std::nan(""), std::nan(""), std::nan(""), 0, 0};
        SpaIter it;
        spa_iter_start(it);
        while (it.status == 0) {
            double k[4];
            col.k1234(it.t, k);
            if (it.evals + 1 == nan_at) k[0] = std::nan("");
            if (it.evals == 0) root.I0 = k[1];
            firth_iter_step(it, k[0], k[1], k[2], k[3], q, tol);
        }
        root.status = it.status; root.evals = it.evals;
        if (it.status == 1) {
            root.beta = it.that;
            if (std::isfinite(it.that)) col.k02(it.that, root.K, root.K2);
        }
        double bf = 0.0, sf = 0.0, nf = 0.0;
        const int state = firth_column(root, q, V, beta, se, nlp, &bf, &sf, &nf);
        printf("%d %.17g %.17g %.17g %d\n", state, bf, sf, nf, root.evals);
    }
    return 0;
}
