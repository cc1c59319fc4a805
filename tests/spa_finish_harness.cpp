// Stand-alone harness of csrc/spa_finish.h: the control of the saddlepoint root iteration (spa_iter_step, which the device runs
// in every lane of k_assoc_spa) and the host's finish of a column (spa_column).  The row sums, which the device makes, are made
// here in long double, as tests/spa_spec.py makes them, so that the two can be compared closely.
// stdin, per column:  n q V nlp   then n lines  c_i h_i.   stdout per column:  state value t0 t1 evals0 evals1   (%.17g)
#include "spa_finish.h"
#include <cstdio>
#include <vector>

using namespace mih;

struct Col {
    std::vector<long double> c, h, mu, sp0;
    long double m1 = 0, neg = 0, pos = 0;
    static void parts(long double x, long double &e, long double &r) { e = expl(-fabsl(x)); r = 1.0L / (1.0L + e); }
    void prepare()
    {
        mu.resize(c.size()); sp0.resize(c.size());
        for (size_t i = 0; i < c.size(); ++i) {
            long double e, r;
            parts(h[i], e, r);
            mu[i] = h[i] >= 0 ? r : e * r;
            sp0[i] = fmaxl(h[i], 0.0L) + log1pl(e);
            m1 += c[i] * mu[i]; neg += fminl(c[i], 0.0L); pos += fmaxl(c[i], 0.0L);
        }
    }
    void k12(double t, double &k1, double &k2) const
    {
        long double a = 0, b = 0;
        for (size_t i = 0; i < c.size(); ++i) {
            long double e, r;
            const long double x = h[i] + c[i] * (long double)t;
            parts(x, e, r);
            a += c[i] * ((x >= 0 ? r : e * r) - mu[i]);
            b += (c[i] * c[i]) * ((e * r) * r);
        }
        k1 = (double)a; k2 = (double)b;
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
    double q, V, nlp;
    while (scanf("%lld %lf %lf %lf", &n, &q, &V, &nlp) == 4) {
        if (n < 1 || n > 100000000) return 2;
        Col col;
        col.c.resize((size_t)n); col.h.resize((size_t)n);
        for (long long i = 0; i < n; ++i) {
            double c, h;
            if (scanf("%lf %lf", &c, &h) != 2) return 2;
            col.c[(size_t)i] = c; col.h[(size_t)i] = h;
        }
        col.prepare();
        const double smin = (double)(col.neg - col.m1), smax = (double)(col.pos - col.m1), aq = std::fabs(q), tol = kSpaTolF * std::sqrt(V);
        const int obs = q >= 0.0 ? 0 : 1;
        SpaTail tl[2];
        for (int k = 0; k < 2; ++k) {
            const double s = k == 0 ? aq : -aq;
            tl[k] = SpaTail{std::nan(""), std::nan(""), std::nan(""), 0, 0};
            if (!(k == obs || (k == 0 ? s < smax : s > smin))) continue;
            SpaIter it;
            spa_iter_start(it);
            while (it.status == 0) {
                double k1, k2;
                col.k12(it.t, k1, k2);
                spa_iter_step(it, k1, k2, s, tol);
            }
            tl[k].status = it.status; tl[k].evals = it.evals;
            if (it.status == 1) {
                tl[k].t = it.that;
                if (std::isfinite(it.that)) col.k02(it.that, tl[k].K, tl[k].K2);
            }
        }
        double val = 0.0;
        const int state = spa_column(tl, q, V, nlp, &val);
        printf("%d %.17g %.17g %.17g %d %d\n", state, val, tl[0].status == 1 ? tl[0].t : std::nan(""), tl[1].status == 1 ? tl[1].t : std::nan(""),
               tl[0].evals, tl[1].evals);
    }
    return 0;
}
