// skato_tail.h -- the host step and the integrand of SKAT-O, the optimal combination of the burden and the SKAT test of a set
// (mih_assoc_sets_skato).  Plain C++ on top of mixture_tail.h, so that a stand-alone harness can test it on the CPU
// (tests/skato_tail_harness.cpp); the integrand and the log-sum-exp are compiled for the device too (assoc_skato.hip).
// tests/skato_spec.py states the same in numpy; include/mendeliht_hip.h has the definitions in full.
//
// Per set, from the eigenvalues lambda^(rho) of M_rho (R of them) and lambda~ of M~ = M - rs rs' / S, and T, S, Q, rr = rs' rs,
// wt = rs' M~ rs:   Q_rho = (1 - rho) Q + rho (T T),  p_rho = mixture_tail(lambda^(rho), Q_rho),  p_min the smallest (a tie goes to
// the smaller rho),  q_rho the quantile with tail_rho(q_rho) = p_min,  tau_rho = rho S + (1 - rho) rr / S,  mu = sum lambda~,
// v_xi = 4 wt / S (not below 0),  v = 2 sum lambda~^2 + v_xi,  kfac = sqrt((v - v_xi) / v),  u0 = sqrt(min_rho q_rho / tau_rho), and
//     p = 2 int_0^u0 S~(delta'(u^2)) phi(u) du + 2 Phi(-u0),   delta(x) = min_rho (q_rho - tau_rho x) / (1 - rho),
//     delta' = (delta - mu) kfac + mu,   S~ = mixture_tail(lambda~, .), 1 where delta' <= 0.
//
// The quantiles.  For the arg-min rho, q_rho = Q_rho.  For a rank-one lambda^(rho) (state 2), q_rho = lambda_1 z^2 with
// neglog10p_of_z(z) = -log10 p_min: z by bisection from [0, the first power of two whose tail is small enough] until the midpoint
// is an end.  Otherwise the saddlepoint is inverted in its own parameter s = 2 lambda_1 t:  q(s) = lambda_1 g(s) and
// log tail(s) = log Phi(-r(s)) with mixture_tail's w^2, v and near-the-mean limit; r increases in s.  The iteration runs in
// y = 1 / (1 - s), in which q and the log tail are close to linear;  F(y) = log tail(1 - 1 / y) - log p_min:
//     a = 1 / (1 - s_rho), s_rho the saddlepoint of Q_rho (F(a) >= 0 up to rounding, since p_rho >= p_min); evaluate F(a)
//     |F(a)| <= 2^-40 |log p_min| or F(a) < 0: take a -- stop
//     b = 2 a; while F(b) > 0: a = b, b = 2 b
//     repeat (the Illinois rule): y = b - F(b) (b - a) / (F(b) - F(a)), the midpoint if that is not inside (a, b); evaluate F(y)
//         |F(y)| <= 2^-40 |log p_min|: converged -- stop
//         F(y) > 0: a = y, and F(b) is halved if a moved the last time too;  else b = y, and F(a) is halved likewise
//         b - a <= 2^-40 b: converged too, with this y (near the mean the rounding of w^2 = s q + sum log1p(-mu s) leaves F a
//         noise above the first tolerance) -- stop
//     128 evaluations of F in all: not converged -- the set falls back.
//
// The integral: 16 panels of [0, u0] with the 16-point Gauss-Legendre rule in each, one node per thread of the device's
// workgroup, term t = 16 panel + node:  log weight + log S~ + log phi(u) + log(h / 2), h the panel's width.  The 256 terms are
// combined by a fixed pairwise tree of log-sum-exp (for k = 128, 64 .. 1: term[t] = lse(term[t], term[t + k]), t < k), and log 2 is
// added.  delta has up to R - 1 kinks where the minimising rho changes, and the panels are cut there (with 16 equal panels the
// rule loses ten digits on them: 2e-4 against 1e-12 relative in log p).  The kinks (skato_kinks): with a_rho = q_rho / (1 - rho),
// b_rho = tau_rho / (1 - rho), a walk along the lower envelope of the lines a - b x from the line lowest at x = 0 (the steepest
// among equals); the next kink is the nearest crossing ahead with a steeper line (the steepest among equals), until x0 = u0^2.
// The panels (skato_edges): the segments between 0, the kinks (as u = sqrt x) and u0 get one panel each, the remaining panels go
// one at a time to the segment whose panels are widest (the first among equals); a segment's panels are equal.
//
// skato_state:
//     0  no value: m = 0, S <= 0 (or NaN), SKAT state 0, or some p_rho without a value
//     2  rank one, m = 1 or SKAT state 2: the value is neglog10p_skat bit for bit
//     4  fallback: some p_rho came from state 4 (Q_rho <= 0) or 5 (not converged), p_min = 1, a quantile did not converge or the
//        integral is not a number: min(1, R p_min)
//     1  the integral's value
//     3  clamped: the integral left [p_min, R p_min] and was moved to the nearer end
#pragma once
#include "mixture_tail.h"
#include <cmath>
#include <cstdint>

namespace mih {

constexpr int kSkatoMaxRho = 16;
constexpr double kSkatoRhoCap = 0.999;
constexpr int kSkatoDefaultRho = 8;
constexpr double kSkatoDefaultGrid[kSkatoDefaultRho] = {0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0};     // SKAT's optimal.adj
constexpr double kSkatoTolP = 9.094947017729282e-13;      // 2^-40: |log tail - log p_min| <= kSkatoTolP |log p_min|
constexpr int kSkatoMaxEvals = 128;
constexpr int kSkatoPanels = 16, kSkatoNodes = 16;
enum { kSkatoNone = 0, kSkatoIntegral = 1, kSkatoRankOne = 2, kSkatoClamped = 3, kSkatoFallback = 4 };

// ---- the quantiles (host) ------------------------------------------------------------------------------------------------------------
// q = lambda_1 g(s) and the log tail at the saddlepoint parameter s
inline void skato_tail_of_s(int m, const double *lambda, double s, double *q, double *lt)
{
    const double l1 = lambda[0];
    double g, g2, lg = 0.0, s2 = 0.0, s3 = 0.0;
    mix_eval(m, lambda, s, &g, &g2);
    for (int i = 0; i < m; ++i) {
        const double mu = lambda[i] / l1;
        lg = lg + std::log1p(-mu * s);
        s2 = s2 + mu * mu; s3 = s3 + (mu * mu) * mu;
    }
    const double w2 = s * g + lg;
    double r;
    if (!(w2 >= kMixNearMean)) r = (8.0 * s3 / std::pow(2.0 * s2, 1.5)) / 6.0;
    else {
        const double w = std::copysign(std::sqrt(w2), s);
        r = w + std::log((s * std::sqrt(g2 / 2.0)) / w) / w;
    }
    *q = l1 * g; *lt = mix_log_phi_neg(r);
}

struct SkatoQuantile { double q; int ok, evals; };

// the iteration of the header comment; s0: the saddlepoint of a Q whose tail is not below exp(logp)
inline SkatoQuantile skato_quantile(int m, const double *lambda, double s0, double logp)
{
    const double tol = kSkatoTolP * std::fabs(logp);
    SkatoQuantile r = {std::nan(""), 0, 0};
    double a = 1.0 / (1.0 - s0), qa, Fa, b, qb, Fb;
    skato_tail_of_s(m, lambda, 1.0 - 1.0 / a, &qa, &Fa); Fa -= logp; ++r.evals;
    if (std::fabs(Fa) <= tol || Fa < 0.0) { r.q = qa; r.ok = 1; return r; }
    b = 2.0 * a;
    skato_tail_of_s(m, lambda, 1.0 - 1.0 / b, &qb, &Fb); Fb -= logp; ++r.evals;
    while (Fb > 0.0) {
        if (r.evals >= kSkatoMaxEvals) return r;
        a = b; Fa = Fb; b = 2.0 * b;
        skato_tail_of_s(m, lambda, 1.0 - 1.0 / b, &qb, &Fb); Fb -= logp; ++r.evals;
    }
    if (std::fabs(Fb) <= tol) { r.q = qb; r.ok = 1; return r; }
    if (!(Fb < 0.0)) return r;                                   // a NaN
    int side = 0;
    for (;;) {
        if (r.evals >= kSkatoMaxEvals) return r;
        double y = b - Fb * (b - a) / (Fb - Fa), qy, Fy;
        if (!(y > a && y < b)) y = (a + b) / 2.0;
        skato_tail_of_s(m, lambda, 1.0 - 1.0 / y, &qy, &Fy); Fy -= logp; ++r.evals;
        if (std::fabs(Fy) <= tol) { r.q = qy; r.ok = 1; return r; }
        if (Fy > 0.0) { a = y; Fa = Fy; if (side == 1) Fb = Fb / 2.0; side = 1; }
        else if (Fy < 0.0) { b = y; Fb = Fy; if (side == -1) Fa = Fa / 2.0; side = -1; }
        else return r;                                           // a NaN
        if (b - a <= kSkatoTolP * b) { r.q = qy; r.ok = 1; return r; }
    }
}

// lambda_1 z^2 with neglog10p_of_z(z) = nlp (finite, > 0)
inline double skato_chi1_quantile(double l1, double nlp)
{
    double lo = 0.0, hi = 1.0;
    while (neglog10p_of_z(hi) < nlp && hi < 1e300) { lo = hi; hi = 2.0 * hi; }
    for (;;) {
        const double mid = (lo + hi) / 2.0;
        if (!(mid > lo && mid < hi)) break;
        if (neglog10p_of_z(mid) < nlp) lo = mid; else hi = mid;
    }
    return l1 * (hi * hi);
}

// ---- the integrand (host and device) -------------------------------------------------------------------------------------------------
// log(exp(a) + exp(b)); a NaN gives a NaN
MIH_TAIL_FN double skato_lse(double a, double b)
{
    if (std::isnan(a) || std::isnan(b)) return a + b;
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (std::isinf(hi)) return hi;
    return hi + std::log1p(std::exp(lo - hi));
}

// what the integral of a set needs beside lambda~: q_rho, tau_rho and 1 - rho per grid value, mu, kfac, u0 and the panels' edges
struct SkatoIntegrand { int R; double q[kSkatoMaxRho], tau[kSkatoMaxRho], omr[kSkatoMaxRho], mu, kfac, u0, edge[kSkatoPanels + 1]; };

// the kinks of delta in (0, x0), ascending, into x (at most R - 1); returns their count
inline int skato_kinks(const SkatoIntegrand &g, double x0, double *x)
{
    double a[kSkatoMaxRho], b[kSkatoMaxRho];
    for (int r = 0; r < g.R; ++r) { a[r] = g.q[r] / g.omr[r]; b[r] = g.tau[r] / g.omr[r]; }
    int cur = 0, n = 0;
    for (int r = 1; r < g.R; ++r)
        if (a[r] < a[cur] || (a[r] == a[cur] && b[r] > b[cur])) cur = r;
    double at = 0.0;
    for (int step = 0; step < g.R - 1; ++step) {
        int nxt = -1;
        double xn = x0;
        for (int r = 0; r < g.R; ++r)
            if (b[r] > b[cur]) {
                const double xc = (a[r] - a[cur]) / (b[r] - b[cur]);
                if (xc > at && (xc < xn || (xc == xn && nxt >= 0 && b[r] > b[nxt]))) { nxt = r; xn = xc; }
            }
        if (nxt < 0) break;
        x[n++] = xn; cur = nxt; at = xn;
    }
    return n;
}

// the edges of the panels into g.edge
inline void skato_edges(SkatoIntegrand &g)
{
    double pts[kSkatoMaxRho + 1], kx[kSkatoMaxRho];
    const int nk = skato_kinks(g, g.u0 * g.u0, kx), nseg = nk + 1;
    int cnt[kSkatoMaxRho];
    pts[0] = 0.0;
    for (int i = 0; i < nk; ++i) pts[i + 1] = std::sqrt(kx[i]);
    pts[nseg] = g.u0;
    for (int i = 0; i < nseg; ++i) cnt[i] = 1;
    for (int left = kSkatoPanels - nseg; left > 0; --left) {
        int best = 0;
        for (int i = 1; i < nseg; ++i)
            if ((pts[i + 1] - pts[i]) / cnt[i] > (pts[best + 1] - pts[best]) / cnt[best]) best = i;
        ++cnt[best];
    }
    int e = 0;
    for (int i = 0; i < nseg; ++i)
        for (int j = 0; j < cnt[i]; ++j) g.edge[e++] = pts[i] + (pts[i + 1] - pts[i]) * j / cnt[i];
    g.edge[kSkatoPanels] = g.u0;
}

// term t of the integral: log weight + log S~(delta'(u^2)) + log phi(u) + log(h / 2) at node t & 15 of panel t >> 4
MIH_TAIL_FN double skato_term(int t, int m, const double *lam_t, const SkatoIntegrand &g)
{
    const double x16[kSkatoNodes] = {-0.9894009349916499, -0.9445750230732326, -0.8656312023878318, -0.755404408355003, -0.6178762444026438,
                                     -0.45801677765722737, -0.2816035507792589, -0.09501250983763745, 0.09501250983763745, 0.2816035507792589,
                                     0.45801677765722737, 0.6178762444026438, 0.755404408355003, 0.8656312023878318, 0.9445750230732326,
                                     0.9894009349916499};
    const double w16[kSkatoNodes] = {0.027152459411754037, 0.062253523938647706, 0.09515851168249259, 0.12462897125553403, 0.14959598881657676,
                                     0.16915651939500262, 0.1826034150449236, 0.18945061045506859, 0.18945061045506859, 0.1826034150449236,
                                     0.16915651939500262, 0.14959598881657676, 0.12462897125553403, 0.09515851168249259, 0.062253523938647706,
                                     0.027152459411754037};
    const int pnl = t / kSkatoNodes, nd = t % kSkatoNodes;
    const double h = g.edge[pnl + 1] - g.edge[pnl], u = g.edge[pnl] + h * ((x16[nd] + 1.0) / 2.0), x = u * u;
    double d = (g.q[0] - g.tau[0] * x) / g.omr[0];
    for (int r = 1; r < g.R; ++r) {
        const double dr = (g.q[r] - g.tau[r] * x) / g.omr[r];
        if (dr < d) d = dr;
    }
    const double dp = (d - g.mu) * g.kfac + g.mu;
    double ls;
    if (dp > 0.0) ls = -mixture_tail(m, lam_t, dp).neglog10p * 2.302585092994046;
    else ls = dp <= 0.0 ? 0.0 : dp;                              // (a NaN stays one)
    return ((std::log(w16[nd]) + ls) + (-(u * u) / 2.0 - 0.9189385332046727 /* log sqrt(2 pi) */)) + std::log(h / 2.0);
}

// the tree's result to log(2 int): + log 2
MIH_TAIL_FN double skato_scale(double tree) { return tree + 0.6931471805599453; }

// ---- a set (host) ------------------------------------------------------------------------------------------------------------------------
struct SkatoPrep {
    int state;                   // decided before the integral: kSkatoNone, kSkatoRankOne, kSkatoFallback; kSkatoIntegral: pending
    double neglog10p;            // the value where decided
    int rho;                     // index of the arg-min rho (-1 without one)
    double nlp_min;
    SkatoIntegrand g;
};

// grid: R values, capped.  lam_rho: the eigenvalues of M_rho r at lam_rho + r stride (m each), lam_t those of M~.  nlp_rho (R):
// -log10 p_rho, written for every set with members; st_rho (R): their states.
inline SkatoPrep skato_prepare(int m, int R, const double *grid, const double *lam_rho, int64_t stride, const double *lam_t, double Q, double T,
                               double S, double rr, double wt, double nlp_skat, int skat_state, double *nlp_rho, int *st_rho)
{
    const double nan = std::nan("");
    SkatoPrep p;
    p.state = kSkatoNone; p.neglog10p = nan; p.rho = -1; p.nlp_min = nan;
    p.g.R = R; p.g.mu = p.g.kfac = p.g.u0 = nan;
    for (int r = 0; r < R; ++r) { nlp_rho[r] = nan; st_rho[r] = 0; p.g.q[r] = p.g.tau[r] = nan; p.g.omr[r] = 1.0 - grid[r]; }
    for (int i = 0; i <= kSkatoPanels; ++i) p.g.edge[i] = nan;
    if (m < 1) return p;
    double shat[kSkatoMaxRho];
    bool none = false, fall = false;
    for (int r = 0; r < R; ++r) {
        const double *lam = lam_rho + (int64_t)r * stride;
        const MixResult t = mixture_tail(m, lam, (1.0 - grid[r]) * Q + grid[r] * (T * T));
        nlp_rho[r] = t.neglog10p; st_rho[r] = t.state;
        shat[r] = t.t_hat * (2.0 * lam[0]);
        none = none || t.state == 0;
        fall = fall || t.state == 4 || t.state == 5;
    }
    if (!(S > 0.0) || skat_state == 0 || none) return p;
    if (m == 1 || skat_state == 2) { p.state = kSkatoRankOne; p.neglog10p = nlp_skat; return p; }
    int best = 0;
    for (int r = 1; r < R; ++r)
        if (nlp_rho[r] > nlp_rho[best]) best = r;
    p.rho = best;
    const double pmin = nlp_rho[best], fb = std::fmax(0.0, pmin - std::log10((double)R));
    p.nlp_min = pmin;
    p.state = kSkatoFallback; p.neglog10p = fb;
    if (fall || !(pmin > 0.0)) return p;
    const double logp = -pmin * 2.302585092994046;
    for (int r = 0; r < R; ++r) {
        const double *lam = lam_rho + (int64_t)r * stride;
        p.g.tau[r] = grid[r] * S + (1.0 - grid[r]) * rr / S;
        if (r == best) p.g.q[r] = (1.0 - grid[r]) * Q + grid[r] * (T * T);
        else if (st_rho[r] == 2) p.g.q[r] = skato_chi1_quantile(lam[0], pmin);
        else {
            const SkatoQuantile qq = skato_quantile(m, lam, shat[r], logp);
            if (!qq.ok) return p;
            p.g.q[r] = qq.q;
        }
    }
    double mu = 0.0, s2 = 0.0;
    for (int i = 0; i < m; ++i) { mu = mu + lam_t[i]; s2 = s2 + lam_t[i] * lam_t[i]; }
    const double vxi = std::fmax(4.0 * wt / S, 0.0), v = 2.0 * s2 + vxi;
    double x0 = p.g.q[0] / p.g.tau[0];
    for (int r = 1; r < R; ++r) x0 = std::fmin(x0, p.g.q[r] / p.g.tau[r]);
    p.g.mu = mu; p.g.kfac = std::sqrt((v - vxi) / v); p.g.u0 = std::sqrt(x0);
    if (!(p.g.u0 >= 0.0) || !std::isfinite(p.g.u0) || !std::isfinite(p.g.kfac) || !std::isfinite(mu)) return p;
    skato_edges(p.g);
    p.state = kSkatoIntegral; p.neglog10p = nan;
    return p;
}

// li = log(2 int_0^u0 ...) of a pending set: the value and the state after SKAT's clamp
inline void skato_finish(SkatoPrep &p, double li, double *nlp_int)
{
    const double lp = skato_lse(li, 0.6931471805599453 + mix_log_phi_neg(p.g.u0)), val = -lp * 0.4342944819032518;
    const double lowest = p.nlp_min - std::log10((double)p.g.R);
    if (nlp_int) *nlp_int = val;
    if (std::isnan(val)) { p.state = kSkatoFallback; p.neglog10p = std::fmax(0.0, lowest); return; }
    if (val > p.nlp_min) { p.state = kSkatoClamped; p.neglog10p = p.nlp_min; }
    else if (val < lowest) { p.state = kSkatoClamped; p.neglog10p = std::fmax(0.0, lowest); }
    else { p.state = kSkatoIntegral; p.neglog10p = std::fmax(0.0, val); }
}

}  // namespace mih
