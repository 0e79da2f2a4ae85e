// kmc_quantile_host.hpp -- the pure host stages of the Monte-Carlo standard error of quantiles (kmc_quantile.hip; include/kissmcmc_hip.h;
// DESIGN.md section 4o): the quantile function of the Beta distribution, the rank interval that follows from it, and the chain moments
// of an indicator from its count.  Standard C++ only, no HIP: tests/sanitize/beta_quantile_main.cpp includes it on its own.  Internal.
//
// Every expression is formed as written (the library and the stand-alone program are built with -ffp-contract=off); the only library
// functions are log, log1p, exp, sqrt, lgamma, floor, ceil and nextafter.  Equal inputs give equal bits on every run.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

namespace kmc_quantile_host {

constexpr double kPhiMinus1 = 0.15865525393145707;         // Phi(-1)
constexpr double kPhiPlus1 = 0.8413447460685429;           // Phi(+1)
constexpr double kStirlingFrom = 10.0;                     // from here on log Gamma goes by Stirling's series
constexpr int kBetaCfMaxIter = 4000000;                    // the continued fraction needs O(sqrt(max(A, B))) terms
constexpr int kBetaInvMaxIter = 200;

// Delta(z) = log Gamma(z) - [(z - 1/2) log z - z + log(2 pi) / 2], z >= 10: five terms, the sixth is below 1e-14 there
inline double stirling_delta(double z)
{
    const double w = 1.0 / (z * z);
    return ((((8.417508417508417508e-4 * w - 5.952380952380952381e-4) * w + 7.936507936507936508e-4) * w - 2.777777777777777778e-3) * w +
            8.333333333333333333e-2) / z;
}

// e - log(1 + e), e > -1: the series e^2/2 - e^3/3 + ... where the difference would cancel
inline double rlog1(double e)
{
    if (std::fabs(e) >= 0.01) return e - std::log1p(e);
    return e * e * (1.0 / 2.0 - e * (1.0 / 3.0 - e * (1.0 / 4.0 - e * (1.0 / 5.0 - e * (1.0 / 6.0 - e * (1.0 / 7.0 - e * (1.0 / 8.0 - e * (1.0 / 9.0 -
           e * (1.0 / 10.0)))))))));
}

// log[ x^a y^b / B(a, b) ], y = 1 - x, a, b >= 1, 0 < x < 1.  Three forms, by which of a and b have reached kStirlingFrom:
//   neither   log Gamma from the C library;
//   one       the small one from the C library, log Gamma(big) - log Gamma(small + big) by Stirling's series, without the cancellation;
//   both      TOMS 708's BRCOMP: lambda = a - (a + b) x, -(a rlog1(-lambda / a) + b rlog1(lambda / b)) + log(a b / (a + b)) / 2
//             - log(2 pi) / 2 - [Delta(a) + Delta(b) - Delta(a + b)]: nothing of the size of a log x is ever formed.
inline double log_beta_term(double a, double b, double x, double y)
{
    const double lx = x < 0.5 ? std::log(x) : std::log1p(-y), ly = x < 0.5 ? std::log1p(-x) : std::log(y);
    if (a < kStirlingFrom && b < kStirlingFrom) return a * lx + b * ly + ((std::lgamma(a + b) - std::lgamma(a)) - std::lgamma(b));
    if (a < kStirlingFrom || b < kStirlingFrom) {
        const double s = a < b ? a : b, g = a < b ? b : a;
        const double diff = (g - 0.5) * std::log1p(s / g) + s * (std::log(s + g) - 1.0) + (stirling_delta(s + g) - stirling_delta(g));
        return a * lx + b * ly + (diff - std::lgamma(s));
    }
    const double lambda = a <= b ? a - (a + b) * x : (a + b) * y - b;
    const double u = rlog1(-lambda / a), v = rlog1(lambda / b);
    const double corr = (stirling_delta(a) + stirling_delta(b)) - stirling_delta(a + b);
    return -(a * u + b * v) + 0.5 * std::log(a * b / (a + b)) - 0.918938533204672742 - corr;
}

// the continued fraction of the incomplete beta function (Numerical Recipes' betacf: the modified Lentz method), to two ulp of a factor
inline double beta_cf(double a, double b, double x, bool* converged)
{
    const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= kBetaCfMaxIter; ++m) {
        const double fm = (double)m, m2 = 2.0 * fm;
        double aa = fm * (b - fm) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + fm) * (qab + fm) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) <= 4.5e-16) return h;
    }
    *converged = false;
    return h;
}

// I_x(a, b) - prob, and the density of Beta(a, b) at x.  The fraction is taken on the side of the mode where it converges fast
// (x < (a + 1) / (a + b + 2), else for 1 - x with a and b exchanged) and the difference is formed on that side.
inline double beta_cdf_minus(double a, double b, double x, double prob, double* pdf, bool* converged)
{
    const double y = 1.0 - x, term = std::exp(log_beta_term(a, b, x, y));
    *pdf = term / (x * y);
    if (x < (a + 1.0) / (a + b + 2.0)) return term * beta_cf(a, b, x, converged) / a - prob;
    return (1.0 - prob) - term * beta_cf(b, a, y, converged) / b;
}

// The quantile function of Beta(A, B): the x with I_x(A, B) = prob.  0 < prob < 1, A, B >= 1 and finite (checked by the caller).
// Newton's iteration on I_x - prob from the normal approximation mean -+ sd, kept inside a bracket that every evaluation narrows, a
// bisection step whenever Newton's leaves the bracket; it ends when the step no longer changes x or the bracket's ends are neighbours,
// after at most kBetaInvMaxIter evaluations.  false: the continued fraction did not converge.
inline bool beta_quantile(double prob, double A, double B, double* out)
{
    double lo = 0.0, hi = 1.0;
    const double mu = A / (A + B), sd = std::sqrt(mu * (1.0 - mu) / (A + B + 1.0));
    double x = mu + (prob < 0.5 ? -sd : sd);
    if (!(x > 0.0)) x = 0.5 * mu;
    if (!(x < 1.0)) x = 0.5 * (1.0 + mu);
    bool converged = true;
    for (int it = 0; it < kBetaInvMaxIter; ++it) {
        double pdf = 0.0;
        const double f = beta_cdf_minus(A, B, x, prob, &pdf, &converged);
        if (!converged) return false;
        if (f == 0.0) break;
        if (f < 0.0) lo = x; else hi = x;
        if (std::nextafter(lo, hi) >= hi) break;
        double next = x - f / pdf;
        if (!(next > lo && next < hi)) next = lo + 0.5 * (hi - lo);
        if (next == x) break;
        x = next;
    }
    *out = x;
    return true;
}

// The rank interval of the quantile p among S draws of effective size ess (include/kissmcmc_hip.h): A = ess p + 1, B = ess (1 - p) + 1,
// a = Bq(Phi(-1); A, B), b = Bq(Phi(1); A, B), i1 = max(floor(a S), 1) - 1, i2 = min(ceil(b S), S) - 1.  ess NaN or <= 0: a = b = NaN,
// i1 = i2 = -1.  false: the continued fraction did not converge.
inline bool quantile_mcse_ranks(int64_t S, double p, double ess, double* a, double* b, int64_t* i1, int64_t* i2)
{
    *a = *b = std::numeric_limits<double>::quiet_NaN();
    *i1 = *i2 = -1;
    if (!(ess > 0.0) || !(ess <= std::numeric_limits<double>::max())) return true;
    const double A = ess * p + 1.0, B = ess * (1.0 - p) + 1.0;
    if (!beta_quantile(kPhiMinus1, A, B, a) || !beta_quantile(kPhiPlus1, A, B, b)) return false;
    const double fa = std::floor(*a * (double)S), cb = std::ceil(*b * (double)S);
    *i1 = (int64_t)(fa > 1.0 ? fa : 1.0) - 1;
    *i2 = (int64_t)(cb < (double)S ? cb : (double)S) - 1;
    if (*i2 < 0) *i2 = 0;                                    // (b S underflowed to 0: not reachable with A >= 1)
    return true;
}

// chain mean and variance of an indicator with k ones among h samples: mu = k / h, ss = k ((1 - mu)(1 - mu)) + (h - k)(mu mu),
// s2 = ss / (h - 1), every operation rounded on its own in this order
inline void indicator_moments(int64_t h, int64_t k, double* mu, double* s2)
{
    const double m = (double)k / (double)h, om = 1.0 - m;
    const double ss = (double)k * (om * om) + (double)(h - k) * (m * m);
    *mu = m;
    *s2 = ss / (double)(h - 1);
}

}  // namespace kmc_quantile_host
