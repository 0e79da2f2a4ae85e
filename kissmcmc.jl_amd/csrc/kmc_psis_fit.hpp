// kmc_psis_fit.hpp -- the arithmetic of Pareto-smoothed importance sampling for one observation, compiled for both sides: the device's
// fit kernel (kmc_pointwise.hpp: psis_fit_kernel) and the host form (kmc_psis_smooth_host, tests/sanitize/psis_fit_main.cpp).  The two
// differ in their exp / log / log1p / expm1 and in nothing else: every sum below runs in an order that is a function of its length
// alone.  include/kissmcmc_hip.h has the definition (steps 3 to 5), DESIGN.md section 4l the plan.
//
// A context Ctx supplies the two loops:
//     ctx.par(count, f)   -- f(t) for every t in [0, count); the calls are independent (the device spreads them over kFitLanes threads)
//     ctx.sum(count, f)   -- lane l of kFitLanes adds f(l), f(l + kFitLanes), ... in that order from 0.0; the kFitLanes partials are
//                            folded by halving: p[l] += p[l + h] for h = kFitLanes / 2, ..., 1.  Every caller gets the same value.
//     ctx.set(array, i, v) + ctx.sync() -- one write of a value every caller holds, visible after the sync
// On the device every thread of the workgroup runs psis_fit with the same arguments; the scalars are uniform.
#pragma once
#ifndef __HIPCC_RTC__
#include <cmath>
#endif
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define KMC_PSIS_HD __host__ __device__
#else
#define KMC_PSIS_HD
#endif

namespace kmc_psis {

constexpr int kFitLanes = 256;                          // threads of the fit kernel's workgroup; the lanes of every sum
constexpr int kMaxTail = 4096;                          // M at most: the tail of one observation is sorted in one workgroup's LDS
constexpr int kMinFit = 5;                              // tails of fewer draws are not fitted: k = +inf, raw weights
constexpr int kMaxGrid = 30 + 64;                       // m_est = 30 + floor(sqrt(nt)) at nt = kMaxTail
constexpr double kLogDblMin = -0x1.6232bdd7abcd2p+9;    // log(DBL_MIN) = -708.3964185322641, rounded to nearest
constexpr double kTenEps = 10.0 * 2.220446049250313e-16;
constexpr int kSelectBits = 4;                          // the select's digit: 16 counters a lane
constexpr int kSelectBins = 1 << kSelectBits;
constexpr int kSelectPasses = 64 / kSelectBits;

struct FitScratch { double *b, *L, *w; };               // [kMaxGrid] each
struct FitResult { double k, sigma, w_tail, n_tail; };  // w_tail = sum exp(s_i), n_tail = sum exp(s_i - x_(i))

// x: the tail's shifted log ratios, ascending, [nt].  e: work space [nt]; on return the smoothed s_i (x_(i) itself where the tail is not
// smoothed).  xc: the cut-off.
template <class Ctx>
KMC_PSIS_HD FitResult psis_fit(Ctx& ctx, const double* x, double* e, int nt, double xc, const FitScratch& sc)
{
    FitResult r;
    r.k = __builtin_inf();
    r.sigma = __builtin_nan("");
    const double dnt = (double)nt;
    if (nt >= kMinFit) {
        const double exc = exp(xc);
        ctx.par(nt, [&](int t) { e[t] = exp(x[t]) - exc; });
        const int m_est = 30 + (int)floor(sqrt(dnt));
        const double dm = (double)m_est;
        const double scale = 3.0 * e[(int)(dnt / 4.0 + 0.5) - 1], inv_max = 1.0 / e[nt - 1];
        ctx.par(m_est, [&](int i) { sc.b[i] = (1.0 - sqrt(dm / ((double)(i + 1) - 0.5))) / scale + inv_max; });
        for (int i = 0; i < m_est; ++i) {
            const double bi = sc.b[i];
            const double kap = ctx.sum(nt, [&](int t) { return log1p(-bi * e[t]); }) / dnt;
            ctx.set(sc.L, i, dnt * (log(-bi / kap) - kap - 1.0));
        }
        ctx.sync();
        for (int i = 0; i < m_est; ++i) {
            const double Li = sc.L[i];
            ctx.set(sc.w, i, 1.0 / ctx.sum(m_est, [&](int q) { return exp(sc.L[q] - Li); }));
        }
        ctx.sync();
        double wsum = 0.0, bbar = 0.0;
        for (int i = 0; i < m_est; ++i) if (sc.w[i] >= kTenEps) wsum += sc.w[i];
        for (int i = 0; i < m_est; ++i) if (sc.w[i] >= kTenEps) bbar += sc.b[i] * (sc.w[i] / wsum);
        const double kbar = ctx.sum(nt, [&](int t) { return log1p(-bbar * e[t]); }) / dnt;
        r.sigma = -kbar / bbar;
        r.k = (dnt * kbar + 5.0) / (dnt + 10.0);
        if (r.k - r.k == 0.0) {                                                       // finite: smooth
            const bool ok = r.sigma > 0.0 && r.sigma - r.sigma == 0.0;
            const double k = r.k, sigma = r.sigma;
            ctx.par(nt, [&](int t) {
                const double p = ((double)(t + 1) - 0.5) / dnt;
                const double s = log(sigma * expm1(-k * log1p(-p)) / k + exc);
                e[t] = ok ? (s < 0.0 || s != s ? s : 0.0) : __builtin_nan("");
            });
        } else {
            ctx.par(nt, [&](int t) { e[t] = x[t]; });
        }
    } else {
        ctx.par(nt, [&](int t) { e[t] = x[t]; });
    }
    r.w_tail = ctx.sum(nt, [&](int t) { return exp(e[t]); });
    r.n_tail = ctx.sum(nt, [&](int t) { return exp(e[t] - x[t]); });
    return r;
}

// step 5: elpd_loo_j from the shift m, the sum of the raw weights outside the tail, and the fit's two sums
KMC_PSIS_HD inline double psis_elpd(double m, double nontail, long long n, int nt, const FitResult& r)
{
    const double W = nontail + r.w_tail, N = (double)(n - nt) + r.n_tail;
    return m + log(N / W);
}

#ifndef __HIPCC_RTC__
// the tail length of n rows: ceil(min(0.2 n, 3 sqrt(n / r_eff)))
inline long long tail_length(long long n, double r_eff)
{
    const double a = 0.2 * (double)n, b = 3.0 * std::sqrt((double)n / r_eff);
    return (long long)std::ceil(a < b ? a : b);
}

// the host's context: the same lanes and the same fold, one after the other
struct HostCtx {
    template <class Fn> void par(int count, Fn f) { for (int t = 0; t < count; ++t) f(t); }
    template <class Fn> double sum(int count, Fn f)
    {
        double p[kFitLanes];
        for (int l = 0; l < kFitLanes; ++l) {
            double acc = 0.0;
            for (int t = l; t < count; t += kFitLanes) acc += f(t);
            p[l] = acc;
        }
        for (int h = kFitLanes / 2; h > 0; h >>= 1)
            for (int l = 0; l < h; ++l) p[l] += p[l + h];
        return p[0];
    }
    void set(double* a, int i, double v) { a[i] = v; }
    void sync() {}
};
#endif

}  // namespace kmc_psis
