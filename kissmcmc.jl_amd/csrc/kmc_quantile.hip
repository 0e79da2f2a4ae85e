// kmc_quantile.hip -- the effective sample size and the Monte-Carlo standard error of quantiles of a stored chain (Vehtari, Gelman,
// Simpson, Carpenter and Buerkner 2021): the ess of the indicator x <= q_p, and the width of a Beta-distributed rank interval read off
// the sorted draws (include/kissmcmc_hip.h).  The columns are sorted once by the sort of kmc_rank.hip; the
// indicators are bit-packed series whose lag counts are popcounts (kmc_quantile_kernels.hpp); the statistics are kmc_convergence_stats,
// the Beta quantile and the index rule are pure host stages (kmc_quantile_host.hpp).  The two entry points are their checks between the
// steps of a ConvSession (kmc_convergence_host.hpp); the quantiles and the ends of the rank intervals come out of the sorted-columns
// service (kmc_rank_host.hpp), the lag counts grow in the one loop of the family (grow_lags).
#include <algorithm>
#include <limits>
#include <vector>

#include "kmc_quantile_host.hpp"
#include "kmc_quantile_kernels.hpp"
#include "kmc_rank_host.hpp"

using namespace kmc_rank_host;                              // (and through it kmc_host, kmc_chain_view, kmc_conv_host)
using namespace kmc_quantile;
using namespace kmc_quantile_host;

namespace {

int64_t words_of(int64_t h) { return (h + kQindWordBits - 1) / kQindWordBits; }

kmc_status check_probs(int32_t nprobs, const double* probs, bool inside_unit)
{
    if (nprobs < 1 || nprobs > kQindMaxProbs)
        return fail(KMC_ERR_BAD_ARG, "nprobs = " + std::to_string(nprobs) + ": need 1 <= nprobs <= " + std::to_string(kQindMaxProbs));
    if (!probs) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (inside_unit)
        for (int32_t k = 0; k < nprobs; ++k)
            if (!(probs[k] > 0.0 && probs[k] < 1.0))
                return fail(KMC_ERR_BAD_ARG, "probs[" + std::to_string(k) + "] = " + num(probs[k], "%g") + ": a probability must be finite and lie strictly inside (0, 1)");
    return KMC_OK;
}

// the device side of the indicators of one call
struct IndicatorBuffers {
    double* thr = nullptr;
    uint64_t* words = nullptr;
    unsigned long long *ones = nullptr, *counts = nullptr;
    ~IndicatorBuffers() { (void)hipFree(thr); (void)hipFree(words); (void)hipFree(ones); (void)hipFree(counts); }
};

// bytes of the words, the counts of the ones, the lag counters and the thresholds
double indicator_bytes(const ConvShape& sh, int64_t ncols, int32_t nprobs, int64_t max_lags)
{
    const double series = (double)nprobs * (double)ncols;
    return 8.0 * series * ((double)sh.m * (double)words_of(sh.h) + (double)sh.m + (double)max_lags + 1.0);
}

kmc_status indicator_alloc(IndicatorBuffers& ib, const ConvShape& sh, int64_t ncols, int32_t nprobs, int64_t max_lags)
{
    const size_t series = (size_t)nprobs * (size_t)ncols;
    HIP_TRY(hipMalloc((void**)&ib.thr, series * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&ib.words, series * (size_t)sh.m * (size_t)words_of(sh.h) * sizeof(uint64_t)));
    HIP_TRY(hipMalloc((void**)&ib.ones, series * (size_t)sh.m * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void**)&ib.counts, series * (size_t)std::max<int64_t>(max_lags, 1) * sizeof(unsigned long long)));
    return KMC_OK;
}

// thresholds [nprobs][ncols] up, words and ones [nprobs][ncols][m] made; ones to the host
kmc_status pack(IndicatorBuffers& ib, const ConvSession& ses, int32_t nprobs, const double* thr, int64_t* ones)
{
    const ChainView& v = ses.v;
    const ConvShape& sh = ses.sh;
    const ConvBuffers& b = ses.b;
    const hipStream_t st = ses.st();
    const bool with_logp = ses.with_logp;
    const int64_t ncols = ses.ncols, nwords = words_of(sh.h);
    const size_t series = (size_t)nprobs * (size_t)ncols;
    HIP_TRY(copy_sync(ib.thr, thr, series * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(ib.ones, 0, series * (size_t)sh.m * sizeof(unsigned long long), st));
    for (const ConvSource& src : sources(v, with_logp)) {
        PackArgs a{};
        a.src = src.src; a.rank = b.rank; a.thr = ib.thr; a.words = ib.words; a.ones = ib.ones;
        a.first = sh.first; a.half_off = sh.half_off; a.h = sh.h; a.nl = v.nl; a.ld = src.ld; a.np = v.nl * src.ld; a.nw = sh.nw; a.m = sh.m;
        a.nwords = nwords; a.ntile_p = (a.np + kQindThreads - 1) / kQindThreads;
        a.ndim = src.ndim; a.is_float = src.is_float ? 1 : 0; a.col0 = src.col0; a.ncols = (int32_t)ncols; a.nprobs = nprobs;
        const int64_t grid = a.ntile_p * nwords * sh.nhalf;
        if (grid >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one indicator call");
        hipLaunchKernelGGL(qind_pack, dim3((unsigned)grid), dim3(kQindThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts go out as int64");
    HIP_TRY(copy_sync(ones, ib.ones, series * (size_t)sh.m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return KMC_OK;
}

// counts[series * nlags + k] = D_(lag0 + k), k < nlags; *words_read grows by the words the kernel loaded
kmc_status lag_counts(IndicatorBuffers& ib, const ConvShape& sh, int64_t ncols, int32_t nprobs, int64_t lag0, int64_t nlags, hipStream_t st,
                      uint64_t* counts, int64_t* words_read)
{
    if (nlags == 0) return KMC_OK;
    const int64_t nwords = words_of(sh.h), wpc = sh.m * nwords, series = (int64_t)nprobs * ncols;
    if (wpc >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one indicator call");
    HIP_TRY(hipMemsetAsync(ib.counts, 0, (size_t)(series * nlags) * sizeof(unsigned long long), st));
    LagCountArgs a{};
    a.words = ib.words; a.counts = ib.counts; a.h = sh.h; a.wpc = (uint32_t)wpc; a.nwords = (uint32_t)nwords;
    a.lag0 = (int32_t)lag0; a.nlags = (int32_t)nlags; a.ncols = (int32_t)ncols;
    const int64_t nchunks = (wpc + kQindChunkWords - 1) / kQindChunkWords;
    hipLaunchKernelGGL(qind_lag_counts, dim3((unsigned)nchunks, (unsigned)ncols, (unsigned)nprobs), dim3(kQindThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(copy_sync(counts, ib.counts, (size_t)(series * nlags) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (words_read) *words_read += series * wpc;
    return KMC_OK;
}

kmc_status indicator_room(const ConvShape& sh, int64_t ncols, int32_t nprobs, int64_t nlags)
{
    const double need = indicator_bytes(sh, ncols, nprobs, nlags) + 64.0 * 1048576.0;
    size_t free_b = 0;
    bool fits = false;
    KMC_TRY(device_fits(need, &fits, &free_b));
    if (!fits)
        return fail(KMC_ERR_UNSUPPORTED, "the indicators of " + std::to_string(nprobs) + " probabilities, " + std::to_string(ncols) + " columns and " +
                                             std::to_string(sh.m) + " chains of " + std::to_string(sh.h) + " samples need " +
                                             std::to_string((int64_t)(need / 1048576.0)) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free");
    return KMC_OK;
}

// ---- the device stage alone ----
kmc_status indicator_lags(const ChainSource& src, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t nprobs, const double* thr,
                          int64_t lag0, int64_t nlags, int64_t* ones, uint64_t* lagcount, int64_t* m_out, int64_t* h_out)
{
    IndicatorBuffers ib;                                      // (before the session: the stream is drained before they go)
    ConvSession S(src);
    KMC_TRY(S.describe());
    KMC_TRY(check_probs(nprobs, thr, false));
    if (!ones || (nlags > 0 && !lagcount)) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(S.chains(first_sample, walker_mask, split != 0));
    KMC_TRY(S.lags(lag0, nlags));
    KMC_TRY(rank_limits(S.sh, S.ncols));
    KMC_TRY(S.open(m_out, h_out));
    KMC_TRY(indicator_room(S.sh, S.ncols, nprobs, nlags));
    KMC_TRY(indicator_alloc(ib, S.sh, S.ncols, nprobs, nlags));
    KMC_TRY(pack(ib, S, nprobs, thr, ones));
    return lag_counts(ib, S.sh, S.ncols, nprobs, lag0, nlags, S.st(), lagcount, nullptr);
}

// ---- the whole thing ----
struct QuantileOut {
    double *quantile, *ess, *mcse, *lower, *upper;            // [nprobs][ncols]
    int64_t* T;
    int32_t* flags;
    bool complete() const { return quantile && ess && mcse && lower && upper && T && flags; }
};

kmc_status quantile_mcse_stage(IndicatorBuffers& ib, const ConvSession& ses, int32_t nprobs, const double* probs, const QuantileOut& o, int64_t* info)
{
    SortedColumns sc;                                         // (dies before the session: it drains the session's live stream itself)
    const ChainView& v = ses.v;
    const ConvShape& sh = ses.sh;
    const int64_t ncols = ses.ncols, S = sh.m * sh.h, series = (int64_t)nprobs * ncols, max_lag = ses.max_lag;
    const double nan_v = std::numeric_limits<double>::quiet_NaN();
    const hipStream_t st = ses.st();
    KMC_TRY(sc.sort(ses, 0, false, indicator_bytes(sh, ncols, nprobs, max_lag) + 32.0 * (double)series));
    KMC_TRY(indicator_alloc(ib, sh, ncols, nprobs, max_lag));
    KMC_TRY(sc.quantiles(probs, nprobs, o.quantile));

    // the indicators, their chain moments from the counts, and the lag counts in the growing blocks of grow_lags until every series' rule has fired
    std::vector<int64_t> ones((size_t)(series * sh.m));
    KMC_TRY(pack(ib, ses, nprobs, o.quantile, ones.data()));
    std::vector<double> mu(ones.size()), s2(ones.size());
    if ((size_t)sh.h < ones.size()) {                        // many chains: the moments of every count 0 .. h once, the same bits
        std::vector<double> tmu((size_t)sh.h + 1), ts2((size_t)sh.h + 1);
        for (int64_t k = 0; k <= sh.h; ++k) indicator_moments(sh.h, k, &tmu[(size_t)k], &ts2[(size_t)k]);
        for (size_t i = 0; i < ones.size(); ++i) {
            if (ones[i] < 0 || ones[i] > sh.h) return fail(KMC_ERR_HIP, "internal: a count of ones outside [0, h]");
            mu[i] = tmu[(size_t)ones[i]]; s2[i] = ts2[(size_t)ones[i]];
        }
    } else {
        for (size_t i = 0; i < ones.size(); ++i) indicator_moments(sh.h, ones[i], &mu[i], &s2[i]);
    }
    std::vector<double> mean((size_t)series), W((size_t)series), B((size_t)series), vp((size_t)series), rhat((size_t)series), mc((size_t)series);
    std::vector<uint64_t> cnt;
    int64_t have = 0, words_read = 0;
    KMC_TRY(grow_lags(
        series, max_lag,
        [&](int64_t lag0, int64_t nlags, double* block, int64_t stride, int64_t out0) {        // the counts are integers below 2^53: exact doubles
            cnt.resize((size_t)(series * nlags));
            KMC_TRY(lag_counts(ib, sh, ncols, nprobs, lag0, nlags, st, cnt.data(), &words_read));
            for (int64_t s = 0; s < series; ++s)
                for (int64_t k = 0; k < nlags; ++k) block[s * stride + out0 + k] = (double)cnt[(size_t)(s * nlags + k)];
            return KMC_OK;
        },
        [&](const double* block, int64_t nlags) {
            return kmc_convergence_stats(sh.m, sh.h, series, mu.data(), s2.data(), block, nlags, max_lag, mean.data(), W.data(), B.data(), vp.data(),
                                         rhat.data(), o.ess, mc.data(), o.T, o.flags);
        },
        o.flags, &have));

    // the rank interval of every quantile, and its ends out of the sorted columns (still in key_a)
    std::vector<char> has((size_t)series, 0);
    std::vector<int64_t> pos((size_t)(2 * series));
    std::vector<uint64_t> got;
    for (int32_t p = 0; p < nprobs; ++p)
        for (int64_t c = 0; c < ncols; ++c) {
            const size_t e = (size_t)(p * ncols + c);
            pos[2 * e] = pos[2 * e + 1] = c * S;
            if (sc.nan[(size_t)c]) {
                o.ess[e] = nan_v; o.T[e] = 0; o.flags[e] = KMC_CONV_HAS_NAN;
                continue;
            }
            double qa, qb;
            int64_t i1, i2;
            if (!quantile_mcse_ranks(S, probs[p], o.ess[e], &qa, &qb, &i1, &i2))
                return fail(KMC_ERR_UNSUPPORTED, "the Beta quantile did not converge for ess = " + num(o.ess[e], "%g") + ", p = " + num(probs[p], "%g"));
            if (i1 < 0) continue;
            has[e] = 1;
            pos[2 * e] = c * S + i1; pos[2 * e + 1] = c * S + i2;
        }
    KMC_TRY(sc.pick_at(pos, &got));
    for (int64_t e = 0; e < series; ++e) {
        o.lower[e] = has[(size_t)e] ? unkey(got[(size_t)(2 * e)]) : nan_v;
        o.upper[e] = has[(size_t)e] ? unkey(got[(size_t)(2 * e + 1)]) : nan_v;
        o.mcse[e] = has[(size_t)e] ? (o.upper[e] - o.lower[e]) / 2.0 : nan_v;
    }
    if (info) {
        int32_t passes = 0;
        (void)kmc_rank_plan(nullptr, nullptr, &passes, nullptr);
        const int64_t elem = v.is_float ? 4 : 8;
        info[0] = have;
        info[1] = (int64_t)passes * 24 * ncols * S;                                                   // one sort: a pass reads the keys twice and writes them once
        info[2] = sh.nhalf * sh.h * sh.nw * (v.ndim * elem + (ses.with_logp ? 8 : 0));
        info[3] = words_read;
    }
    return KMC_OK;
}

kmc_status quantile_mcse(const ChainSource& src, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag, int32_t nprobs,
                         const double* probs, const QuantileOut& o, int64_t* m_out, int64_t* h_out, int64_t* info)
{
    IndicatorBuffers ib;                                      // (before the session: the stream is drained before they go)
    ConvSession S(src);
    KMC_TRY(S.describe());
    KMC_TRY(check_probs(nprobs, probs, true));
    KMC_TRY(S.chains(first_sample, walker_mask, split != 0));
    KMC_TRY(S.max_lag_from(max_lag));
    KMC_TRY(rank_limits(S.sh, S.ncols));
    if (!o.complete()) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(S.open(m_out, h_out));
    return quantile_mcse_stage(ib, S, nprobs, probs, o, info);
}

}  // namespace

// ---- the pure host stages ----
KMC_EXPORT kmc_status kmc_beta_quantile(double prob, double A, double B, double* x)
{
    if (!x) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (!(prob > 0.0 && prob < 1.0)) return fail(KMC_ERR_BAD_ARG, "prob = " + num(prob, "%g") + ": need 0 < prob < 1");
    if (!(A >= 1.0 && A <= std::numeric_limits<double>::max()) || !(B >= 1.0 && B <= std::numeric_limits<double>::max()))
        return fail(KMC_ERR_BAD_ARG, "A = " + num(A, "%g") + ", B = " + num(B, "%g") + ": both must be finite and >= 1");
    if (!beta_quantile(prob, A, B, x)) return fail(KMC_ERR_UNSUPPORTED, "the continued fraction did not converge for A = " + num(A, "%g") + ", B = " + num(B, "%g"));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_quantile_mcse_ranks(int64_t S, double p, double ess, double* a, double* b, int64_t* i1, int64_t* i2)
{
    if (S < 1 || S >= ((int64_t)1 << 52)) return fail(KMC_ERR_BAD_ARG, "S = " + std::to_string(S) + ": need 1 <= S < 2^52");
    if (!(p > 0.0 && p < 1.0)) return fail(KMC_ERR_BAD_ARG, "p = " + num(p, "%g") + ": a probability must be finite and lie strictly inside (0, 1)");
    double qa, qb;
    int64_t r1, r2;
    if (!quantile_mcse_ranks(S, p, ess, &qa, &qb, &r1, &r2))
        return fail(KMC_ERR_UNSUPPORTED, "the Beta quantile did not converge for ess = " + num(ess, "%g") + ", p = " + num(p, "%g"));
    if (a) *a = qa;
    if (b) *b = qb;
    if (i1) *i1 = r1;
    if (i2) *i2 = r2;
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_indicator_moments(int64_t h, int64_t k, double* mu, double* s2)
{
    if (h < 2 || k < 0 || k > h) return fail(KMC_ERR_BAD_ARG, "h = " + std::to_string(h) + ", k = " + std::to_string(k) + ": need h >= 2 and 0 <= k <= h");
    double m_, s_;
    indicator_moments(h, k, &m_, &s_);
    if (mu) *mu = m_;
    if (s2) *s2 = s_;
    return KMC_OK;
}

// The tile shape of the indicator kernels; for tests and benchmarks.  Touches no device.
KMC_EXPORT kmc_status kmc_indicator_plan(int32_t* word_bits, int32_t* threads, int32_t* chunk_words, int32_t* lds_bytes)
{
    if (word_bits) *word_bits = kQindWordBits;
    if (threads) *threads = kQindThreads;
    if (chunk_words) *chunk_words = kQindChunkWords;
    if (lds_bytes) *lds_bytes = kQindLdsBytes;
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_indicator_lags(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                                 int32_t nprobs, const double* thresholds, int64_t lag0, int64_t nlags, int64_t* ones,
                                                 uint64_t* lagcount, int64_t* m_out, int64_t* h_out)
{
    return indicator_lags(ChainSource(s, with_logp != 0, "kmc_chain_indicator_lags"), first_sample, walker_mask, split, nprobs, thresholds, lag0, nlags,
                          ones, lagcount, m_out, h_out);
}

KMC_EXPORT kmc_status kmc_chain_indicator_lags(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                               int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t nprobs,
                                               const double* thresholds, int64_t lag0, int64_t nlags, int device, int64_t* ones,
                                               uint64_t* lagcount, int64_t* m_out, int64_t* h_out)
{
    return indicator_lags(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, split, nprobs, thresholds,
                          lag0, nlags, ones, lagcount, m_out, h_out);
}

KMC_EXPORT kmc_status kmc_sampler_quantile_mcse(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                                int64_t max_lag, int32_t nprobs, const double* probs, double* quantile, double* ess, double* mcse,
                                                double* lower, double* upper, int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out,
                                                int64_t* info)
{
    return quantile_mcse(ChainSource(s, with_logp != 0, "kmc_chain_quantile_mcse"), first_sample, walker_mask, split, max_lag, nprobs, probs,
                         {quantile, ess, mcse, lower, upper, T, flags}, m_out, h_out, info);
}

KMC_EXPORT kmc_status kmc_chain_quantile_mcse(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                              int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag, int32_t nprobs,
                                              const double* probs, int device, double* quantile, double* ess, double* mcse, double* lower,
                                              double* upper, int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info)
{
    return quantile_mcse(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, split, max_lag, nprobs, probs,
                         {quantile, ess, mcse, lower, upper, T, flags}, m_out, h_out, info);
}
