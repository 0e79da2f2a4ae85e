// kmc_convergence.hip -- convergence diagnostics across chains of a stored chain: split-R^, the effective sample size and the Monte-Carlo
// standard error of the mean (BDA3, Gelman et al. 2014, pp. 284-287; the evaluate_convergence and error_of_estimated_mean that reference
// src/analysis.jl sketches).  Three stages: the device stage (kmc_sampler_lag_sums, kmc_chain_lag_sums: chain means, chain variances and
// the lag sums of the variogram, read from the chain where it lies), the pure host stage (kmc_convergence_stats: everything else, in the
// fixed order of DESIGN.md section 2) and the two in one call (kmc_sampler_convergence, kmc_chain_convergence).  Every entry point is
// its own argument checks between the steps of a ConvSession (kmc_convergence_host.hpp: describe, the chains of the request, open on
// the stream of the source), then its stages; the lag-growth loop of the family (grow_lags) is here.
// Kernels: kmc_convergence_kernels.hpp.
#include <algorithm>
#include <limits>
#include <vector>

#include "kmc_convergence_host.hpp"
#include "kmc_convergence_kernels.hpp"

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_conv;

namespace kmc_conv_host {                  // (kmc_convergence_host.hpp: kmc_rank.hip and kmc_quantile.hip run the same stages on their series)

constexpr int64_t kConvDefaultMaxLag = 1024;
constexpr int64_t kConvTargetWorkgroups = 2048;            // of conv_lag_partials and conv_moment_partials: 8 per compute unit

kmc_status conv_shape(const ChainView& v, int64_t first_sample, const uint8_t* mask_host, bool split, ConvShape* sh)
{
    int64_t N = 0;
    KMC_TRY(selection_size(v, first_sample, mask_host, &N));
    sh->first = first_sample;
    sh->n = v.nsamples - first_sample;
    sh->nw = N / sh->n;
    sh->nhalf = split ? 2 : 1;
    sh->h = split ? sh->n / 2 : sh->n;
    sh->m = sh->nw * sh->nhalf;
    sh->half_off = sh->n - sh->h;                            // the second half ends with the last sample; an odd n leaves the middle one out
    if (sh->h < 4) return fail(KMC_ERR_BAD_ARG, "a chain needs at least 4 samples (h = " + std::to_string(sh->h) + ")");
    if (sh->m < 2) return fail(KMC_ERR_BAD_ARG, "at least 2 chains are needed (m = " + std::to_string(sh->m) + "): select more walkers or split");
    if (sh->h >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chains of 2^31 samples or more");
    return KMC_OK;
}

kmc_status check_lags(const ConvShape& sh, int64_t lag0, int64_t nlags)
{
    if (lag0 < 1 || nlags < 0 || lag0 + nlags - 1 > sh.h - 1)
        return fail(KMC_ERR_BAD_ARG, "the lags lag0 .. lag0 + nlags - 1 must lie in [1, h - 1] (h = " + std::to_string(sh.h) + ")");
    return KMC_OK;
}

kmc_status resolve_max_lag(const ConvShape& sh, int64_t* max_lag)
{
    if (*max_lag == 0) *max_lag = std::min(sh.h - 1, kConvDefaultMaxLag);
    if (*max_lag < 3 || *max_lag > sh.h - 1)
        return fail(KMC_ERR_BAD_ARG, "max_lag must lie in [3, h - 1] (h = " + std::to_string(sh.h) + "), or be 0 for min(h - 1, 1024)");
    return KMC_OK;
}

kmc_status upload_rank(ConvBuffers& b, const uint8_t* mask_host, int64_t nl, hipStream_t st)
{
    std::vector<int32_t> rank((size_t)nl);
    int32_t k = 0;
    for (int64_t w = 0; w < nl; ++w) rank[(size_t)w] = (!mask_host || mask_host[w]) ? k++ : -1;
    HIP_TRY(hipMalloc((void**)&b.rank, rank.size() * sizeof(int32_t)));
    HIP_TRY(copy_sync(b.rank, rank.data(), rank.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return KMC_OK;
}

// chain_mean, chain_var [ncols][m]
kmc_status moments_device(ConvBuffers& b, const ChainView& v, const ConvShape& sh, bool with_logp, hipStream_t st, double* chain_mean, double* chain_var)
{
    const int64_t ncols = v.ndim + (with_logp ? 1 : 0);
    const size_t out_bytes = (size_t)ncols * (size_t)sh.m * sizeof(double);
    KMC_TRY(b.room(&b.out, &b.out_bytes, 2 * out_bytes));
    double* d_mean = b.out;
    double* d_var = b.out + ncols * sh.m;
    for (const ConvSource& src : sources(v, with_logp)) {
        const int64_t np = v.nl * src.ld, gx = (np + kConvThreads - 1) / kConvThreads;
        // chunks of the sample axis: as many as fill the device when the rows are short, of 16 samples or more
        int64_t nchunk = (kConvTargetWorkgroups + gx * sh.nhalf - 1) / (gx * sh.nhalf);
        nchunk = std::max<int64_t>(1, std::min(nchunk, (sh.h + 15) / 16));
        const int64_t clen = (sh.h + nchunk - 1) / nchunk;
        nchunk = (sh.h + clen - 1) / clen;
        if (gx >= ((int64_t)1 << 23) || nchunk * sh.nhalf > 65535) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one convergence call");
        KMC_TRY(b.room(&b.mean_p, &b.mean_bytes, (size_t)sh.nhalf * (size_t)np * sizeof(double)));   // (kept from call to call: a view per group of observations)
        KMC_TRY(b.room(&b.part, &b.part_bytes, (size_t)(sh.nhalf * nchunk) * (size_t)np * sizeof(double)));
        MomentArgs a{};
        a.src = src.src; a.rank = b.rank; a.mean_p = b.mean_p; a.part = b.part;
        a.first = sh.first; a.half_off = sh.half_off; a.h = sh.h; a.nl = v.nl; a.ld = src.ld; a.np = np; a.m = sh.m; a.nw = sh.nw; a.clen = clen;
        a.ndim = src.ndim; a.is_float = src.is_float ? 1 : 0; a.nhalf = sh.nhalf; a.nchunk = (int32_t)nchunk; a.col0 = src.col0;
        for (int pass = 0; pass < 2; ++pass) {
            a.pass = pass;
            a.out = pass == 0 ? d_mean : d_var;
            hipLaunchKernelGGL(conv_moment_partials, dim3((unsigned)gx, (unsigned)(sh.nhalf * nchunk)), dim3(kConvThreads), 0, st, a);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(conv_moment_fold, dim3((unsigned)gx, (unsigned)sh.nhalf), dim3(kConvThreads), 0, st, a);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(copy_sync(chain_mean, d_mean, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(copy_sync(chain_var, d_var, out_bytes, hipMemcpyDeviceToHost, st));
    return KMC_OK;
}

// what one call of lags_device did: for the benchmark (kmc_*_convergence's info)
struct LagWork {
    int64_t lag_blocks = 0, bytes_read = 0;
};

// rows of one window that lie inside the half, summed over the sample tiles: what a selected (walker, column) loads for one lag block
int64_t window_rows(int64_t h, int64_t t0)
{
    const int64_t span = t0 + kConvLagBlock - 1, cur_base = std::min<int64_t>(span, kConvPartnerRows);
    int64_t rows = 0;
    for (int64_t i0 = 0; i0 < h; i0 += kConvTileSamples) {
        if (cur_base < kConvPartnerRows) {                   // one contiguous run of samples [i0 - span, i0 + 32)
            rows += std::min(h, i0 + kConvTileSamples) - std::max<int64_t>(0, i0 - span);
        } else {
            const int64_t lo = std::max<int64_t>(0, i0 - span), hi = std::min(h, i0 - span + kConvPartnerRows);
            rows += std::max<int64_t>(0, hi - lo) + std::min(h, i0 + kConvTileSamples) - i0;
        }
    }
    return rows;
}

// lagsum[c * out_stride + out0 + k] = D_(lag0 + k), k = 0 .. nlags - 1.  The grid of one lag block depends on the shape of the selection
// alone, not on lag0 or nlags, and a lag's additions are ordered by sample, lane and workgroup, not by its place in a block: D_t has the
// same bits however the lags are cut into calls.  At most kConvBlocksPerLaunch lag blocks go into one launch (the partial sums of one
// block are up to 2048 * 32 * 64 doubles).
constexpr int64_t kConvBlocksPerLaunch = 4;

kmc_status lags_device(ConvBuffers& b, const ChainView& v, const ConvShape& sh, bool with_logp, int64_t lag0, int64_t nlags, hipStream_t st,
                       double* lagsum, int64_t out_stride, int64_t out0, LagWork* work)
{
    if (nlags == 0) return KMC_OK;
    const int64_t ncols = v.ndim + (with_logp ? 1 : 0);
    const int64_t nlb = (nlags + kConvLagBlock - 1) / kConvLagBlock, ntile_i = (sh.h + kConvTileSamples - 1) / kConvTileSamples;
    KMC_TRY(b.room(&b.out, &b.out_bytes, (size_t)ncols * (size_t)nlags * sizeof(double)));
    for (const ConvSource& src : sources(v, with_logp)) {
        const int64_t np = v.nl * src.ld, ntile_p = (np + kConvLanes - 1) / kConvLanes;
        int64_t g = src.ld, r = kConvLanes;
        while (r) { const int64_t t = g % r; g = r; r = t; }
        const int64_t period = src.ld / g, per_residue = (ntile_p + period - 1) / period;
        const int64_t nslot = std::min<int64_t>(src.ld, kConvLanes);
        // workgroups along the positions first, then -- short rows -- chunks of the sample axis, until the device is full
        const int64_t nb = std::max<int64_t>(1, std::min(per_residue, kConvTargetWorkgroups / (period * sh.nhalf)));
        int64_t nchunk = (kConvTargetWorkgroups + period * nb * sh.nhalf - 1) / (period * nb * sh.nhalf);
        nchunk = std::max<int64_t>(1, std::min(nchunk, ntile_i));
        const int64_t tpc = (ntile_i + nchunk - 1) / nchunk;
        nchunk = (ntile_i + tpc - 1) / tpc;
        const int64_t gx = period * nb, gy = sh.nhalf * nchunk;
        if (gx * gy * kConvBlocksPerLaunch >= ((int64_t)1 << 23) || gy > 65535) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one convergence call");
        KMC_TRY(b.room(&b.part, &b.part_bytes, (size_t)(gx * gy * std::min(nlb, kConvBlocksPerLaunch)) * kConvLagBlock * (size_t)nslot * sizeof(double)));
        for (int64_t z0 = 0; z0 < nlb; z0 += kConvBlocksPerLaunch) {
            const int64_t nz = std::min(kConvBlocksPerLaunch, nlb - z0), k0 = z0 * kConvLagBlock, nk = std::min<int64_t>(nz * kConvLagBlock, nlags - k0);
            LagArgs a{};
            a.src = src.src; a.rank = b.rank; a.part = b.part;
            a.first = sh.first; a.half_off = sh.half_off; a.h = sh.h; a.nl = v.nl; a.ld = src.ld; a.np = np; a.ntile_p = ntile_p;
            a.ndim = src.ndim; a.is_float = src.is_float ? 1 : 0; a.period = (int32_t)period; a.nb = (int32_t)nb; a.nchunk = (int32_t)nchunk;
            a.tpc = (int32_t)tpc; a.lag0 = (int32_t)(lag0 + k0); a.nslot = (int32_t)nslot;
            hipLaunchKernelGGL(conv_lag_partials, dim3((unsigned)gx, (unsigned)gy, (unsigned)nz), dim3(kConvThreads), kConvLdsBytes, st, a);
            HIP_TRY(hipGetLastError());
            LagFoldArgs f{};
            f.part = b.part; f.out = b.out; f.ld = src.ld; f.nlags_out = nlags; f.gx = (int32_t)gx; f.gy = (int32_t)gy; f.period = (int32_t)period;
            f.nslot = (int32_t)nslot; f.col0 = src.col0; f.lag_out0 = (int32_t)k0;
            hipLaunchKernelGGL(conv_lag_fold, dim3((unsigned)src.ndim, (unsigned)nk), dim3(kConvLanes), 0, st, f);
            HIP_TRY(hipGetLastError());
        }
        if (work) {
            const int64_t elem = src.is_float ? 4 : 8;
            for (int64_t z = 0; z < nlb; ++z) work->bytes_read += window_rows(sh.h, lag0 + z * kConvLagBlock) * sh.nhalf * sh.nw * src.ndim * elem;
        }
    }
    if (work) work->lag_blocks += nlb;
    std::vector<double> o((size_t)ncols * (size_t)nlags);
    HIP_TRY(copy_sync(o.data(), b.out, o.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    for (int64_t c = 0; c < ncols; ++c)
        for (int64_t k = 0; k < nlags; ++k) lagsum[c * out_stride + out0 + k] = o[(size_t)(c * nlags + k)];
    return KMC_OK;
}

// ---- the host stage ----
// Per column, every sum sequential in index order; no device.
kmc_status stats_check(int64_t m, int64_t h, int64_t ncols, const double* chain_mean, const double* chain_var, const double* lagsum, int64_t nlags,
                       int64_t max_lag, const StatsOut& o)
{
    if (!chain_mean || !chain_var || (!lagsum && nlags > 0) || !o.complete()) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (ncols < 1) return fail(KMC_ERR_BAD_ARG, "need ncols >= 1");
    if (h < 4) return fail(KMC_ERR_BAD_ARG, "a chain needs at least 4 samples (h)");
    if (m < 2) return fail(KMC_ERR_BAD_ARG, "at least 2 chains are needed (m)");
    if (max_lag < 3 || max_lag > h - 1) return fail(KMC_ERR_BAD_ARG, "max_lag must lie in [3, h - 1]");
    if (nlags < 0 || nlags > h - 1) return fail(KMC_ERR_BAD_ARG, "nlags must lie in [0, h - 1]");
    return KMC_OK;
}

void stats_host(int64_t m, int64_t h, int64_t ncols, const double* chain_mean, const double* chain_var, const double* lagsum, int64_t nlags,
                int64_t max_lag, const StatsOut& o)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t c = 0; c < ncols; ++c) {
        const double *mu = chain_mean + c * m, *s2 = chain_var + c * m, *D = lagsum ? lagsum + c * nlags : nullptr;
        double sm = 0.0, sw = 0.0, sb = 0.0;
        for (int64_t j = 0; j < m; ++j) sm += mu[j];
        const double mean = sm / (double)m;
        for (int64_t j = 0; j < m; ++j) sw += s2[j];
        const double W = sw / (double)m;
        for (int64_t j = 0; j < m; ++j) {
            const double d = mu[j] - mean;
            sb += d * d;
        }
        const double B_over_h = sb / (double)(m - 1);
        const double frac = (double)(h - 1) / (double)h;
        const double vp = frac * W + B_over_h;
        o.mean[c] = mean; o.W[c] = W; o.B[c] = (double)h * B_over_h; o.var_plus[c] = vp;
        if (W == 0.0) {                                       // a constant chain: nothing to estimate, and no error
            o.rhat[c] = o.ess[c] = o.mcse[c] = nan;
            o.T[c] = 0; o.flags[c] = 0;
            continue;
        }
        o.rhat[c] = std::sqrt(vp / W);
        auto rho = [&](int64_t t) { return 1.0 - (D[t - 1] / ((double)m * (double)(h - t))) / (2.0 * vp); };
        int64_t T = 1;
        int32_t flags = 0;
        for (;;) {
            if (T + 2 > max_lag) { flags |= KMC_CONV_TRUNCATED; break; }
            if (T + 2 > nlags) { flags |= KMC_CONV_NEED_LAGS; break; }
            if (rho(T + 1) + rho(T + 2) < 0.0) break;
            T += 2;
        }
        double S = 0.0;
        for (int64_t t = 1; t <= T && t <= nlags; ++t) S += rho(t);
        const double den = 1.0 + 2.0 * S;
        o.ess[c] = den > 0.0 ? ((double)m * (double)h) / den : nan;
        o.mcse[c] = std::sqrt(vp / o.ess[c]);
        o.T[c] = T; o.flags[c] = flags;
    }
}

// the lag-growth loop (kmc_convergence_host.hpp)
kmc_status grow_lags(int64_t nseries, int64_t max_lag, const LagFetch& fetch, const LagStats& stats, const int32_t* flags, int64_t* have_out)
{
    std::vector<double> lag, next;
    int64_t have = 0;
    for (;;) {
        const int64_t want = std::min(max_lag, have == 0 ? (int64_t)kConvLagBlock : 2 * have);        // 32, 64, 128, ... lags in all
        next.assign((size_t)(nseries * want), 0.0);
        for (int64_t s = 0; s < nseries; ++s) std::copy(lag.begin() + s * have, lag.begin() + (s + 1) * have, next.begin() + s * want);
        KMC_TRY(fetch(have + 1, want - have, next.data(), want, have));
        lag.swap(next);
        have = want;
        KMC_TRY(stats(lag.data(), have));
        bool more = false;
        for (int64_t s = 0; s < nseries; ++s) more = more || (flags[s] & KMC_CONV_NEED_LAGS);
        if (!more) break;                                      // (have == max_lag: the rule reports KMC_CONV_TRUNCATED instead)
    }
    *have_out = have;
    return KMC_OK;
}

// the whole thing on a view, on the caller's stream, with b.rank in place: chain moments once, then lag blocks until every column's rule
// has fired or max_lag is reached
kmc_status convergence_on_stream(ConvBuffers& b, const ChainView& v, const ConvShape& sh, bool with_logp, int64_t max_lag, const StatsOut& o,
                                 int64_t* info, hipStream_t st)
{
    const int64_t ncols = v.ndim + (with_logp ? 1 : 0);
    std::vector<double> cm((size_t)(ncols * sh.m)), cv((size_t)(ncols * sh.m));
    KMC_TRY(moments_device(b, v, sh, with_logp, st, cm.data(), cv.data()));
    LagWork work;
    int64_t have = 0;
    KMC_TRY(grow_lags(
        ncols, max_lag,
        [&](int64_t lag0, int64_t nlags, double* block, int64_t stride, int64_t out0) {
            return lags_device(b, v, sh, with_logp, lag0, nlags, st, block, stride, out0, &work);
        },
        [&](const double* block, int64_t nlags) {
            stats_host(sh.m, sh.h, ncols, cm.data(), cv.data(), block, nlags, max_lag, o);
            return KMC_OK;
        },
        o.flags, &have));
    if (info) {
        const int64_t elem = v.is_float ? 4 : 8;
        info[0] = have; info[1] = work.lag_blocks; info[2] = work.bytes_read;
        info[3] = 2 * sh.nhalf * sh.h * sh.nw * (v.ndim * elem + (with_logp ? 8 : 0));                // the two passes of the chain moments
    }
    return KMC_OK;
}

}  // namespace kmc_conv_host

using namespace kmc_conv_host;

KMC_EXPORT kmc_status kmc_convergence_stats(int64_t m, int64_t h, int64_t ncols, const double* chain_mean, const double* chain_var, const double* lagsum,
                                            int64_t nlags, int64_t max_lag, double* mean, double* W, double* B, double* var_plus, double* rhat,
                                            double* ess, double* mcse, int64_t* T, int32_t* flags)
{
    const StatsOut o{mean, W, B, var_plus, rhat, ess, mcse, T, flags};
    KMC_TRY(stats_check(m, h, ncols, chain_mean, chain_var, lagsum, nlags, max_lag, o));
    stats_host(m, h, ncols, chain_mean, chain_var, lagsum, nlags, max_lag, o);
    return KMC_OK;
}

namespace {

kmc_status lag_sums(const ChainSource& src, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t lag0, int64_t nlags,
                    double* chain_mean, double* chain_var, double* lagsum, int64_t* m_out, int64_t* h_out)
{
    ConvSession S(src);
    KMC_TRY(S.describe());
    if ((chain_mean == nullptr) != (chain_var == nullptr)) return fail(KMC_ERR_BAD_ARG, "chain_mean and chain_var go together: both or neither");
    if (nlags > 0 && !lagsum) return fail(KMC_ERR_BAD_ARG, "null lagsum with nlags > 0");
    KMC_TRY(S.chains(first_sample, walker_mask, split != 0));
    KMC_TRY(S.lags(lag0, nlags));
    KMC_TRY(S.open(m_out, h_out));
    if (chain_mean) KMC_TRY(moments_device(S.b, S.v, S.sh, S.with_logp, S.st(), chain_mean, chain_var));
    return lags_device(S.b, S.v, S.sh, S.with_logp, lag0, nlags, S.st(), lagsum, nlags, 0, nullptr);
}

kmc_status convergence(const ChainSource& src, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag, const StatsOut& o,
                       int64_t* m_out, int64_t* h_out, int64_t* info)
{
    ConvSession S(src);
    KMC_TRY(S.describe());
    KMC_TRY(S.chains(first_sample, walker_mask, split != 0));
    KMC_TRY(S.max_lag_from(max_lag));
    if (!o.complete()) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(S.open(m_out, h_out));
    return convergence_on_stream(S.b, S.v, S.sh, S.with_logp, S.max_lag, o, info, S.st());
}

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_lag_sums(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                           int64_t lag0, int64_t nlags, double* chain_mean, double* chain_var, double* lagsum, int64_t* m_out,
                                           int64_t* h_out)
{
    return lag_sums(ChainSource(s, with_logp != 0, "kmc_chain_lag_sums"), first_sample, walker_mask, split, lag0, nlags, chain_mean, chain_var,
                    lagsum, m_out, h_out);
}

KMC_EXPORT kmc_status kmc_chain_lag_sums(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                         int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t lag0, int64_t nlags, int device,
                                         double* chain_mean, double* chain_var, double* lagsum, int64_t* m_out, int64_t* h_out)
{
    return lag_sums(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, split, lag0, nlags, chain_mean,
                    chain_var, lagsum, m_out, h_out);
}

KMC_EXPORT kmc_status kmc_sampler_convergence(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                              int64_t max_lag, double* mean, double* W, double* B, double* var_plus, double* rhat, double* ess,
                                              double* mcse, int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info)
{
    return convergence(ChainSource(s, with_logp != 0, "kmc_chain_convergence"), first_sample, walker_mask, split, max_lag,
                       {mean, W, B, var_plus, rhat, ess, mcse, T, flags}, m_out, h_out, info);
}

KMC_EXPORT kmc_status kmc_chain_convergence(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                            int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag, int device,
                                            double* mean, double* W, double* B, double* var_plus, double* rhat, double* ess, double* mcse,
                                            int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info)
{
    return convergence(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, split, max_lag,
                       {mean, W, B, var_plus, rhat, ess, mcse, T, flags}, m_out, h_out, info);
}

// The tile shape of the lag kernel; for tests and benchmarks.  Touches no device.
KMC_EXPORT kmc_status kmc_convergence_plan(int32_t* lag_block, int32_t* tile_samples, int32_t* lanes, int32_t* lds_bytes)
{
    if (lag_block) *lag_block = kConvLagBlock;
    if (tile_samples) *tile_samples = kConvTileSamples;
    if (lanes) *lanes = kConvLanes;
    if (lds_bytes) *lds_bytes = kConvLdsBytes;
    return KMC_OK;
}
