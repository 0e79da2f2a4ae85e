// kmc_convergence_host.hpp -- what the host sides of the read-outs built on the chains of a stored chain share (kmc_convergence.hip,
// kmc_rank.hip, kmc_quantile.hip, kmc_hdi.hip, and the relative-efficiency stage of kmc_pointwise.hip): the chains of a request, the
// work space of one call, the session every entry point of the family opens in steps, and the stages -- chain moments, lag sums, the
// lag-growth loop, the whole thing on a view.  Internal.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "kmc_chain_view.hpp"

namespace kmc_conv_host {

using namespace kmc_host;
using namespace kmc_chain_view;

// the chains of a request (include/kissmcmc_hip.h): from the sizes alone
struct ConvShape {
    int64_t first = 0, n = 0, nw = 0, h = 0, m = 0, half_off = 0;
    int nhalf = 1;
};

struct ConvBuffers : ChainUpload {
    int32_t* rank = nullptr;
    double *mean_p = nullptr, *part = nullptr, *out = nullptr;
    size_t mean_bytes = 0, part_bytes = 0, out_bytes = 0;
    ~ConvBuffers() { (void)hipFree(rank); (void)hipFree(mean_p); (void)hipFree(part); (void)hipFree(out); }
    kmc_status room(double** p, size_t* have, size_t need)
    {
        if (need <= *have) return KMC_OK;
        (void)hipFree(*p);
        *p = nullptr; *have = 0;
        KMC_TRY(check_device_room(need, "the convergence work space"));
        HIP_TRY(hipMalloc((void**)p, need));
        *have = need;
        return KMC_OK;
    }
};

// one source of columns: the chain, or the log-densities as a chain of ld = ndim = 1
struct ConvSource {
    const void* src;
    bool is_float;
    int64_t ld;
    int32_t ndim, col0;
};

inline std::vector<ConvSource> sources(const ChainView& v, bool with_logp)
{
    std::vector<ConvSource> s;
    s.push_back({v.chain, v.is_float, v.ld, (int32_t)v.ndim, 0});
    if (with_logp) s.push_back({v.logp, false, 1, 1, (int32_t)v.ndim});
    return s;
}

// Per column, every sum sequential in index order; no device.
struct StatsOut {
    double *mean, *W, *B, *var_plus, *rhat, *ess, *mcse;
    int64_t* T;
    int32_t* flags;
    bool complete() const { return mean && W && B && var_plus && rhat && ess && mcse && T && flags; }
};

kmc_status conv_shape(const ChainView& v, int64_t first_sample, const uint8_t* mask_host, bool split, ConvShape* sh);
kmc_status check_lags(const ConvShape& sh, int64_t lag0, int64_t nlags);
kmc_status resolve_max_lag(const ConvShape& sh, int64_t* max_lag);
kmc_status upload_rank(ConvBuffers& b, const uint8_t* mask_host, int64_t nl, hipStream_t st);

// One call of the family, by either route.  It opens in steps, and an entry point puts its own argument checks
// between them where its order of refusals has them: describe() -- the sizes of the view; chains() or unsplit() -- the chains of the
// request -- then lags() or max_lag_from() (and rank_limits of kmc_rank_host.hpp for a call that sorts); open() -- the sizes out, the
// pointers of the view (a host chain: uploaded), the stream (ChainSource::stream(): a sampler's own) and the walker-rank map.  Nothing
// before open() touches the device on the host route; a call's room checks follow it.  Members die in reverse order, so the stream is
// drained before the buffers go; a call's further plain buffers are declared BEFORE its session for the same reason (SortedColumns, which
// drains the stream itself, after it).
struct ConvSession {
    const ChainSource& src;
    ChainView v;
    ConvShape sh;
    int64_t ncols = 0, max_lag = 0;
    bool with_logp;
    const uint8_t* mask = nullptr;
    ConvBuffers b;
    ScopedStream ss;

    explicit ConvSession(const ChainSource& src_) : src(src_), with_logp(src_.with_logp) {}
    hipStream_t st() const { return ss.get(); }
    kmc_status describe() { KMC_TRY(src.describe(&v)); ncols = v.ndim + (with_logp ? 1 : 0); return KMC_OK; }
    kmc_status chains(int64_t first, const uint8_t* mask_host, bool split) { mask = mask_host; return conv_shape(v, first, mask_host, split, &sh); }
    // every selected walker one chain of all selected samples, N draws per column in all: no rule on h or m (kmc_hdi.hip)
    kmc_status unsplit(int64_t first, const uint8_t* mask_host, int64_t* N)
    {
        mask = mask_host;
        KMC_TRY(selection_size(v, first, mask_host, N));
        sh = ConvShape{};
        sh.first = first; sh.n = sh.h = v.nsamples - first; sh.nw = sh.m = *N / sh.n;
        return KMC_OK;
    }
    kmc_status lags(int64_t lag0, int64_t nlags) const { return check_lags(sh, lag0, nlags); }
    kmc_status max_lag_from(int64_t asked) { max_lag = asked; return resolve_max_lag(sh, &max_lag); }
    kmc_status open(int64_t* m_out, int64_t* h_out)
    {
        if (m_out) *m_out = sh.m;
        if (h_out) *h_out = sh.h;
        KMC_TRY(src.open(b, &v));
        HIP_TRY(src.stream(&ss));
        return upload_rank(b, mask, v.nl, ss.get());
    }
};

// The lag-growth loop: 32, 64, 128, ... lags in all and at most max_lag; the block of the lags so far [nseries][have] is copied into
// the wider one [nseries][want], `fetch` fills lags have + 1 .. want of every series into it (block[s * stride + out0 + k]), `stats`
// evaluates the statistics of the caller's series on the block and leaves their flags in `flags`; it ends when no series' rule asks for
// more (KMC_CONV_NEED_LAGS; at max_lag the rule reports KMC_CONV_TRUNCATED instead).  *have: the lags fetched in all.
using LagFetch = std::function<kmc_status(int64_t lag0, int64_t nlags, double* block, int64_t stride, int64_t out0)>;
using LagStats = std::function<kmc_status(const double* block, int64_t nlags)>;
kmc_status grow_lags(int64_t nseries, int64_t max_lag, const LagFetch& fetch, const LagStats& stats, const int32_t* flags, int64_t* have);

// the whole thing on a view, on the caller's stream, with b.rank uploaded (upload_rank): chain moments once, then lag blocks until every
// column's rule has fired or max_lag is reached.  A caller that runs many views of one shape keeps its stream and its buffers.
kmc_status convergence_on_stream(ConvBuffers& b, const ChainView& v, const ConvShape& sh, bool with_logp, int64_t max_lag, const StatsOut& o,
                                 int64_t* info, hipStream_t st);

}  // namespace kmc_conv_host
