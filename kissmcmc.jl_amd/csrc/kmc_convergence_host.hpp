// kmc_convergence_host.hpp -- what the host side of the convergence diagnostics (kmc_convergence.hip) shares with the rank-normalised
// form built in front of it (kmc_rank.hip): the chains of a request, the work space of one call and the three stages -- chain moments,
// lag sums, the whole thing on a view.  Internal.
#pragma once
#include <cstdint>
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
};

kmc_status conv_shape(const ChainView& v, int64_t first_sample, const uint8_t* mask_host, bool split, ConvShape* sh);
kmc_status resolve_max_lag(const ConvShape& sh, int64_t* max_lag);
kmc_status upload_rank(ConvBuffers& b, const uint8_t* mask_host, int64_t nl, hipStream_t st);
// the whole thing on a view: chain moments once, then lag blocks until every column's rule has fired or max_lag is reached
kmc_status convergence_device(ConvBuffers& b, const ChainView& v, const ConvShape& sh, const uint8_t* mask_host, bool with_logp, int64_t max_lag,
                              const StatsOut& o, int64_t* info);
// the same on the caller's stream, with b.rank uploaded (upload_rank): for a caller that runs many views of one shape
kmc_status convergence_on_stream(ConvBuffers& b, const ChainView& v, const ConvShape& sh, bool with_logp, int64_t max_lag, const StatsOut& o,
                                 int64_t* info, hipStream_t st);

}  // namespace kmc_conv_host
