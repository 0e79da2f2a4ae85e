// kmc_chain_view.hpp -- what the calls that read a stored chain where it lies share on the host side (kmc_summary.hip, kmc_hist.hip,
// kmc_convergence.hip, kmc_rank.hip, kmc_quantile.hip, kmc_hdi.hip, kmc_pointwise.hip, kmc_psis.hip): the view of a chain on the device, the selection (first_sample, walker mask) and the source of
// such a view -- the chain a sampler holds, or a dense host chain uploaded for the call.  Internal.
#pragma once
#include "kmc_host.hpp"
#include "kmc_sampler.hpp"

namespace kmc_chain_view {

using namespace kmc_host;

struct ChainView {
    const void* chain = nullptr;       // device [nsamples][nl][ld], float or double
    bool is_float = false;
    int64_t ld = 0, ndim = 0;
    const double* logp = nullptr;      // device [nsamples][nl] or nullptr
    int64_t nsamples = 0, nl = 0;
};

// the device copies one call owns: the walker mask, and for kmc_chain_* the uploaded chain and log-densities
struct ChainUpload {
    uint8_t* mask = nullptr;
    double *chain = nullptr, *logp = nullptr;
    ~ChainUpload() { (void)hipFree(mask); (void)hipFree(chain); (void)hipFree(logp); }
};

// N = (nsamples - first_sample) * popcount(mask): what the ranks index
inline kmc_status selection_size(const ChainView& v, int64_t first_sample, const uint8_t* mask_host, int64_t* n)
{
    if (v.nsamples < 0 || v.nl <= 0 || v.ndim <= 0) return fail(KMC_ERR_BAD_ARG, "need nsamples >= 0, nwalkers, ndim > 0");
    if (v.nl >= ((int64_t)1 << 31) || v.ndim >= ((int64_t)1 << 24)) return fail(KMC_ERR_UNSUPPORTED, "chain too large: walkers < 2^31, ndim < 2^24");
    if (first_sample < 0 || first_sample > v.nsamples) return fail(KMC_ERR_BAD_ARG, "first_sample must lie in [0, samples stored]");
    int64_t nw = v.nl;
    if (mask_host) {
        nw = 0;
        for (int64_t w = 0; w < v.nl; ++w) nw += mask_host[w] != 0;
    }
    *n = (v.nsamples - first_sample) * nw;
    if (*n <= 0) return fail(KMC_ERR_BAD_ARG, "the selection is empty: no stored sample at or after first_sample, or no walker in the mask");
    return KMC_OK;
}

inline kmc_status upload_mask(ChainUpload& b, const uint8_t* mask_host, int64_t nl, hipStream_t st)
{
    if (!mask_host) return KMC_OK;
    HIP_TRY(hipMalloc((void**)&b.mask, (size_t)nl));
    HIP_TRY(copy_sync(b.mask, mask_host, (size_t)nl, hipMemcpyHostToDevice, st));
    return KMC_OK;
}

// Where a read-out takes its chain from: the chain a sampler holds, or a dense host chain uploaded for the call.
// Two steps, so that every read-out, by either route, goes describe -> its own argument checks on the sizes -> sizes out (m, h, n) ->
// open -> device work: a host chain is refused from its sizes before the device is touched.
struct ChainSource {
    kmc_sampler* s = nullptr;
    const char* host_call = nullptr;                             // the call for a chain in host memory, for the sampler route's messages
    const double *chain_host = nullptr, *logp_host = nullptr;    // [nsamples][nwalkers][ndim], [nsamples][nwalkers] or nullptr
    int64_t nsamples = 0, nwalkers = 0, ndim = 0;
    int device = 0;
    bool host = false, with_logp = false;                        // with_logp: the log-densities are one more column (host: when they are given)

    ChainSource(kmc_sampler* s_, bool with_logp_, const char* host_call_) : s(s_), host_call(host_call_), with_logp(with_logp_) {}
    ChainSource(const double* chain, const double* logp, int64_t nsamples_, int64_t nwalkers_, int64_t ndim_, int device_)
        : chain_host(chain), logp_host(logp), nsamples(nsamples_), nwalkers(nwalkers_), ndim(ndim_), device(device_), host(true), with_logp(logp != nullptr) {}

    // the sizes of the view.  Host chain: from the arguments alone, no HIP call.  Sampler: its checks, its device made current and its
    // stream drained; the view is complete.
    kmc_status describe(ChainView* v) const
    {
        if (host) {
            if (!chain_host) return fail(KMC_ERR_BAD_ARG, "null argument");
            if (nsamples <= 0 || nwalkers <= 0 || ndim <= 0) return fail(KMC_ERR_BAD_ARG, "need nsamples, nwalkers, ndim > 0");
            v->is_float = false; v->ld = ndim; v->ndim = ndim; v->nsamples = nsamples; v->nl = nwalkers;
            return KMC_OK;
        }
        if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
        if (!s->d_chain) return fail(KMC_ERR_BAD_ARG, "sampler was created without KMC_STORE_CHAIN");
        if (with_logp && !s->d_chain_logp) return fail(KMC_ERR_BAD_ARG, "sampler was created without KMC_STORE_LOGP");
        if (s->stream_chain) return fail(KMC_ERR_UNSUPPORTED, std::string("KMC_STREAM_CHAIN: the chain is on the host; use ") + host_call + " on it");
        if (s->cfg.shard_count > 1 || s->p2p)
            return fail(KMC_ERR_UNSUPPORTED, std::string("sharded sampler: a shard holds only its own walkers and a select across GPUs is not built; gather the chain and use ") + host_call);
        HIP_TRY(hipSetDevice(s->cfg.device));
        HIP_TRY(hipStreamSynchronize(s->stream));
        v->chain = s->d_chain; v->is_float = s->f32; v->ld = s->ld; v->ndim = s->cfg.ndim;
        v->logp = s->d_chain_logp; v->nsamples = samples_done(s); v->nl = s->nlocal;
        return KMC_OK;
    }

    // the pointers of the view.  Host chain: the device, the room and the upload, owned by `b`.  Sampler: nothing left to do.
    kmc_status open(ChainUpload& b, ChainView* v) const
    {
        if (!host) return KMC_OK;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            (void)hipGetLastError();
            return fail(KMC_ERR_NO_DEVICE, "no HIP device visible");
        }
        if (device < 0 || device >= ndev) return fail(KMC_ERR_BAD_ARG, "device ordinal out of range");
        HIP_TRY(hipSetDevice(device));
        size_t free_b = 0;
        bool fits = false;
        const double need = (double)nsamples * (double)nwalkers * ((double)ndim + 1.0) * 8.0 + 64.0 * 1048576.0;
        KMC_TRY(device_fits(need, &fits, &free_b));
        if (!fits)
            return fail(KMC_ERR_UNSUPPORTED, "the chain (" + std::to_string((int64_t)(need / 1048576.0)) + " MiB with its work space) does not fit the device (" +
                                                 std::to_string(free_b >> 20) + " MiB free); streaming a host chain through the device is not built");
        const size_t rows = (size_t)nsamples * (size_t)nwalkers;
        ScopedStream up;
        HIP_TRY(up.create());
        HIP_TRY(hipMalloc((void**)&b.chain, rows * (size_t)ndim * sizeof(double)));
        HIP_TRY(copy_sync(b.chain, chain_host, rows * (size_t)ndim * sizeof(double), hipMemcpyHostToDevice, up.st));
        if (logp_host) {
            HIP_TRY(hipMalloc((void**)&b.logp, rows * sizeof(double)));
            HIP_TRY(copy_sync(b.logp, logp_host, rows * sizeof(double), hipMemcpyHostToDevice, up.st));
        }
        v->chain = b.chain; v->logp = b.logp;
        return KMC_OK;
    }

    // The stream of one call, after describe().  Never the legacy stream (kmc_host.hpp: copy_sync).  A sampler's own stream, which
    // describe() has drained, serves: creating and destroying a stream for the call costs 3.4 to 4.4 ms, several times the two
    // pointwise passes at the README's small shape and more than a whole interval scan at a small one.  Declare `ss` after the call's
    // buffers: the stream is drained before they go.
    hipError_t stream(ScopedStream* ss) const
    {
        if (host || !s->stream) return ss->create();
        ss->borrowed = s->stream;
        return hipSuccess;
    }
};

// kmc_cov.hip: mean [ndim] and covariance [ndim][ndim] (divisor nrows - 1) of dense device rows [nrows][ndim] of doubles, the kernels of
// kmc_chain_covariance on stream `st`; returns after the stream has delivered them.  Bit for bit what kmc_chain_covariance gives on the
// same rows as a chain of one sample and nrows walkers.
kmc_status covariance_of_rows(const double* rows_dev, int64_t nrows, int64_t ndim, hipStream_t st, double* mean, double* cov);

}  // namespace kmc_chain_view
