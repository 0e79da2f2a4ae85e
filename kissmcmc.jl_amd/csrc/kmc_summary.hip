// kmc_summary.hip -- posterior summaries of a stored chain on the device: exact order statistics (kmc_sampler_order_stats,
// kmc_chain_order_stats) and the MAP sample (kmc_sampler_chain_argmax, kmc_chain_argmax).  Kernels: kmc_summary_kernels.hpp.
#include <vector>

#include "kmc_chain_view.hpp"
#include "kmc_summary_kernels.hpp"

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_summary;

// ------------------------------------------------------------------------------------------
// The median, the 16 / 84 % quantiles and the best sample of a run (the summarize_run of reference src/analysis.jl:9-42, commented out
// there) without moving the chain to the host.  Order statistics: a most-significant-digit radix select over the 64-bit keys of
// kmc_summary_kernels.hpp, kSelectPasses passes of {clear the table, count the next digit per slot, scan per slot} enqueued on one
// private stream with no host synchronisation between them, then one copy of the result.  Every pass reads the selected part of the
// chain once for all requested ranks; the columns are cut into groups so that one workgroup's counters (columns x ranks x 256 x 4 B) fit
// 64 KiB of LDS, and the log-densities are one more column.
// ------------------------------------------------------------------------------------------

namespace {

struct SummaryBuffers : ChainUpload {                 // (kmc_chain_view.hpp: the mask, and for kmc_chain_* the uploaded copies)
    unsigned long long* hist = nullptr;
    uint64_t* prefix = nullptr;
    int64_t* krem = nullptr;
    double* out = nullptr;
    double* pv = nullptr;
    int64_t* pi = nullptr;
    ~SummaryBuffers()
    {
        (void)hipFree(hist); (void)hipFree(prefix); (void)hipFree(krem); (void)hipFree(out); (void)hipFree(pv); (void)hipFree(pi);
    }
};

kmc_status order_stats(const ChainSource& src, int64_t first_sample, const uint8_t* mask_host, const int64_t* ranks, int32_t nranks,
                       double* theta_out, double* logp_out, int64_t* n_out)
{
    ChainView v;
    KMC_TRY(src.describe(&v));
    if (!ranks || !theta_out) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (nranks < 1 || nranks > kMaxRanks) return fail(KMC_ERR_BAD_ARG, "between 1 and 16 ranks per call");
    int64_t N = 0;
    KMC_TRY(selection_size(v, first_sample, mask_host, &N));
    if (n_out) *n_out = N;
    for (int r = 0; r < nranks; ++r)
        if (ranks[r] < 0 || ranks[r] >= N) return fail(KMC_ERR_BAD_ARG, "rank " + std::to_string(ranks[r]) + " outside [0, " + std::to_string(N) + ")");
    const bool with_logp = logp_out != nullptr;
    const int64_t ncols = v.ndim + (with_logp ? 1 : 0), nslots = ncols * nranks;
    int cg_shift = 0;                                   // columns per group: the largest power of two with columns x ranks <= kSelectSlots ...
    while ((2 << cg_shift) * nranks <= kSelectSlots) ++cg_shift;
    while (cg_shift > 0 && (1 << (cg_shift - 1)) >= v.ndim) --cg_shift;                 // ... and no wider than the row needs
    const int64_t ngroups_chain = (v.ndim + (1 << cg_shift) - 1) >> cg_shift, ngroups = ngroups_chain + (with_logp ? 1 : 0);
    const int64_t nrows = (v.nsamples - first_sample) * v.nl;
    // workgroups per group: enough to fill the device, few enough that their flushes stay small next to their reads, and so many that no
    // workgroup's 32-bit counters can wrap (fewer than 2^24 steps of at most 256 elements each)
    const int64_t steps_min = (nrows + 255) / 256, steps_max = (nrows + (256 >> cg_shift) - 1) / (256 >> cg_shift);
    int64_t nwg = steps_min < 512 ? steps_min : 512;
    const int64_t need = (steps_max >> 23) + 1;
    if (nwg < need) nwg = need;
    if (nwg < 1) nwg = 1;
    if (ngroups * nwg >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one select");

    SummaryBuffers b;
    KMC_TRY(src.open(b, &v));
    ScopedStream ss;                              // never the legacy stream (kmc_host.hpp: copy_sync)
    HIP_TRY(ss.create());
    const hipStream_t st = ss.st;
    KMC_TRY(upload_mask(b, mask_host, v.nl, st));
    const size_t hist_bytes = (size_t)nslots * kSelectBins * sizeof(unsigned long long);
    HIP_TRY(hipMalloc((void**)&b.hist, hist_bytes));
    HIP_TRY(hipMalloc((void**)&b.prefix, (size_t)nslots * sizeof(uint64_t)));
    HIP_TRY(hipMalloc((void**)&b.krem, (size_t)nslots * sizeof(int64_t)));
    HIP_TRY(hipMalloc((void**)&b.out, (size_t)nslots * sizeof(double)));
    std::vector<int64_t> k0((size_t)nslots);
    for (int64_t s = 0; s < nslots; ++s) k0[(size_t)s] = ranks[s % nranks];
    HIP_TRY(copy_sync(b.krem, k0.data(), k0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b.prefix, 0, (size_t)nslots * sizeof(uint64_t), st));

    SelectArgs a{};
    a.chain = v.chain; a.logp = with_logp ? v.logp : nullptr; a.mask = b.mask; a.prefix = b.prefix; a.hist = b.hist;
    a.row0 = first_sample * v.nl; a.nrows = nrows; a.nl = v.nl; a.ld = v.ld;
    a.ndim = (int32_t)v.ndim; a.is_float = v.is_float ? 1 : 0; a.nranks = nranks; a.cg_shift = cg_shift;
    a.ngroups_chain = (int32_t)ngroups_chain; a.nwg = (int32_t)nwg;
    const int64_t cols_g = v.ndim < (1 << cg_shift) ? v.ndim : (1 << cg_shift);
    const unsigned lds = (unsigned)(cols_g * nranks * kSelectBins * sizeof(uint32_t));
    for (int pass = 0; pass < kSelectPasses; ++pass) {
        a.pass = pass;
        HIP_TRY(hipMemsetAsync(b.hist, 0, hist_bytes, st));
        hipLaunchKernelGGL(select_hist, dim3((unsigned)(ngroups * nwg)), dim3(256), lds, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(select_scan, dim3((unsigned)nslots), dim3(kSelectBins), 0, st, b.hist, b.prefix, b.krem, b.out, (int)nranks, pass);
        HIP_TRY(hipGetLastError());
    }
    std::vector<double> out((size_t)nslots);
    HIP_TRY(copy_sync(out.data(), b.out, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    for (int r = 0; r < nranks; ++r) {                  // slot = column * nranks + rank
        for (int64_t d = 0; d < v.ndim; ++d) theta_out[(int64_t)r * v.ndim + d] = out[(size_t)(d * nranks + r)];
        if (with_logp) logp_out[r] = out[(size_t)(v.ndim * nranks + r)];
    }
    return KMC_OK;
}

kmc_status argmax(const ChainSource& src, int64_t first_sample, const uint8_t* mask_host, int64_t* sample, int64_t* walker, double* theta, double* logp)
{
    ChainView v;
    KMC_TRY(src.describe(&v));
    if (!sample || !walker || !theta || !logp) return fail(KMC_ERR_BAD_ARG, "null argument");
    int64_t N = 0;
    KMC_TRY(selection_size(v, first_sample, mask_host, &N));
    const int64_t nrows = (v.nsamples - first_sample) * v.nl;
    int64_t np = (nrows + 2047) / 2048;
    if (np > 1024) np = 1024;
    SummaryBuffers b;
    KMC_TRY(src.open(b, &v));
    ScopedStream ss;
    HIP_TRY(ss.create());
    const hipStream_t st = ss.st;
    KMC_TRY(upload_mask(b, mask_host, v.nl, st));
    HIP_TRY(hipMalloc((void**)&b.pv, (size_t)np * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&b.pi, (size_t)np * sizeof(int64_t)));
    HIP_TRY(hipMalloc((void**)&b.out, (size_t)(v.ndim + 2) * sizeof(double)));
    hipLaunchKernelGGL(argmax_partial, dim3((unsigned)np), dim3(256), 0, st, v.logp, (const uint8_t*)b.mask, first_sample * v.nl, nrows, v.nl, b.pv, b.pi);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(argmax_final, dim3(1), dim3(256), 0, st, (const double*)b.pv, (const int64_t*)b.pi, (int)np, v.chain, v.is_float ? 1 : 0, v.ld, (int)v.ndim, b.out);
    HIP_TRY(hipGetLastError());
    std::vector<double> res((size_t)v.ndim + 2);
    HIP_TRY(copy_sync(res.data(), b.out, res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    int64_t idx;
    std::memcpy(&idx, &res[(size_t)v.ndim + 1], sizeof(idx));
    if (idx < 0) return fail(KMC_ERR_BAD_ARG, "every selected log-density is NaN");
    std::memcpy(theta, res.data(), (size_t)v.ndim * sizeof(double));
    *logp = res[(size_t)v.ndim];
    *sample = idx / v.nl;
    *walker = idx % v.nl;
    return KMC_OK;
}

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_order_stats(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, const int64_t* ranks, int32_t nranks,
                                              double* theta_out, double* logp_out, int64_t* n_out)
{
    return order_stats(ChainSource(s, logp_out != nullptr, "kmc_chain_order_stats"), first_sample, walker_mask, ranks, nranks, theta_out,
                       logp_out, n_out);
}

KMC_EXPORT kmc_status kmc_sampler_chain_argmax(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t* sample, int64_t* walker,
                                               double* theta, double* logp)
{
    return argmax(ChainSource(s, true, "kmc_chain_argmax"), first_sample, walker_mask, sample, walker, theta, logp);
}

KMC_EXPORT kmc_status kmc_chain_order_stats(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                            int64_t first_sample, const uint8_t* walker_mask, const int64_t* ranks, int32_t nranks, int device,
                                            double* theta_out, double* logp_out, int64_t* n_out)
{
    if (logp_out && !logp_host) return fail(KMC_ERR_BAD_ARG, "logp_out without logp_host");
    return order_stats(ChainSource(chain_host, logp_out ? logp_host : nullptr, nsamples, nwalkers, ndim, device), first_sample, walker_mask,
                       ranks, nranks, theta_out, logp_out, n_out);               // (the log-densities are uploaded only when asked for)
}

KMC_EXPORT kmc_status kmc_chain_argmax(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                       int64_t first_sample, const uint8_t* walker_mask, int device, int64_t* sample, int64_t* walker, double* theta,
                                       double* logp)
{
    if (!logp_host) return fail(KMC_ERR_BAD_ARG, "null argument");
    return argmax(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, sample, walker, theta, logp);
}
