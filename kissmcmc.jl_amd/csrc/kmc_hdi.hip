// kmc_hdi.hip -- highest-density intervals of a stored chain, scanned on the device: per column the narrowest interval that holds
// k = floor(p N) + 1 consecutive draws of the sorted selection (ArviZ's unimodal rule with the ties and the special values pinned:
// include/kissmcmc_hip.h).  Gather and sort are those of the rank statistics (kmc_rank_host.hpp), on an unsplit
// shape (the sorted-columns service of kmc_rank_host.hpp on a ConvSession opened unsplit: kmc_convergence_host.hpp); the scan over the
// sorted columns is here.  Kernels: kmc_hdi_kernels.hpp.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "kmc_hdi_kernels.hpp"
#include "kmc_rank_host.hpp"

using namespace kmc_rank_host;                               // (and through it kmc_host, kmc_chain_view, kmc_conv_host)
using namespace kmc_hdi;

namespace {

struct HdiBuffers {
    uint64_t *part = nullptr, *out = nullptr;
    ~HdiBuffers() { (void)hipFree(part); (void)hipFree(out); }
};

// the one check of a probability; `name`: what the message calls it
kmc_status check_prob(double p, const std::string& name)
{
    if (!std::isfinite(p) || p <= 0.0 || p >= 1.0) return fail(KMC_ERR_BAD_ARG, "prob must be finite and lie in (0, 1) (" + name + " = " + num(p, "%.17g") + ")");
    return KMC_OK;
}

// k = floor(p n) in double as written, and the refusals that need n beside a checked p
kmc_status span(int64_t n, double p, int64_t* k)
{
    if (n < 2) return fail(KMC_ERR_BAD_ARG, "an interval needs at least 2 draws (N = " + std::to_string(n) + ")");
    if (n >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "2^31 draws or more per column (N = " + std::to_string(n) + ")");
    const int64_t kk = (int64_t)std::floor(p * (double)n);
    if (kk < 1) return fail(KMC_ERR_BAD_ARG, "prob * N < 1: no draw besides the first lies in the interval (prob = " + num(p, "%.17g") + ", N = " + std::to_string(n) + ")");
    if (kk > n - 1) return fail(KMC_ERR_BAD_ARG, "floor(prob * N) = N: no window is left (prob = " + num(p, "%.17g") + ", N = " + std::to_string(n) + ")");
    *k = kk;
    return KMC_OK;
}

template <int P>
void launch_scan(const HdiArgs& a, int64_t ncols, hipStream_t st)
{
    hipLaunchKernelGGL(hdi_scan<P>, dim3((unsigned)a.ntiles, (unsigned)ncols), dim3(kHdiThreads), 0, st, a);
}

kmc_status hdi(const ChainSource& src, int64_t first_sample, const uint8_t* mask_host, const double* probs, int32_t nprob, double* lo, double* hi,
               int64_t* start, int64_t* n_out, int64_t* nan_count, int64_t* info)
{
    HdiBuffers hb;                                            // (before the session: the stream is drained before they go)
    ConvSession S(src);
    SortedColumns sc;                                         // (after it: the service drains the session's live stream itself)
    KMC_TRY(S.describe());
    if (!probs || !lo || !hi || !start) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (nprob < 1 || nprob > kHdiMaxProbs) return fail(KMC_ERR_BAD_ARG, "between 1 and 16 probabilities per call (nprob = " + std::to_string(nprob) + ")");
    for (int p = 0; p < nprob; ++p) KMC_TRY(check_prob(probs[p], "probs[" + std::to_string(p) + "]"));
    int64_t N = 0;
    KMC_TRY(S.unsplit(first_sample, mask_host, &N));          // every selected walker one chain of all selected samples
    if (n_out) *n_out = N;
    const int64_t ncols = S.ncols;
    HdiArgs a{};
    a.N = N; a.nprob = nprob;
    int64_t kmin = 0, windows = 0;
    for (int p = 0; p < nprob; ++p) {
        KMC_TRY(span(N, probs[p], &a.k[p]));
        kmin = p == 0 ? a.k[p] : std::min(kmin, a.k[p]);
        windows += N - a.k[p];
    }
    KMC_TRY(rank_limits(S.sh, ncols));
    a.ntiles = (N - kmin + kHdiTileStarts - 1) / kHdiTileStarts;
    const size_t part_bytes = (size_t)ncols * (size_t)nprob * (size_t)a.ntiles * 2 * sizeof(uint64_t);
    const size_t out_bytes = (size_t)ncols * (size_t)nprob * 3 * sizeof(uint64_t);

    KMC_TRY(S.open(nullptr, nullptr));
    const hipStream_t st = S.st();
    TimedEvents<4> ev;                                        // around the three stages, for info: gather, sort, scan + fold
    if (info) HIP_TRY(ev.create());
    KMC_TRY(sc.sort(S, 0, false, (double)part_bytes + (double)out_bytes, info ? ev.e : nullptr));
    HIP_TRY(hipMalloc((void**)&hb.part, part_bytes));
    HIP_TRY(hipMalloc((void**)&hb.out, out_bytes));
    a.keys = sc.key_a; a.part = hb.part; a.out = hb.out;

    if (nprob == 1) launch_scan<1>(a, ncols, st);
    else if (nprob <= 4) launch_scan<4>(a, ncols, st);
    else launch_scan<kHdiMaxProbs>(a, ncols, st);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hdi_fold, dim3((unsigned)(ncols * nprob)), dim3(kHdiLanes), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (info) HIP_TRY(hipEventRecord(ev.e[3], st));
    std::vector<uint64_t> got((size_t)ncols * (size_t)nprob * 3);
    HIP_TRY(copy_sync(got.data(), hb.out, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    const double nan_v = std::numeric_limits<double>::quiet_NaN();
    for (int64_t c = 0; c < ncols; ++c) {
        if (nan_count) nan_count[c] = sc.nan[(size_t)c];
        for (int p = 0; p < nprob; ++p) {
            const uint64_t* g = &got[(size_t)((c * nprob + p) * 3)];
            const int64_t at = (int64_t)p * ncols + c;
            if (sc.nan[(size_t)c] || g[0] == kHdiNone) {         // a NaN among the draws: no interval
                lo[at] = hi[at] = nan_v;
                start[at] = -1;
            } else {
                lo[at] = unkey(g[1]); hi[at] = unkey(g[2]);
                start[at] = (int64_t)g[0];
            }
        }
    }
    if (info) {
        info[0] = N; info[1] = a.ntiles;
        info[2] = 8 * ncols * ((N - kmin) + windows);         // the scan's loads: key[i] once per start, key[i + k_p] per window
        for (int k = 0; k < 3; ++k) HIP_TRY(ev.elapsed_ns(k, k + 1, &info[3 + k]));
    }
    return KMC_OK;
}

}  // namespace

// k = floor(p n) and the number of windows n - k, with the argument checks of the chain calls.  Touches no device.
KMC_EXPORT kmc_status kmc_hdi_span(int64_t n, double p, int64_t* k, int64_t* nwindows)
{
    int64_t kk = 0;
    KMC_TRY(check_prob(p, "prob"));
    KMC_TRY(span(n, p, &kk));
    if (k) *k = kk;
    if (nwindows) *nwindows = n - kk;
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_hdi(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t with_logp, const double* probs,
                                      int32_t nprob, double* lo, double* hi, int64_t* start, int64_t* n_out, int64_t* nan_count, int64_t* info)
{
    return hdi(ChainSource(s, with_logp != 0, "kmc_chain_hdi"), first_sample, walker_mask, probs, nprob, lo, hi, start, n_out, nan_count, info);
}

KMC_EXPORT kmc_status kmc_chain_hdi(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                    int64_t first_sample, const uint8_t* walker_mask, const double* probs, int32_t nprob, int device, double* lo,
                                    double* hi, int64_t* start, int64_t* n_out, int64_t* nan_count, int64_t* info)
{
    return hdi(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, probs, nprob, lo, hi, start,
               n_out, nan_count, info);
}
