// kmc_hist.hip -- marginal histograms of a stored chain on the device: the 1-D histogram of every selected column and, on request, the
// 2-D histogram of every pair of them -- the numbers of a corner plot (kmc_sampler_histograms, kmc_chain_histograms).
// Kernels: kmc_hist_kernels.hpp.
#include <vector>

#include "kmc_chain_view.hpp"
#include "kmc_hist_kernels.hpp"

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_hist;

// ------------------------------------------------------------------------------------------
// One launch of hist1d reads the selected rows once for all selected columns (and the log-densities); one launch of hist2d reads them
// once per GROUP of pairs, a group being as many pairs as have their counters in one workgroup's LDS (plan2).  Both on one private stream,
// then one copy of the counts.  The selection (first_sample, walker mask) and the two sources of a chain are those of the order
// statistics (kmc_chain_view.hpp).
// ------------------------------------------------------------------------------------------

namespace {

struct HistBuffers : ChainUpload {
    double* edges = nullptr;
    int32_t *slot_of_col = nullptr, *groups = nullptr, *dims = nullptr;
    uint8_t* pair_ab = nullptr;
    unsigned long long *out1 = nullptr, *out2 = nullptr;
    ~HistBuffers()
    {
        (void)hipFree(edges); (void)hipFree(slot_of_col); (void)hipFree(groups); (void)hipFree(dims); (void)hipFree(pair_ab);
        (void)hipFree(out1); (void)hipFree(out2);
    }
};

// hist1d: columns per group (a power of two, 1 << shift) and counter copies, from the LDS budget.  A column costs its edges and one set of
// counters per copy.  The widest group that fits with one copy and that the row needs; then, as long as a group stays 8 columns (64-byte
// pieces of a row of doubles) or more, it is halved until every wave has a copy of its own.
void plan1(int nbins, int64_t ndim, int* shift, int* copies)
{
    const int e_bytes = (nbins + 1) * (int)sizeof(double), c_bytes = (nbins + 3) * (int)sizeof(uint32_t);
    auto copies_at = [&](int sh) {
        const int room = kHistLdsBytes / (1 << sh) - e_bytes;
        const int c = room / c_bytes;
        return c >= kHistWaves ? kHistWaves : c >= 2 ? 2 : c;
    };
    int sh = 0;
    while (sh < 6 && copies_at(sh + 1) >= 1) ++sh;
    while (sh > 0 && (1 << (sh - 1)) >= ndim) --sh;
    while (sh > 3 && copies_at(sh) < kHistWaves) --sh;
    *shift = sh;
    *copies = copies_at(sh);
}

// hist2d: pairs per group, groups and the LDS one workgroup asks for.  Edges [nsel][B + 1], the tile [kHistTileRows][nsel rounded up to a
// power of two] and two bytes per pair come off the budget first; a pair's counters are B * B * 4 bytes.
void plan2(int nsel, int nbins, int* sel_shift, int* ppg, int* ngroups, int* lds_bytes)
{
    int ss = 0;
    while ((1 << ss) < nsel) ++ss;
    const int npairs = nsel * (nsel - 1) / 2;
    const int fixed = nsel * (nbins + 1) * (int)sizeof(double) + (kHistTileRows << ss);
    const int per_pair = nbins * nbins * (int)sizeof(uint32_t) + 2;
    int p = (kHistLdsBytes - fixed) / per_pair;
    if (p > npairs) p = npairs;
    *sel_shift = ss;
    *ppg = p;
    *ngroups = p > 0 ? (npairs + p - 1) / p : 0;
    *lds_bytes = fixed + p * per_pair;
}

// everything about the request that needs no device: the messages name the argument
kmc_status check_request(int64_t ndim, const int32_t* dims, int32_t ndims, const double* edges, int32_t nbins, bool with_logp, bool pairs,
                         const int64_t* counts1, const int64_t* outside, std::vector<int32_t>* sel)
{
    if (!edges || !counts1 || !outside) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (nbins < 1 || nbins > kHistMaxBins) return fail(KMC_ERR_BAD_ARG, "nbins must lie in 1..256");
    if (pairs && nbins > kHistMaxBins2) return fail(KMC_ERR_BAD_ARG, "nbins must lie in 1..64 when the 2-D histograms are asked for");
    if (ndims < 0 || (ndims > 0 && !dims) || ndims > ndim) return fail(KMC_ERR_BAD_ARG, "ndims must lie in 0..ndim, with dims given when it is not 0");
    sel->clear();
    if (!dims || ndims == 0) {
        for (int64_t d = 0; d < ndim; ++d) sel->push_back((int32_t)d);
    } else {
        for (int32_t i = 0; i < ndims; ++i) {
            if (dims[i] < 0 || dims[i] >= ndim) return fail(KMC_ERR_BAD_ARG, "dimension " + std::to_string(dims[i]) + " outside [0, " + std::to_string(ndim) + ")");
            for (int32_t k = 0; k < i; ++k)
                if (dims[k] == dims[i]) return fail(KMC_ERR_BAD_ARG, "dimension " + std::to_string(dims[i]) + " is selected twice");
            sel->push_back(dims[i]);
        }
    }
    const int64_t nsel = (int64_t)sel->size();
    if (pairs && (nsel < 2 || nsel > kHistMaxDims2)) return fail(KMC_ERR_BAD_ARG, "the 2-D histograms take between 2 and 16 selected dimensions");
    const int64_t ncols = nsel + (with_logp ? 1 : 0);
    for (int64_t c = 0; c < ncols; ++c) {
        const double* e = edges + c * (nbins + 1);
        for (int i = 0; i <= nbins; ++i)
            if (!std::isfinite(e[i]) || (i > 0 && !(e[i] > e[i - 1])))
                return fail(KMC_ERR_BAD_ARG, "the edges of column " + std::to_string(c) + " are not finite and strictly increasing");
    }
    return KMC_OK;
}

// workgroups per group: enough to fill the device, and so many that no workgroup's 32-bit LDS counters can wrap (fewer than 2^23 steps of
// at most 256 elements each) -- the select's rule
int64_t workgroups(int64_t nsteps)
{
    int64_t nwg = nsteps < 512 ? nsteps : 512;
    const int64_t need = (nsteps >> 23) + 1;
    if (nwg < need) nwg = need;
    return nwg < 1 ? 1 : nwg;
}

kmc_status histograms(const ChainSource& src, int64_t first_sample, const uint8_t* mask_host, const int32_t* dims, int32_t ndims, const double* edges,
                      int32_t nbins, int64_t* counts1, int64_t* outside, int64_t* counts2, int64_t* n_out)
{
    const bool with_logp = src.with_logp;                             // the log-densities are the last column of the 1-D output
    ChainView v;
    KMC_TRY(src.describe(&v));
    std::vector<int32_t> sel;
    KMC_TRY(check_request(v.ndim, dims, ndims, edges, nbins, with_logp, counts2 != nullptr, counts1, outside, &sel));
    int64_t N = 0;
    KMC_TRY(selection_size(v, first_sample, mask_host, &N));
    if (n_out) *n_out = N;
    HistBuffers b;
    KMC_TRY(src.open(b, &v));
    const int64_t nsel = (int64_t)sel.size(), ncols = nsel + (with_logp ? 1 : 0), nrows = (v.nsamples - first_sample) * v.nl;
    const int ne = nbins + 1, nc = nbins + 3;
    ScopedStream ss;                              // never the legacy stream (kmc_host.hpp: copy_sync)
    HIP_TRY(ss.create());
    const hipStream_t st = ss.st;
    KMC_TRY(upload_mask(b, mask_host, v.nl, st));
    HIP_TRY(hipMalloc((void**)&b.edges, (size_t)ncols * ne * sizeof(double)));
    HIP_TRY(copy_sync(b.edges, edges, (size_t)ncols * ne * sizeof(double), hipMemcpyHostToDevice, st));

    // ---- 1-D ----
    int sh = 0, copies = 1;
    plan1(nbins, v.ndim, &sh, &copies);
    std::vector<int32_t> slot_of_col((size_t)v.ndim, -1), groups;
    for (int64_t i = 0; i < nsel; ++i) slot_of_col[(size_t)sel[(size_t)i]] = (int32_t)i;
    for (int64_t g = 0; g < ((v.ndim + (1 << sh) - 1) >> sh); ++g) {
        bool any = false;
        for (int64_t c = g << sh; c < v.ndim && c < ((g + 1) << sh); ++c) any = any || slot_of_col[(size_t)c] >= 0;
        if (any) groups.push_back((int32_t)g);
    }
    const int64_t ngroups = (int64_t)groups.size() + (with_logp ? 1 : 0);
    const int64_t rp = kHistThreads >> sh, nwg1 = workgroups((nrows + rp - 1) / rp);
    if (ngroups * nwg1 >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one histogram call");
    HIP_TRY(hipMalloc((void**)&b.slot_of_col, slot_of_col.size() * sizeof(int32_t)));
    HIP_TRY(copy_sync(b.slot_of_col, slot_of_col.data(), slot_of_col.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMalloc((void**)&b.groups, groups.size() * sizeof(int32_t)));
    HIP_TRY(copy_sync(b.groups, groups.data(), groups.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const size_t out1_bytes = (size_t)ncols * nc * sizeof(unsigned long long);
    HIP_TRY(hipMalloc((void**)&b.out1, out1_bytes));
    HIP_TRY(hipMemsetAsync(b.out1, 0, out1_bytes, st));
    Hist1Args a1{};
    a1.chain = v.chain; a1.logp = with_logp ? v.logp : nullptr; a1.mask = b.mask; a1.edges = b.edges; a1.slot_of_col = b.slot_of_col;
    a1.groups = b.groups; a1.out = b.out1; a1.row0 = first_sample * v.nl; a1.nrows = nrows; a1.nl = v.nl; a1.ld = v.ld;
    a1.ndim = (int32_t)v.ndim; a1.is_float = v.is_float ? 1 : 0; a1.nbins = nbins; a1.cg_shift = sh; a1.ngroups_chain = (int32_t)groups.size();
    a1.lp_slot = with_logp ? (int32_t)nsel : -1; a1.nwg = (int32_t)nwg1; a1.copies = copies;
    const int64_t cols_g = v.ndim < (1 << sh) ? v.ndim : (1 << sh);
    const unsigned lds1 = (unsigned)(cols_g * (ne * sizeof(double) + (size_t)copies * nc * sizeof(uint32_t)));
    hipLaunchKernelGGL(hist1d, dim3((unsigned)(ngroups * nwg1)), dim3(kHistThreads), lds1, st, a1);
    HIP_TRY(hipGetLastError());

    // ---- 2-D: every pair (a, b), a < b, in list order ----
    int64_t npairs = 0;
    if (counts2) {
        int sel_shift = 0, ppg = 0, ng2 = 0, lds2 = 0;
        plan2((int)nsel, nbins, &sel_shift, &ppg, &ng2, &lds2);
        if (ppg < 1) return fail(KMC_ERR_UNSUPPORTED, "one pair's counters do not fit the workgroup's LDS");       // (not with nbins <= 64)
        npairs = nsel * (nsel - 1) / 2;
        std::vector<uint8_t> ab;
        for (int64_t i = 0; i < nsel; ++i)
            for (int64_t j = i + 1; j < nsel; ++j) { ab.push_back((uint8_t)i); ab.push_back((uint8_t)j); }
        const int64_t nwg2 = workgroups((nrows + kHistTileRows - 1) / kHistTileRows);
        if (ng2 * nwg2 >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one histogram call");
        HIP_TRY(hipMalloc((void**)&b.dims, sel.size() * sizeof(int32_t)));
        HIP_TRY(copy_sync(b.dims, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMalloc((void**)&b.pair_ab, ab.size()));
        HIP_TRY(copy_sync(b.pair_ab, ab.data(), ab.size(), hipMemcpyHostToDevice, st));
        const size_t out2_bytes = (size_t)npairs * nbins * nbins * sizeof(unsigned long long);
        HIP_TRY(hipMalloc((void**)&b.out2, out2_bytes));
        HIP_TRY(hipMemsetAsync(b.out2, 0, out2_bytes, st));
        Hist2Args a2{};
        a2.chain = v.chain; a2.mask = b.mask; a2.edges = b.edges; a2.dims = b.dims; a2.pair_ab = b.pair_ab; a2.out = b.out2;
        a2.row0 = first_sample * v.nl; a2.nrows = nrows; a2.nl = v.nl; a2.ld = v.ld; a2.is_float = v.is_float ? 1 : 0; a2.nbins = nbins;
        a2.nsel = (int32_t)nsel; a2.sel_shift = sel_shift; a2.npairs = (int32_t)npairs; a2.ppg = ppg; a2.nwg = (int32_t)nwg2;
        hipLaunchKernelGGL(hist2d, dim3((unsigned)(ng2 * nwg2)), dim3(kHistThreads), (unsigned)lds2, st, a2);
        HIP_TRY(hipGetLastError());
    }

    std::vector<unsigned long long> o1((size_t)ncols * nc);
    HIP_TRY(copy_sync(o1.data(), b.out1, out1_bytes, hipMemcpyDeviceToHost, st));
    for (int64_t c = 0; c < ncols; ++c) {
        for (int i = 0; i < nbins; ++i) counts1[c * nbins + i] = (int64_t)o1[(size_t)(c * nc + i)];
        for (int i = 0; i < 3; ++i) outside[c * 3 + i] = (int64_t)o1[(size_t)(c * nc + nbins + i)];
    }
    if (counts2) HIP_TRY(copy_sync(counts2, b.out2, (size_t)npairs * nbins * nbins * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return KMC_OK;
}

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_histograms(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, const int32_t* dims, int32_t ndims,
                                             const double* edges, int32_t nbins, int32_t with_logp, int64_t* counts1, int64_t* outside,
                                             int64_t* counts2, int64_t* n_out)
{
    return histograms(ChainSource(s, with_logp != 0, "kmc_chain_histograms"), first_sample, walker_mask, dims, ndims, edges, nbins, counts1,
                      outside, counts2, n_out);
}

KMC_EXPORT kmc_status kmc_chain_histograms(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                           int64_t first_sample, const uint8_t* walker_mask, const int32_t* dims, int32_t ndims, const double* edges,
                                           int32_t nbins, int device, int64_t* counts1, int64_t* outside, int64_t* counts2, int64_t* n_out)
{
    return histograms(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, dims, ndims, edges, nbins,
                      counts1, outside, counts2, n_out);
}

// How the pairs of `ndims` selected dimensions with `nbins` bins are cut into groups (hist2d reads the selection once per group), and the
// LDS budget that decides it; for tests and benchmarks.  Touches no device.
KMC_EXPORT kmc_status kmc_hist_pair_plan(int32_t ndims, int32_t nbins, int32_t* pairs_per_group, int32_t* ngroups, int32_t* lds_budget)
{
    if (ndims < 2 || ndims > kHistMaxDims2 || nbins < 1 || nbins > kHistMaxBins2) return fail(KMC_ERR_BAD_ARG, "need 2..16 dimensions and 1..64 bins");
    int ss = 0, ppg = 0, ng = 0, lds = 0;
    plan2(ndims, nbins, &ss, &ppg, &ng, &lds);
    if (pairs_per_group) *pairs_per_group = ppg;
    if (ngroups) *ngroups = ng;
    if (lds_budget) *lds_budget = kHistLdsBytes;
    return KMC_OK;
}
