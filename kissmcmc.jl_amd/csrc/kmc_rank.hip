// kmc_rank.hip -- rank-normalised R^ with bulk and tail effective sample sizes (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021)
// of a stored chain, ranked on the device: every pooled draw of a column gets its exact average rank among all draws of the column by
// a segmented radix sort of the column's keys and two binary searches, the rank becomes a normal score, and the statistics are those of
// kmc_convergence.hip applied to the transformed columns (include/kissmcmc_hip.h).  The sort's host side is the
// sorted-columns service of kmc_rank_host.hpp, defined here; the two entry points are their checks between the steps of a ConvSession
// (kmc_convergence_host.hpp) and run both halves -- ranking, then the statistics of the scratch chain -- on its one stream.
// Kernels: kmc_rank_kernels.hpp.
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>

#include "kmc_rank_host.hpp"
#include "kmc_rank_kernels.hpp"

using namespace kmc_rank;
using namespace kmc_rank_host;                               // (and through it kmc_host, kmc_chain_view, kmc_conv_host)

namespace {

constexpr int kTransforms = 4;                               // bulk z, folded z, I05, I95: the column sets of the scratch chain

int64_t tiles_of(int64_t S) { return (S + kRankTileKeys - 1) / kRankTileKeys; }

// The work space: two key buffers (16 B), the digit counts, and 8 B per transformed column (or 16 B for rank2 and z), per pooled draw;
// checked against the free memory, then allocated.
kmc_status reserve(SortedColumns& sc, const ConvShape& sh, int transformed, bool outputs, double extra)
{
    const int64_t ncols = sc.ncols, S = sc.S;
    const double keys = 16.0 * (double)ncols * (double)S, counts = 4.0 * kRankBins * (double)tiles_of(S) * (double)ncols;
    const double scratch = 8.0 * (double)transformed * (double)ncols * (double)sh.n * (double)sh.nw, outs = outputs ? 16.0 * (double)ncols * (double)S : 0.0;
    const double need = keys + counts + scratch + outs + extra + 64.0 * 1048576.0;
    size_t free_b = 0;
    bool fits = false;
    KMC_TRY(device_fits(need, &fits, &free_b));
    if (!fits)
        return fail(KMC_ERR_UNSUPPORTED, "ranking " + std::to_string(ncols) + " columns of " + std::to_string(S) + " pooled draws needs " +
                                             std::to_string((int64_t)(need / 1048576.0)) + " MiB of device memory (keys " + std::to_string((int64_t)(keys / 1048576.0)) +
                                             " MiB, transformed columns " + std::to_string((int64_t)((scratch + outs) / 1048576.0)) + " MiB), " +
                                             std::to_string(free_b >> 20) + " MiB are free; ranking in column groups is not built");
    const size_t kb = (size_t)ncols * (size_t)S * sizeof(uint64_t);
    HIP_TRY(hipMalloc((void**)&sc.key_a, kb));
    HIP_TRY(hipMalloc((void**)&sc.key_b, kb));
    HIP_TRY(hipMalloc((void**)&sc.counts, (size_t)ncols * (size_t)tiles_of(S) * kRankBins * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&sc.nan_dev, (size_t)ncols * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void**)&sc.centre, (size_t)ncols * 3 * sizeof(double)));
    if (outputs) {
        HIP_TRY(hipMalloc((void**)&sc.out_rank2, kb));
        HIP_TRY(hipMalloc((void**)&sc.out_z, kb));
    }
    return KMC_OK;
}

// keys of the (folded) selection into key_a; sc.nan[c]: the NaNs among them
kmc_status gather(SortedColumns& sc, const ConvSession& ses, bool folded)
{
    const ChainView& v = ses.v;
    const ConvShape& sh = ses.sh;
    HIP_TRY(hipMemsetAsync(sc.nan_dev, 0, (size_t)ses.ncols * sizeof(unsigned long long), ses.st()));
    for (const ConvSource& src : sources(v, ses.with_logp)) {
        GatherArgs a{};
        a.src = src.src; a.rank = ses.b.rank; a.centre = folded ? sc.centre : nullptr; a.keys = sc.key_a; a.nan_count = sc.nan_dev;
        a.first = sh.first; a.half_off = sh.half_off; a.h = sh.h; a.nl = v.nl; a.ld = src.ld; a.np = v.nl * src.ld; a.nw = sh.nw; a.S = sc.S;
        a.ntile_p = (a.np + kRankGatherTile - 1) / kRankGatherTile;
        a.ntile_i = (sh.h + kRankGatherTile - 1) / kRankGatherTile;
        a.ndim = src.ndim; a.is_float = src.is_float ? 1 : 0; a.col0 = src.col0;
        const int64_t grid = a.ntile_p * a.ntile_i * sh.nhalf;
        if (grid >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one ranking call");
        hipLaunchKernelGGL(rank_gather, dim3((unsigned)grid), dim3(kRankThreads), 0, ses.st(), a);
        HIP_TRY(hipGetLastError());
    }
    std::vector<unsigned long long> n((size_t)ses.ncols);
    HIP_TRY(copy_sync(n.data(), sc.nan_dev, n.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ses.st()));
    sc.nan.assign(n.begin(), n.end());
    return KMC_OK;
}

// key_a sorted, every column on its own: 8 passes between key_a and key_b, an even number, so the result is in key_a again
kmc_status sort_columns(SortedColumns& sc)
{
    const hipStream_t st = sc.st;
    SortArgs a{};
    a.S = sc.S; a.ntiles = tiles_of(sc.S); a.counts = sc.counts;
    uint64_t *in = sc.key_a, *out = sc.key_b;
    for (int pass = 0; pass < kRankPasses; ++pass) {
        a.in = in; a.out = out; a.shift = pass * kRankDigitBits;
        const dim3 grid((unsigned)a.ntiles, (unsigned)sc.ncols);
        hipLaunchKernelGGL(rank_sort_hist, grid, dim3(kRankThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(rank_sort_scan, dim3((unsigned)sc.ncols), dim3(kRankThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(rank_sort_scatter, grid, dim3(kRankThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        std::swap(in, out);
    }
    return KMC_OK;
}

}  // namespace

// ---- the sorted columns as a service (kmc_rank_host.hpp) ----
namespace kmc_rank_host {

// the sizes one call may have, from the shape alone
kmc_status rank_limits(const ConvShape& sh, int64_t ncols)
{
    const int64_t S = sh.m * sh.h;
    if (S >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "2^31 pooled draws or more per column (" + std::to_string(S) + ")");
    if (ncols > 65535) return fail(KMC_ERR_UNSUPPORTED, "more than 65535 columns");
    return KMC_OK;
}

double unkey(uint64_t key)
{
    const uint64_t bits = chain_unkey(key);
    double x;
    std::memcpy(&x, &bits, sizeof x);
    return x;
}

kmc_status SortedColumns::sort(const ConvSession& ses, int transformed, bool outputs, double extra, const hipEvent_t* marks)
{
    ncols = ses.ncols; S = ses.sh.m * ses.sh.h; st = ses.st();
    KMC_TRY(reserve(*this, ses.sh, transformed, outputs, extra));
    if (marks) HIP_TRY(hipEventRecord(marks[0], st));
    KMC_TRY(gather(*this, ses, false));
    if (marks) HIP_TRY(hipEventRecord(marks[1], st));
    KMC_TRY(sort_columns(*this));
    if (marks) HIP_TRY(hipEventRecord(marks[2], st));
    return KMC_OK;
}

kmc_status SortedColumns::sort_folded(const ConvSession& ses)
{
    KMC_TRY(gather(*this, ses, true));
    return sort_columns(*this);
}

kmc_status SortedColumns::pick_at(const std::vector<int64_t>& pos, std::vector<uint64_t>* out)
{
    for (int64_t at : pos)
        if (at < 0 || at >= ncols * S) return fail(KMC_ERR_HIP, "internal: an order statistic outside the sorted columns");
    if (pos.size() > npos) {
        (void)hipFree(pos_dev); (void)hipFree(picked);
        pos_dev = nullptr; picked = nullptr; npos = 0;
        HIP_TRY(hipMalloc((void**)&pos_dev, pos.size() * sizeof(int64_t)));
        HIP_TRY(hipMalloc((void**)&picked, pos.size() * sizeof(uint64_t)));
        npos = pos.size();
    }
    HIP_TRY(copy_sync(pos_dev, pos.data(), pos.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    SelectArgs a{};
    a.sorted = key_a; a.pos = pos_dev; a.out = picked; a.n = (int64_t)pos.size();
    hipLaunchKernelGGL(rank_select, dim3((unsigned)((a.n + kRankThreads - 1) / kRankThreads)), dim3(kRankThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    out->resize(pos.size());
    HIP_TRY(copy_sync(out->data(), picked, pos.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return KMC_OK;
}

kmc_status SortedColumns::quantiles(const double* q, int nq, double* out)
{
    std::vector<int64_t> pos((size_t)(2 * nq * ncols));
    for (int k = 0; k < nq; ++k) {
        const QuantileAt at(q[k], S);
        for (int64_t c = 0; c < ncols; ++c) {
            pos[(size_t)(2 * (k * ncols + c))] = c * S + at.lo;
            pos[(size_t)(2 * (k * ncols + c) + 1)] = c * S + at.hi;
        }
    }
    std::vector<uint64_t> got;
    KMC_TRY(pick_at(pos, &got));
    for (int k = 0; k < nq; ++k) {
        const QuantileAt at(q[k], S);
        for (int64_t c = 0; c < ncols; ++c) {
            const size_t e = (size_t)(k * ncols + c);
            out[e] = nan[(size_t)c] ? std::numeric_limits<double>::quiet_NaN() : at.between(unkey(got[2 * e]), unkey(got[2 * e + 1]));
        }
    }
    return KMC_OK;
}

}  // namespace kmc_rank_host

namespace {

// The quantiles 0.5, 0.05, 0.95 of the sorted columns: centre[3][ncols] on the host and in sc.centre, for the fold and the indicators;
// NaN for a column that holds one.
kmc_status centres(SortedColumns& sc, std::vector<double>* centre)
{
    static const double q[3] = {0.5, 0.05, 0.95};
    centre->resize((size_t)(3 * sc.ncols));
    KMC_TRY(sc.quantiles(q, 3, centre->data()));
    HIP_TRY(copy_sync(sc.centre, centre->data(), centre->size() * sizeof(double), hipMemcpyHostToDevice, sc.st));
    return KMC_OK;
}

kmc_status score(SortedColumns& sc, const ConvSession& ses, bool folded, bool indicators, double* scratch, int64_t scratch_cols)
{
    const ChainView& v = ses.v;
    const ConvShape& sh = ses.sh;
    for (const ConvSource& src : sources(v, ses.with_logp)) {
        ScoreArgs a{};
        a.src = src.src; a.rank = ses.b.rank; a.sorted = sc.key_a; a.centre = sc.centre; a.scratch = scratch; a.out_rank2 = sc.out_rank2; a.out_z = sc.out_z;
        a.first = sh.first; a.half_off = sh.half_off; a.h = sh.h; a.nl = v.nl; a.ld = src.ld; a.np = v.nl * src.ld; a.nw = sh.nw; a.S = sh.m * sh.h;
        a.lds_cols = scratch_cols; a.nelem = (int64_t)sh.nhalf * sh.h * a.np;
        a.ndim = src.ndim; a.is_float = src.is_float ? 1 : 0; a.col0 = src.col0; a.ncols = (int32_t)ses.ncols; a.folded = folded ? 1 : 0;
        a.indicators = indicators ? 1 : 0; a.zcol0 = folded ? (int32_t)ses.ncols : 0;
        const int64_t grid = (a.nelem + kRankThreads - 1) / kRankThreads;
        if (grid >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one ranking call");
        hipLaunchKernelGGL(rank_score, dim3((unsigned)grid), dim3(kRankThreads), 0, ses.st(), a);
        HIP_TRY(hipGetLastError());
    }
    return KMC_OK;
}

// ---- the device stage alone: rank2 and z of the (folded) columns ----
kmc_status rank_scores_stage(const ConvSession& ses, bool folded, int64_t* rank2, double* z, double* centre_out, int64_t* nan_count)
{
    SortedColumns sc;                                         // (dies before the session: it drains the session's live stream itself)
    const int64_t ncols = ses.ncols, S = ses.sh.m * ses.sh.h;
    KMC_TRY(sc.sort(ses, 0, true));
    if (folded) {
        std::vector<double> centre;
        KMC_TRY(centres(sc, &centre));
        KMC_TRY(sc.sort_folded(ses));
        if (centre_out) std::copy(centre.begin(), centre.begin() + ncols, centre_out);
    }
    KMC_TRY(score(sc, ses, folded, false, nullptr, 0));
    const size_t bytes = (size_t)ncols * (size_t)S * 8;
    if (rank2) HIP_TRY(copy_sync(rank2, sc.out_rank2, bytes, hipMemcpyDeviceToHost, ses.st()));
    if (z) HIP_TRY(copy_sync(z, sc.out_z, bytes, hipMemcpyDeviceToHost, ses.st()));
    HIP_TRY(hipStreamSynchronize(ses.st()));
    for (int64_t c = 0; c < ncols; ++c) {                     // a column that holds a NaN has no ranks
        if (nan_count) nan_count[c] = sc.nan[(size_t)c];
        if (!sc.nan[(size_t)c]) continue;
        if (rank2) std::fill(rank2 + c * S, rank2 + (c + 1) * S, (int64_t)0);
        if (z) std::fill(z + c * S, z + (c + 1) * S, std::numeric_limits<double>::quiet_NaN());
    }
    return KMC_OK;
}

// ---- the whole thing ----
struct RankOut {
    double *rhat, *rhat_bulk, *rhat_folded, *ess_bulk, *ess_tail, *ess_q05, *ess_q95, *median, *q05, *q95;
    int64_t* T;                        // [4][ncols]
    int32_t* flags;
    bool complete() const { return rhat && rhat_bulk && rhat_folded && ess_bulk && ess_tail && ess_q05 && ess_q95 && median && q05 && q95 && T && flags; }
};

// sb: owns the scratch chain (as its uploaded chain) and the work space of the statistics
kmc_status rank_convergence_stage(const ConvSession& ses, ConvBuffers& sb, const RankOut& o, int64_t* info)
{
    const ConvShape& sh = ses.sh;
    const int64_t ncols = ses.ncols, S = sh.m * sh.h, tcols = kTransforms * ncols;
    const double nan_v = std::numeric_limits<double>::quiet_NaN();
    const hipStream_t st = ses.st();
    std::vector<int64_t> nan_bulk, nan_fold;
    std::vector<double> centre;
    {
        SortedColumns sc;
        KMC_TRY(sc.sort(ses, kTransforms, false));
        nan_bulk = sc.nan;
        const size_t srow = (size_t)sh.nw * (size_t)tcols;
        HIP_TRY(hipMalloc((void**)&sb.chain, (size_t)sh.n * srow * sizeof(double)));
        if (sh.nhalf == 2 && sh.n != 2 * sh.h)               // the middle sample of an odd n belongs to no chain: a row of zeros nobody reads
            HIP_TRY(hipMemsetAsync(sb.chain + (size_t)sh.h * srow, 0, srow * sizeof(double), st));
        KMC_TRY(centres(sc, &centre));
        KMC_TRY(score(sc, ses, false, true, sb.chain, tcols));
        KMC_TRY(sc.sort_folded(ses));
        nan_fold = sc.nan;
        KMC_TRY(score(sc, ses, true, false, sb.chain, tcols));
        HIP_TRY(hipStreamSynchronize(st));
    }                                                         // (the keys are freed before the statistics take their work space)
    ChainView sv;
    sv.chain = sb.chain; sv.is_float = false; sv.ld = tcols; sv.ndim = tcols; sv.logp = nullptr; sv.nsamples = sh.n; sv.nl = sh.nw;
    ConvShape ssh = sh;
    ssh.first = 0;
    std::vector<double> mean((size_t)tcols), W((size_t)tcols), B((size_t)tcols), vp((size_t)tcols), rhat((size_t)tcols), ess((size_t)tcols), mcse((size_t)tcols);
    std::vector<int64_t> T((size_t)tcols);
    std::vector<int32_t> flags((size_t)tcols);
    const StatsOut so{mean.data(), W.data(), B.data(), vp.data(), rhat.data(), ess.data(), mcse.data(), T.data(), flags.data()};
    int64_t cinfo[4] = {0, 0, 0, 0};
    KMC_TRY(upload_rank(sb, nullptr, sv.nl, st));             // the scratch chain holds the selected walkers alone: one rank map of its own
    KMC_TRY(convergence_on_stream(sb, sv, ssh, false, ses.max_lag, so, cinfo, st));
    for (int64_t c = 0; c < ncols; ++c) {
        const size_t bk = (size_t)c, fd = (size_t)(ncols + c), i5 = (size_t)(2 * ncols + c), i95 = (size_t)(3 * ncols + c);
        int32_t f = flags[bk] | flags[fd] | flags[i5] | flags[i95];
        for (int t = 0; t < kTransforms; ++t) o.T[t * ncols + c] = T[(size_t)(t * ncols + c)];
        o.rhat_bulk[c] = rhat[bk]; o.rhat_folded[c] = rhat[fd];
        o.ess_bulk[c] = ess[bk]; o.ess_q05[c] = ess[i5]; o.ess_q95[c] = ess[i95];
        o.median[c] = centre[(size_t)c]; o.q05[c] = centre[(size_t)(ncols + c)]; o.q95[c] = centre[(size_t)(2 * ncols + c)];
        if (nan_bulk[(size_t)c]) {                            // a NaN among the draws: no ranks, nothing to report
            o.rhat_bulk[c] = o.rhat_folded[c] = o.ess_bulk[c] = o.ess_q05[c] = o.ess_q95[c] = nan_v;
            for (int t = 0; t < kTransforms; ++t) o.T[t * ncols + c] = 0;
            f = KMC_CONV_HAS_NAN;
        } else if (nan_fold[(size_t)c]) {                     // inf - inf in the fold: a NaN of the folded column only
            o.rhat_folded[c] = nan_v;
            o.T[ncols + c] = 0;
            f = flags[bk] | flags[i5] | flags[i95] | KMC_CONV_HAS_NAN;
        }
        const double rb_ = o.rhat_bulk[c], rf = o.rhat_folded[c], e5 = o.ess_q05[c], e95 = o.ess_q95[c];
        o.rhat[c] = (rb_ != rb_ || rf != rf) ? nan_v : std::max(rb_, rf);
        o.ess_tail[c] = (e5 != e5 || e95 != e95) ? nan_v : std::min(e5, e95);
        o.flags[c] = f;
    }
    if (info) {
        info[0] = cinfo[0];
        info[1] = 2 * (int64_t)kRankPasses * 24 * ncols * S;                                          // two sorts: a pass reads the keys twice and writes them once
        info[2] = cinfo[2]; info[3] = cinfo[3];
    }
    return KMC_OK;
}

kmc_status rank_scores(const ChainSource& src, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t folded, int64_t* rank2, double* z,
                       double* centre, int64_t* nan_count, int64_t* m_out, int64_t* h_out)
{
    ConvSession S(src);
    KMC_TRY(S.describe());
    KMC_TRY(S.chains(first_sample, walker_mask, split != 0));
    KMC_TRY(rank_limits(S.sh, S.ncols));
    KMC_TRY(S.open(m_out, h_out));
    return rank_scores_stage(S, folded != 0, rank2, z, centre, nan_count);
}

kmc_status rank_convergence(const ChainSource& src, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag, const RankOut& o,
                            int64_t* m_out, int64_t* h_out, int64_t* info)
{
    ConvBuffers scratch;                                      // (before the session: the stream is drained before it goes)
    ConvSession S(src);
    KMC_TRY(S.describe());
    KMC_TRY(S.chains(first_sample, walker_mask, split != 0));
    KMC_TRY(S.max_lag_from(max_lag));
    KMC_TRY(rank_limits(S.sh, S.ncols));
    if (!o.complete()) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(S.open(m_out, h_out));
    return rank_convergence_stage(S, scratch, o, info);
}

}  // namespace

// The shape of the sort; for tests and benchmarks.  Touches no device.
KMC_EXPORT kmc_status kmc_rank_plan(int32_t* tile_keys, int32_t* digit_bits, int32_t* passes, int32_t* lds_bytes)
{
    if (tile_keys) *tile_keys = kRankTileKeys;
    if (digit_bits) *digit_bits = kRankDigitBits;
    if (passes) *passes = kRankPasses;
    if (lds_bytes) *lds_bytes = kRankLdsBytes;
    return KMC_OK;
}

// The host form of the score.  Touches no device.
KMC_EXPORT kmc_status kmc_rank_normal_scores(const int64_t* rank2, int64_t n, int64_t S, double* z)
{
    if (n < 0 || (n > 0 && (!rank2 || !z))) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (S < 1 || S >= ((int64_t)1 << 52)) return fail(KMC_ERR_BAD_ARG, "need 1 <= S < 2^52");
    for (int64_t i = 0; i < n; ++i)
        if (rank2[i] < 2 || rank2[i] > 2 * S) return fail(KMC_ERR_BAD_ARG, "rank2 must lie in [2, 2 S] (element " + std::to_string(i) + ")");
    for (int64_t i = 0; i < n; ++i) z[i] = rank_score_of(rank2[i], S);
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_rank_scores(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                              int32_t folded, int64_t* rank2, double* z, double* centre, int64_t* nan_count, int64_t* m_out,
                                              int64_t* h_out)
{
    return rank_scores(ChainSource(s, with_logp != 0, "kmc_chain_rank_scores"), first_sample, walker_mask, split, folded, rank2, z, centre,
                       nan_count, m_out, h_out);
}

KMC_EXPORT kmc_status kmc_chain_rank_scores(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                            int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t folded, int device,
                                            int64_t* rank2, double* z, double* centre, int64_t* nan_count, int64_t* m_out, int64_t* h_out)
{
    return rank_scores(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, split, folded, rank2, z,
                       centre, nan_count, m_out, h_out);
}

KMC_EXPORT kmc_status kmc_sampler_rank_convergence(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                                   int64_t max_lag, double* rhat, double* rhat_bulk, double* rhat_folded, double* ess_bulk,
                                                   double* ess_tail, double* ess_q05, double* ess_q95, double* median, double* q05, double* q95,
                                                   int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info)
{
    return rank_convergence(ChainSource(s, with_logp != 0, "kmc_chain_rank_convergence"), first_sample, walker_mask, split, max_lag,
                            {rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_q05, ess_q95, median, q05, q95, T, flags}, m_out, h_out, info);
}

KMC_EXPORT kmc_status kmc_chain_rank_convergence(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                                 int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag, int device,
                                                 double* rhat, double* rhat_bulk, double* rhat_folded, double* ess_bulk, double* ess_tail,
                                                 double* ess_q05, double* ess_q95, double* median, double* q05, double* q95, int64_t* T,
                                                 int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info)
{
    return rank_convergence(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, split, max_lag,
                            {rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_q05, ess_q95, median, q05, q95, T, flags}, m_out, h_out, info);
}
