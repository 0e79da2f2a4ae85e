// kmc_cov.hip -- the posterior covariance matrix of a stored chain, summed on the device where the chain lies: the mean of every column
// and the centred cross products of every pair of columns over the selected rows (kmc_sampler_covariance, kmc_chain_covariance), the
// plan of the product kernel (kmc_cov_plan) and the pure host stage that turns a covariance into a correlation matrix
// (kmc_cov_correlation).  include/kissmcmc_hip.h has the definition, DESIGN.md section 4j the plan.  Kernels: kmc_cov_kernels.hpp.
#include <algorithm>
#include <cmath>
#include <vector>

#include "kmc_chain_view.hpp"
#include "kmc_cov_kernels.hpp"

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_cov;

namespace {

constexpr int64_t kCovTargetWaves = 4096;                  // of one launch, over all its strips: 4 per SIMD of 256 compute units

// the cut of ncols columns into tiles, tile pairs and strips: from ncols alone
struct CovPlan {
    int32_t ntiles = 0, nstrips = 0, nslots = 0;
};

CovPlan cov_plan(int64_t ncols)
{
    CovPlan p;
    p.ntiles = (int32_t)((ncols + kCovTile - 1) / kCovTile);
    p.nslots = p.ntiles * (p.ntiles + 1) / 2;
    if (p.ntiles <= 2) {
        p.nstrips = 1;                                       // cov_tri_partials: every pair in one read
    } else {
        for (int32_t ta = 0; ta < p.ntiles; ++ta) p.nstrips += (p.ntiles - ta + kCovStripTiles - 1) / kCovStripTiles;
    }
    return p;
}

// waves of one launch that walk the rows side by side: from the row count and the strip count alone
int64_t cov_waves(int64_t rows, int64_t nstrips)
{
    const int64_t nchunks = (rows + kCovChunkRows - 1) / kCovChunkRows;
    return std::max<int64_t>(1, std::min(nchunks, kCovTargetWaves / nstrips));
}

// the device work of a covariance on stream `st`: the n selected rows (mask_dev, or all) of the view at and after first_sample
kmc_status covariance_on_view(const ChainView& v, bool with_logp, int64_t first_sample, const uint8_t* mask_dev, int64_t n, hipStream_t st,
                              double* mean, double* cov, int64_t* info)
{
    struct Work {
        double* work = nullptr;
        ~Work() { (void)hipFree(work); }
    } b;
    const int64_t C = v.ndim + (with_logp ? 1 : 0);
    const int64_t rows = (v.nsamples - first_sample) * v.nl;
    const CovPlan pl = cov_plan(C);
    const int64_t wm = cov_waves(rows, pl.ntiles), wc = cov_waves(rows, pl.nstrips);
    // the work space of one call, one allocation: the mean, the folded sums and the partial sums
    const size_t mean_bytes = (size_t)pl.ntiles * kCovTile * sizeof(double), out_bytes = (size_t)pl.nslots * kCovTileEntries * sizeof(double);
    const size_t part_bytes = std::max((size_t)pl.ntiles * (size_t)wm * kCovLanes, (size_t)pl.nslots * (size_t)wc * kCovTileEntries) * sizeof(double);
    KMC_TRY(check_device_room(mean_bytes + out_bytes + part_bytes, "the covariance work space"));
    HIP_TRY(hipMalloc((void**)&b.work, mean_bytes + out_bytes + part_bytes));
    double *d_mean = b.work, *d_out = d_mean + (size_t)pl.ntiles * kCovTile, *d_part = d_out + (size_t)pl.nslots * kCovTileEntries;

    CovArgs a{};
    a.chain = v.chain; a.logp = with_logp ? v.logp : nullptr; a.mask = mask_dev; a.mean = d_mean; a.part = d_part; a.out = d_out;
    a.n = (double)n; a.row0 = first_sample * v.nl; a.rows = rows; a.nl = v.nl; a.ld = v.ld;
    a.ndim = (int32_t)v.ndim; a.ncols = (int32_t)C; a.is_float = v.is_float ? 1 : 0; a.ntiles = pl.ntiles;

    // stage 1: the column sums and the mean
    a.nwaves = (int32_t)wm;
    hipLaunchKernelGGL(cov_mean_partials, dim3((unsigned)((wm + kCovWaves - 1) / kCovWaves), (unsigned)pl.ntiles), dim3(kCovThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cov_mean_fold, dim3((unsigned)pl.ntiles), dim3(kCovThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    // stage 2: the cross products, centred on that mean
    a.nwaves = (int32_t)wc;
    const dim3 grid((unsigned)((wc + kCovWaves - 1) / kCovWaves), (unsigned)pl.nstrips);
    if (pl.ntiles == 1) hipLaunchKernelGGL(cov_tri_partials<1>, grid, dim3(kCovThreads), 0, st, a);
    else if (pl.ntiles == 2) hipLaunchKernelGGL(cov_tri_partials<2>, grid, dim3(kCovThreads), 0, st, a);
    else hipLaunchKernelGGL(cov_strip_partials, grid, dim3(kCovThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cov_fold, dim3((unsigned)(pl.nslots * (kCovTileEntries / kCovTile))), dim3(kCovThreads), 0, st, a);
    HIP_TRY(hipGetLastError());

    std::vector<double> mu((size_t)pl.ntiles * kCovTile), sums((size_t)pl.nslots * kCovTileEntries);
    HIP_TRY(copy_sync(mu.data(), d_mean, mean_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(copy_sync(sums.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st));
    std::copy(mu.begin(), mu.begin() + C, mean);
    // the upper triangle from the accumulator map -- lane l, register r: row (l >> 4) + 4 r of the A tile, column l & 15 of the B tile --
    // divided once, and mirrored
    const double nm1 = (double)(n - 1);
    int64_t slot = 0;
    for (int64_t ta = 0; ta < pl.ntiles; ++ta) {
        for (int64_t tb = ta; tb < pl.ntiles; ++tb, ++slot) {
            for (int r = 0; r < 4; ++r) {
                for (int l = 0; l < kCovLanes; ++l) {
                    const int64_t ca = ta * kCovTile + (l >> 4) + 4 * r, cb = tb * kCovTile + (l & 15);
                    if (ca > cb || cb >= C) continue;
                    const double c = sums[(size_t)(slot * kCovTileEntries + r * kCovLanes + l)] / nm1;
                    cov[ca * C + cb] = c;
                    cov[cb * C + ca] = c;
                }
            }
        }
    }
    if (info) {
        // bytes of the chain the kernels loaded: selected rows only; the mean stage reads every column once, the product stage the
        // columns of a strip's tiles once per strip
        const int64_t elem = v.is_float ? 4 : 8;
        auto tile_bytes = [&](int64_t t) {
            int64_t bytes = 0;
            for (int64_t c = t * kCovTile; c < std::min<int64_t>(C, (t + 1) * kCovTile); ++c) bytes += c < v.ndim ? elem : 8;
            return bytes;
        };
        int64_t row_bytes = 0, strip_bytes = 0;
        for (int64_t t = 0; t < pl.ntiles; ++t) row_bytes += tile_bytes(t);
        if (pl.ntiles <= 2) {
            strip_bytes = row_bytes;
        } else {
            for (int64_t ta = 0; ta < pl.ntiles; ++ta) {
                for (int64_t tb0 = ta; tb0 < pl.ntiles; tb0 += kCovStripTiles) {
                    strip_bytes += tile_bytes(ta);
                    for (int64_t tb = tb0; tb < std::min<int64_t>(pl.ntiles, tb0 + kCovStripTiles); ++tb) strip_bytes += tb == ta ? 0 : tile_bytes(tb);
                }
            }
        }
        info[0] = rows; info[1] = wc; info[2] = pl.nstrips; info[3] = n * (row_bytes + strip_bytes);
    }
    return KMC_OK;
}

kmc_status covariance(const ChainSource& src, int64_t first_sample, const uint8_t* walker_mask, double* mean, double* cov, int64_t* n_out,
                      int64_t* info)
{
    ChainView v;
    KMC_TRY(src.describe(&v));
    int64_t n = 0;
    KMC_TRY(selection_size(v, first_sample, walker_mask, &n));
    const int64_t C = v.ndim + (src.with_logp ? 1 : 0);
    if (C > kCovMaxCols)
        return fail(KMC_ERR_UNSUPPORTED, "a covariance matrix of " + std::to_string(C) + " columns: the limit is " + std::to_string(kCovMaxCols));
    if (n < 2) return fail(KMC_ERR_BAD_ARG, "a covariance needs at least 2 selected rows (n = " + std::to_string(n) + ")");
    if (!mean || !cov) return fail(KMC_ERR_BAD_ARG, "null argument");
    const int64_t rows = (v.nsamples - first_sample) * v.nl;
    if (rows >= ((int64_t)1 << 40)) return fail(KMC_ERR_UNSUPPORTED, "chain too large for one covariance call");
    if (n_out) *n_out = n;

    ChainUpload b;
    KMC_TRY(src.open(b, &v));
    ScopedStream ss;                              // never the legacy stream (kmc_host.hpp: copy_sync)
    HIP_TRY(ss.create());
    KMC_TRY(upload_mask(b, walker_mask, v.nl, ss.st));
    return covariance_on_view(v, src.with_logp, first_sample, b.mask, n, ss.st, mean, cov, info);
}

}  // namespace

// The covariance of dense device rows [nrows][ndim] (one sample of nrows walkers): kmc_chain_covariance's kernels, plan and host
// stage on the caller's stream, no copy of the rows (kmc_metropolis_api.hip: the tuning boundaries of kmc_metropolis_run).
kmc_status kmc_chain_view::covariance_of_rows(const double* rows_dev, int64_t nrows, int64_t ndim, hipStream_t st, double* mean, double* cov)
{
    ChainView v;
    v.chain = rows_dev; v.ld = ndim; v.ndim = ndim; v.nsamples = 1; v.nl = nrows;
    if (ndim > kCovMaxCols || nrows < 2) return fail(KMC_ERR_BAD_ARG, "covariance_of_rows: at most " + std::to_string(kCovMaxCols) + " columns, at least 2 rows");
    return covariance_on_view(v, false, 0, nullptr, nrows, st, mean, cov, nullptr);
}

KMC_EXPORT kmc_status kmc_sampler_covariance(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t with_logp, double* mean,
                                             double* cov, int64_t* n_out, int64_t* info)
{
    return covariance(ChainSource(s, with_logp != 0, "kmc_chain_covariance"), first_sample, walker_mask, mean, cov, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_covariance(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                                           int64_t first_sample, const uint8_t* walker_mask, int device, double* mean, double* cov,
                                           int64_t* n_out, int64_t* info)
{
    return covariance(ChainSource(chain_host, logp_host, nsamples, nwalkers, ndim, device), first_sample, walker_mask, mean, cov, n_out, info);
}

// The cut of the product kernel; for tests and benchmarks.  Touches no device.
KMC_EXPORT kmc_status kmc_cov_plan(int64_t ncols, int32_t* tile_cols, int32_t* strip_tiles, int32_t* nstrips, int32_t* rows_per_wave_block)
{
    if (ncols < 1) return fail(KMC_ERR_BAD_ARG, "need ncols >= 1");
    if (ncols > kCovMaxCols)
        return fail(KMC_ERR_UNSUPPORTED, "a covariance matrix of " + std::to_string(ncols) + " columns: the limit is " + std::to_string(kCovMaxCols));
    if (tile_cols) *tile_cols = kCovTile;
    if (strip_tiles) *strip_tiles = kCovStripTiles;
    if (nstrips) *nstrips = cov_plan(ncols).nstrips;
    if (rows_per_wave_block) *rows_per_wave_block = kCovChunkRows;
    return KMC_OK;
}

// The host stage: std[a] = sqrt(cov[a][a]); corr[a][b] = cov[a][b] / (std[a] * std[b]); the diagonal is 1.0 where the variance is finite
// and positive.  No device; no fused multiply-add (the library is built with -ffp-contract=off).
KMC_EXPORT kmc_status kmc_cov_correlation(int64_t ncols, const double* cov, double* corr, double* std_out)
{
    if (ncols < 1) return fail(KMC_ERR_BAD_ARG, "need ncols >= 1");
    if (!cov || !corr) return fail(KMC_ERR_BAD_ARG, "null argument");
    std::vector<double> sd((size_t)ncols);
    for (int64_t a = 0; a < ncols; ++a) sd[(size_t)a] = std::sqrt(cov[a * ncols + a]);
    for (int64_t a = 0; a < ncols; ++a) {
        for (int64_t b = 0; b < ncols; ++b) {
            const double den = sd[(size_t)a] * sd[(size_t)b];
            corr[a * ncols + b] = cov[a * ncols + b] / den;
        }
        const double var = cov[a * ncols + a];
        if (var > 0.0 && std::isfinite(var)) corr[a * ncols + a] = 1.0;
    }
    if (std_out) std::copy(sd.begin(), sd.end(), std_out);
    return KMC_OK;
}
