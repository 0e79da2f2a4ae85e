// kmc_rank_kernels.hpp -- device kernels of the rank-normalised convergence diagnostics (kmc_rank.hip; include/kissmcmc_hip.h; DESIGN.md
// section 4h): the exact rank of every pooled draw among all draws of its column, and from it the normal score.  Internal.
//
// Four steps, every column on its own:
//   rank_gather       reads the selection along the row [sample][walker][ld] (a wave reads 64 consecutive elements), widens floats,
//                     canonicalises zeros (x + 0.0), optionally folds (|x - centre|), makes the key of the order statistics and
//                     writes the keys column-contiguous, keys[column][chain j][sample i], through a 64 x 64 tile transposed in LDS.
//                     NaNs are counted per column with integer atomics.
//   rank_sort_*       a segmented least-significant-digit radix sort of the 64-bit keys, no payload: 8 passes of 8 bits between two
//                     [ncols][S] buffers.  A pass is three kernels: the digit counts of every tile of kRankTileKeys keys (32-bit LDS
//                     atomics, written to the tile's own slot), an exclusive scan over (digit, tile) per column, and a STABLE scatter.
//                     The sorted column is unique, so nothing depends on the geometry or on arrival order; no atomics in the scatter.
//   rank_select       order statistics out of the sorted keys at a list of positions (the quantiles' neighbours, the ends of a rank
//                     interval).
//   rank_score        for every draw in chain order: lower and upper bound in its sorted column by binary search (one shared path until
//                     an equal key parts them), rank2 = #{y < x} + #{y <= x} + 1, the normal score z and, on request, the indicators
//                     x <= q05, x <= q95; written into a scratch chain [sample][selected walker][column] of doubles, which the kernels of
//                     kmc_convergence_kernels.hpp then read like any chain.
//
// No floating-point atomics anywhere.  The score is formed as written (the library is built with -ffp-contract=off): DESIGN.md section 2.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "kmc_chain_kernels.hpp"

namespace kmc_rank {

using namespace kmc_chain;

constexpr int kRankThreads = 256;
constexpr int kRankLanes = 64;
constexpr int kRankWaves = kRankThreads / kRankLanes;
constexpr int kRankDigitBits = 8;
constexpr int kRankBins = 1 << kRankDigitBits;
constexpr int kRankPasses = 64 / kRankDigitBits;
constexpr int kRankKeysPerThread = 16;
constexpr int kRankTileKeys = kRankThreads * kRankKeysPerThread;                 // 4096 keys: one workgroup's tile of a pass
constexpr int kRankWaveKeys = kRankTileKeys / kRankWaves;                        // a wave's contiguous quarter of the tile
constexpr int kRankGatherTile = 64;                                              // positions x samples of the transposed tile
// the scatter's LDS: the tile of keys in digit order, the per-wave digit counters, the digit starts and the global bases
constexpr int kRankLdsBytes = kRankTileKeys * 8 + kRankWaves * kRankBins * 4 + 2 * kRankBins * 4;      // 38,912 B
static_assert(kRankLdsBytes <= 64 * 1024, "a workgroup stays under the default LDS limit");
static_assert(kRankBins == kRankThreads, "one thread per digit in the scans");
static_assert(kRankGatherTile * (kRankGatherTile + 1) * 8 <= 64 * 1024, "the transposed tile fits");

// ---- the normal score ----
// Wichura's AS 241 (PPND16) in exactly the operation order of CPython's statistics._normal_dist_inv_cdf with mu = 0, sigma = 1: every
// product and sum rounded on its own, Horner evaluation as written there.  The central branch uses +, -, *, / only and gives the same
// bits on host and device; the tail branches go through sqrt(-log(r)) and differ only as far as the two logarithms do.
__host__ __device__ inline double rank_ppnd16(double p)
{
    const double q = p - 0.5;
    double num, den;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                   1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                   5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
                   3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                   6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r + 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                   2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                   1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
    }
    double x = num / den;
    if (q < 0.0) x = -x;
    return x;
}

// z of rank2 among S draws: r = rank2 / 2 and r - 0.375 are exact (multiples of 1/8 below 2^33), S + 0.25 is exact, one division.
__host__ __device__ inline double rank_score_of(int64_t rank2, int64_t S)
{
    const double p = ((double)rank2 * 0.5 - 0.375) / ((double)S + 0.25);
    return rank_ppnd16(p);
}

// the value a draw is ranked by: the stored element widened (exact), folded about the column's centre when asked, zeros canonicalised
// (-0.0 + 0.0 = +0.0, so that the two zeros share a key)
__device__ inline double rank_value(const void* src, int is_float, int64_t at, const double* centre, int32_t col)
{
    double x = chain_load(src, is_float, at);
    if (centre) x = fabs(x - centre[col]);
    return x + 0.0;
}

// the key of the order statistics: keys compare as unsigned integers in value order
__device__ inline uint64_t rank_key(double v) { return chain_key((uint64_t)__double_as_longlong(v)); }

// ---- gather ----
// Workgroup b of a 1-D grid: position tile b % ntile_p (64 positions p = walker * ld + column of a row), sample tile b / ntile_p of the
// nhalf * ntile_i tiles of 64 samples of a half.  Wave w loads the samples w, w + 4, ... of the tile, lane l position p0 + l, into
// t[sample][position]; then wave w writes the positions w, w + 4, ..., lane l sample i0 + l: 64 consecutive keys of one chain.
struct GatherArgs {
    const void* src;                   // [sample][nl][ld], float or double
    const int32_t* rank;               // [nl]: index of a walker among the selected ones, -1: not selected
    const double* centre;              // [ncols] or nullptr: fold about it
    uint64_t* keys;                    // [ncols][S], S = m h; column c, chain j = hf * nw + k, sample i at c S + j h + i
    unsigned long long* nan_count;     // [ncols]
    int64_t first, half_off, h, nl, ld, np, nw, S, ntile_p, ntile_i;
    int32_t ndim, is_float, col0;
};

__global__ __launch_bounds__(kRankThreads) void rank_gather(GatherArgs a)
{
    __shared__ uint64_t t[kRankGatherTile][kRankGatherTile + 1];
    const int tid = (int)threadIdx.x, lane = tid & (kRankLanes - 1), wave = tid >> 6;
    const int64_t tp = (int64_t)blockIdx.x % a.ntile_p, ts = (int64_t)blockIdx.x / a.ntile_p;
    const int64_t hf = ts / a.ntile_i, i0 = (ts - hf * a.ntile_i) * kRankGatherTile, p0 = tp * kRankGatherTile;
    const int64_t row = a.nl * a.ld, base = a.first + hf * a.half_off;
    {
        const int64_t p = p0 + lane;
        int64_t w = 0;
        int32_t c = 0;
        const bool ok = chain_lane(a.rank, p, a.np, a.ld, a.ndim, &w, &c);
        unsigned long long nans = 0;
        for (int s = wave; s < kRankGatherTile; s += kRankWaves) {
            const int64_t i = i0 + s;
            uint64_t key = 0;
            if (ok && i < a.h) {
                const double v = rank_value(a.src, a.is_float, (base + i) * row + p, a.centre, a.col0 + c);
                nans += v != v;
                key = rank_key(v);
            }
            t[s][lane] = key;
        }
        if (nans) atomicAdd(&a.nan_count[a.col0 + c], nans);
    }
    __syncthreads();
    const int64_t i = i0 + lane;
    for (int pp = wave; pp < kRankGatherTile; pp += kRankWaves) {
        const int64_t p = p0 + pp;
        if (p >= a.np) break;
        int64_t w = 0;
        int32_t c = 0;
        if (!chain_lane_in_row(a.rank, p, a.ld, a.ndim, &w, &c) || i >= a.h) continue;
        const int32_t k = a.rank[w];
        __builtin_assume(k >= 0);                  // (chain_lane_in_row has seen it; told so, the compiler widens k without a sign extension)
        a.keys[(int64_t)(a.col0 + c) * a.S + (hf * a.nw + k) * a.h + i] = t[lane][pp];
    }
}

// ---- segmented radix sort ----
struct SortArgs {
    const uint64_t* in;                // [ncols][S]
    uint64_t* out;                     // [ncols][S]
    uint32_t* counts;                  // [ncols][ntiles][256]: digit counts of a tile; after the scan, where the tile's keys of a digit go
    int64_t S, ntiles;
    int32_t shift;
};

__device__ inline uint32_t rank_scan256(uint32_t v, uint32_t* lds, int tid)     // exclusive, over the 256 threads; lds[256]
{
    lds[tid] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kRankBins; d <<= 1) {
        const uint32_t add = tid >= d ? lds[tid - d] : 0u;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[tid];
    __syncthreads();
    return incl - v;
}

// workgroup (tile, column): the digit counts of the tile's keys, to the tile's own slot
__global__ __launch_bounds__(kRankThreads) void rank_sort_hist(SortArgs a)
{
    __shared__ uint32_t cnt[kRankBins];
    const int tid = (int)threadIdx.x;
    const int64_t tile = blockIdx.x, c = blockIdx.y, k0 = tile * kRankTileKeys;
    const uint64_t* in = a.in + c * a.S;
    cnt[tid] = 0;
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kRankKeysPerThread; ++r) {
        const int64_t at = k0 + r * kRankThreads + tid;
        if (at < a.S) atomicAdd(&cnt[(uint32_t)(in[at] >> a.shift) & (kRankBins - 1)], 1u);
    }
    __syncthreads();
    a.counts[(c * a.ntiles + tile) * kRankBins + tid] = cnt[tid];
}

// workgroup (column): exclusive scan of the counts over (digit, tile), digit-major.  Thread d adds its digit's counts in tile order.
__global__ __launch_bounds__(kRankThreads) void rank_sort_scan(SortArgs a)
{
    __shared__ uint32_t lds[kRankBins];
    const int tid = (int)threadIdx.x;
    uint32_t* cnt = a.counts + (int64_t)blockIdx.x * a.ntiles * kRankBins + tid;
    uint32_t total = 0;
    for (int64_t t = 0; t < a.ntiles; ++t) total += cnt[t * kRankBins];
    uint32_t run = rank_scan256(total, lds, tid);
    for (int64_t t = 0; t < a.ntiles; ++t) {
        const uint32_t n = cnt[t * kRankBins];
        cnt[t * kRankBins] = run;
        run += n;
    }
}

// workgroup (tile, column): the stable scatter.  Wave w takes the keys [1024 w, 1024 (w + 1)) of the tile, 64 at a time in order.  Eight
// ballots give every lane the mask of the lanes that hold its digit; the popcount below the lane is its place among them in arrival
// order, on top of the wave's counter of that digit, which the first lane of the group then advances.  The waves' counters are combined
// in wave order, the tile is laid out in LDS in digit order (so that the stores of a digit run are consecutive) and written to
// where the scan said.
__global__ __launch_bounds__(kRankThreads) void rank_sort_scatter(SortArgs a)
{
    __shared__ uint64_t tile[kRankTileKeys];
    __shared__ uint32_t wcnt[kRankWaves][kRankBins];
    __shared__ uint32_t dstart[kRankBins];
    __shared__ uint32_t gbase[kRankBins];
    const int tid = (int)threadIdx.x, lane = tid & (kRankLanes - 1), wave = tid >> 6;
    const int64_t tl = blockIdx.x, c = blockIdx.y, k0 = tl * kRankTileKeys;
    const uint64_t* in = a.in + c * a.S + k0;
    uint64_t* out = a.out + c * a.S;
    const int nk = (int)(a.S - k0 < kRankTileKeys ? a.S - k0 : kRankTileKeys);
#pragma unroll
    for (int w = 0; w < kRankWaves; ++w) wcnt[w][tid] = 0;
    __syncthreads();

    uint64_t key[kRankKeysPerThread];
    uint32_t place[kRankKeysPerThread];
    const uint64_t below_mask = ((uint64_t)1 << lane) - 1;
#pragma unroll
    for (int r = 0; r < kRankKeysPerThread; ++r) {
        const int li = wave * kRankWaveKeys + r * kRankLanes + lane;
        const bool ok = li < nk;
        key[r] = ok ? in[li] : ~(uint64_t)0;
    }
#pragma unroll
    for (int r = 0; r < kRankKeysPerThread; ++r) {
        const int li = wave * kRankWaveKeys + r * kRankLanes + lane;
        const bool ok = li < nk;
        const uint32_t d = (uint32_t)(key[r] >> a.shift) & (kRankBins - 1);
        uint64_t same = __ballot(ok);
#pragma unroll
        for (int b = 0; b < kRankDigitBits; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t before = (uint32_t)__popcll(same & below_mask);
        const uint32_t seen = wcnt[wave][d];
        place[r] = seen + before;
        __builtin_amdgcn_wave_barrier();
        if (ok && before == 0) wcnt[wave][d] = seen + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();

    uint32_t wc[kRankWaves], total = 0;
#pragma unroll
    for (int w = 0; w < kRankWaves; ++w) { wc[w] = wcnt[w][tid]; total += wc[w]; }
    const uint32_t start = rank_scan256(total, dstart, tid);                   // where digit tid starts in the tile
    dstart[tid] = start;
    gbase[tid] = a.counts[(c * a.ntiles + tl) * kRankBins + tid] - start;       // (mod 2^32: gbase + place in tile = place in column)
    uint32_t run = start;
#pragma unroll
    for (int w = 0; w < kRankWaves; ++w) { wcnt[w][tid] = run; run += wc[w]; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRankKeysPerThread; ++r) {
        const int li = wave * kRankWaveKeys + r * kRankLanes + lane;
        if (li < nk) {
            const uint32_t d = (uint32_t)(key[r] >> a.shift) & (kRankBins - 1);
            const uint32_t at = wcnt[wave][d] + place[r];
            if (at < (uint32_t)nk) tile[at] = key[r];
        }
    }
    __syncthreads();
    for (int i = tid; i < nk; i += kRankThreads) {
        const uint64_t k = tile[i];
        const int64_t at = (int64_t)(uint32_t)(gbase[(uint32_t)(k >> a.shift) & (kRankBins - 1)] + (uint32_t)i);
        if (at < a.S) out[at] = k;
    }
}

// ---- order statistics out of the sorted columns, at given positions ----
struct SelectArgs {
    const uint64_t* sorted;            // [ncols][S]
    const int64_t* pos;                // [n]: c S + index, checked by the host
    uint64_t* out;                     // [n]
    int64_t n;
};

__global__ __launch_bounds__(kRankThreads) void rank_select(SelectArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kRankThreads + threadIdx.x;
    if (e < a.n) a.out[e] = a.sorted[a.pos[e]];
}

// ---- score ----
// One thread per element of the selection in chain order, e = (hf h + i) np + p: the lanes of a wave read consecutive positions of a row
// and write consecutive columns of the scratch row.
struct ScoreArgs {
    const void* src;
    const int32_t* rank;
    const uint64_t* sorted;            // [ncols][S]
    const double* centre;              // [3][ncols] (median, q05, q95) or nullptr; folded: the values are |x - median|
    double* scratch;                   // [n][nw][lds_cols] or nullptr
    int64_t* out_rank2;                // [ncols][S] or nullptr
    double* out_z;                     // [ncols][S] or nullptr
    int64_t first, half_off, h, nl, ld, np, nw, S, lds_cols, nelem;
    int32_t ndim, is_float, col0, ncols, folded, indicators, zcol0;
};

__global__ __launch_bounds__(kRankThreads) void rank_score(ScoreArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kRankThreads + threadIdx.x;
    if (e >= a.nelem) return;
    const int64_t r = e / a.np, p = e - r * a.np;
    const int64_t hf = r / a.h, i = r - hf * a.h;
    int64_t w = 0;
    int32_t cs = 0;
    if (!chain_lane_in_row(a.rank, p, a.ld, a.ndim, &w, &cs)) return;
    const int32_t k = a.rank[w];
    const int32_t c = a.col0 + cs;
    const double x = rank_value(a.src, a.is_float, (a.first + hf * a.half_off + i) * (a.nl * a.ld) + p, nullptr, 0);
    const double v = a.folded ? fabs(x - a.centre[c]) + 0.0 : x;
    const uint64_t key = rank_key(v);
    const uint64_t* col = a.sorted + (int64_t)c * a.S;
    // lower = #{y < v}, upper = #{y <= v}: one path while every probe differs from the key
    int64_t lo = 0, hi = a.S, lower, upper;
    for (;;) {
        if (lo >= hi) { lower = upper = lo; break; }
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t y = col[mid];
        if (y < key) lo = mid + 1;
        else if (y > key) hi = mid;
        else {
            int64_t l0 = lo, l1 = mid;                                       // the first index with col >= key lies in [lo, mid]
            while (l0 < l1) {
                const int64_t m2 = l0 + ((l1 - l0) >> 1);
                if (col[m2] < key) l0 = m2 + 1; else l1 = m2;
            }
            int64_t u0 = mid + 1, u1 = hi;                                   // the first index with col > key lies in [mid + 1, hi]
            while (u0 < u1) {
                const int64_t m2 = u0 + ((u1 - u0) >> 1);
                if (col[m2] <= key) u0 = m2 + 1; else u1 = m2;
            }
            lower = l0; upper = u0;
            break;
        }
    }
    const int64_t rank2 = lower + upper + 1;
    const double z = rank_score_of(rank2, a.S);
    if (a.scratch) {
        double* srow = a.scratch + ((hf * a.half_off + i) * a.nw + k) * a.lds_cols;
        srow[a.zcol0 + c] = z;
        if (a.indicators) {
            srow[2 * a.ncols + c] = x <= a.centre[a.ncols + c] ? 1.0 : 0.0;
            srow[3 * a.ncols + c] = x <= a.centre[2 * a.ncols + c] ? 1.0 : 0.0;
        }
    }
    const int64_t at = (int64_t)c * a.S + (hf * a.nw + k) * a.h + i;
    if (a.out_rank2) a.out_rank2[at] = rank2;
    if (a.out_z) a.out_z[at] = z;
}

}  // namespace kmc_rank
