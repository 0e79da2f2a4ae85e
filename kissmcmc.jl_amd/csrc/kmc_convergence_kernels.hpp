// kmc_convergence_kernels.hpp -- device kernels of the convergence diagnostics across chains (kmc_convergence.hip): the mean and the
// variance of every chain (conv_moment_partials / conv_moment_fold) and the lag sums D_t = sum_j sum_i (x[i][j] - x[i - t][j])^2 of the
// variogram (conv_lag_partials / conv_lag_fold), from which the host stage takes split-R^, the effective sample size and the
// Monte-Carlo standard error (include/kissmcmc_hip.h).  Internal.
//
// A chain is one selected walker, or one half of it (`split`): samples [first + hf * half_off, ... + h) of the stored chain
// [sample][walker][ld].  Lanes run along the contiguous (walker, column) axis of a sample, position p = walker * ld + column, so that
// the lanes of a wave load consecutive addresses; a lane whose walker is not selected or whose column is padding (column >= ndim) loads
// nothing and adds zeros.  The log-densities [sample][walker] go through the same kernels as a chain of ld = ndim = 1.
//
// No floating-point atomics anywhere: a workgroup writes its sums to a slot of its own in a buffer of partial sums, and a second kernel
// folds the slots in a fixed order, so two identical calls return identical bits.  Every term is formed as the host yardstick forms it
// (a subtraction, a multiplication, both rounded; the library is built with -ffp-contract=off) and only the order of the additions is free.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kmc_chain_kernels.hpp"

namespace kmc_conv {

using namespace kmc_chain;

constexpr int kConvThreads = 256;
constexpr int kConvLanes = 64;                              // positions p of one tile: one wave's width
constexpr int kConvWaves = kConvThreads / kConvLanes;
constexpr int kConvLagBlock = 32;                           // lags one workgroup accumulates from one window in LDS
constexpr int kConvLagsPerLane = kConvLagBlock / kConvWaves;   // ... 8 of them per lane, in registers (wave w: lags 8 w .. 8 w + 7 of the block)
constexpr int kConvTileSamples = 32;                        // leading samples i of one tile
constexpr int kConvPartnerRows = kConvTileSamples + kConvLagBlock - 1;          // trailing samples i - t of one tile: 63
constexpr int kConvWindowRows = kConvPartnerRows + kConvTileSamples;            // 95 rows of 64 doubles
constexpr int kConvLdsBytes = kConvWindowRows * kConvLanes * (int)sizeof(double);   // 48,640 B: under the 64 KiB default dynamic limit
static_assert(kConvLdsBytes <= 64 * 1024, "the window must fit the default dynamic LDS limit");
static_assert(kConvLagBlock * kConvLanes <= kConvWindowRows * kConvLanes, "the reduction reuses the window");
static_assert(kConvTileSamples % kConvLagsPerLane == 0, "a tile is walked in steps of the lags per lane");

// ---- chain moments ----
// pass 0: sum of x; pass 1: sum of (x - mean)^2 with the mean pass 0 left in mean_p.  Workgroup (blockIdx.x, blockIdx.y = hf * nchunk + ck)
// sums the samples [ck * clen, (ck + 1) * clen) of half hf for 256 positions, each lane its own chain, sequentially in sample order;
// part[blockIdx.y][p].  conv_moment_fold adds the chunks of a chain in chunk order and divides: by h (the mean, also kept per position
// for pass 1) or by h - 1 (the variance).
struct MomentArgs {
    const void* src;                   // [sample][nl][ld], float or double
    const int32_t* rank;               // [nl]: index of a walker among the selected ones, -1: not selected
    double* mean_p;                    // [nhalf][np]
    double* part;                      // [nhalf * nchunk][np]
    double* out;                       // pass 0: chain_mean, pass 1: chain_var; [ncols][m], this source's columns from col0
    int64_t first, half_off, h, nl, ld, np, m, nw, clen;
    int32_t ndim, is_float, nhalf, nchunk, pass, col0;
};

__global__ __launch_bounds__(kConvThreads) void conv_moment_partials(MomentArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * kConvThreads + threadIdx.x;
    const int hf = (int)(blockIdx.y / (unsigned)a.nchunk), ck = (int)(blockIdx.y - (unsigned)hf * (unsigned)a.nchunk);
    int64_t w = 0;
    int32_t c = 0;
    if (p >= a.np) return;
    double s = 0.0;
    if (chain_lane(a.rank, p, a.np, a.ld, a.ndim, &w, &c)) {
        const int64_t i0 = (int64_t)ck * a.clen, i1 = i0 + a.clen < a.h ? i0 + a.clen : a.h;
        const int64_t row = a.nl * a.ld;
        int64_t at = (a.first + (int64_t)hf * a.half_off + i0) * row + p;
        if (a.pass == 0) {
#pragma unroll 4
            for (int64_t i = i0; i < i1; ++i, at += row) s += chain_load(a.src, a.is_float, at);
        } else {
            const double mu = a.mean_p[(int64_t)hf * a.np + p];
#pragma unroll 4
            for (int64_t i = i0; i < i1; ++i, at += row) {
                const double d = chain_load(a.src, a.is_float, at) - mu;
                s += d * d;
            }
        }
    }
    a.part[(int64_t)blockIdx.y * a.np + p] = s;
}

__global__ __launch_bounds__(kConvThreads) void conv_moment_fold(MomentArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * kConvThreads + threadIdx.x;
    const int hf = (int)blockIdx.y;
    int64_t w = 0;
    int32_t c = 0;
    if (!chain_lane(a.rank, p, a.np, a.ld, a.ndim, &w, &c)) return;
    double s = 0.0;
    for (int ck = 0; ck < a.nchunk; ++ck) s += a.part[((int64_t)hf * a.nchunk + ck) * a.np + p];
    const double v = a.pass == 0 ? s / (double)a.h : s / (double)(a.h - 1);
    if (a.pass == 0) a.mean_p[(int64_t)hf * a.np + p] = v;
    a.out[(int64_t)(a.col0 + c) * a.m + (int64_t)hf * a.nw + a.rank[w]] = v;
}

// ---- lag sums ----
// The tiles of 64 positions are numbered q = 0 .. ntile_p - 1.  The column of a lane, (64 q + lane) % ld, is the same in every tile of one
// residue q % period, period = ld / gcd(64, ld); a workgroup keeps to one residue, so that a lane's accumulators belong to one column
// throughout.  Workgroup (blockIdx.x = b * period + r, blockIdx.y = hf * nchunk + ck, blockIdx.z = lag block z) takes the position tiles
// q = r + period * (b + nb * k), k = 0, 1, ..., and of each the sample tiles [ck * tpc, (ck + 1) * tpc) of 32 leading samples of half hf,
// for the lags t0 .. t0 + 31, t0 = lag0 + 32 z.
//
// One sample tile: leading samples i in [i0, i0 + 32), trailing samples i - t in [i0 - t0 - 31, i0 + 31 - t0].  The window in LDS holds
// the 63 trailing rows first and then the leading rows that are not among them (all 32 when t0 >= 32; for smaller t0 the two ranges
// overlap and the window is the contiguous run of 31 + t0 + 32 samples), [row][lane] in doubles: every chain element is loaded once per
// tile and lag block as a leading sample and at most (63 / 32) times as a trailing one, not once per lag.  Samples outside [0, h) of the
// half -- before first_sample, in the other half, past the end -- are zero rows and their terms are masked (conv_lag_tile<true>); a tile
// whose window lies inside the half takes the path without masks.  Wave w owns the lags t0 + 8 w + r, r = 0 .. 7, one accumulator each;
// it walks the tile 8 leading samples at a time, with those 8 and the 15 trailing samples they pair with in registers: 23 LDS reads
// for 64 terms.
//
// At the end the accumulators go through LDS ([lag][lane], over the window) and the lanes of one column are added in lane order (ld <
// 64: slot = column; ld >= 64: every lane has a column of its own, slot = lane): part[workgroup][32][nslot].
struct LagArgs {
    const void* src;
    const int32_t* rank;
    double* part;                      // [gridDim.z * gridDim.y * gridDim.x][kConvLagBlock][nslot]
    int64_t first, half_off, h, nl, ld, np, ntile_p;
    int32_t ndim, is_float, period, nb, nchunk, tpc, lag0, nslot;
};

template <bool kEdge>
__device__ inline void conv_lag_tile(const double* win, int cur_base, int wave, int lane, int64_t i0, int64_t h, int t_wave, double (&acc)[kConvLagsPerLane])
{
    constexpr int R = kConvLagsPerLane;
    const int off = kConvLagBlock - 1 - R * wave - (R - 1);                 // window row of the trailing sample of (u = 0, r = R - 1) at ub = 0
#pragma unroll 1
    for (int ub = 0; ub < kConvTileSamples; ub += R) {
        double c[R], q[2 * R - 1];
#pragma unroll
        for (int u = 0; u < R; ++u) c[u] = win[(cur_base + ub + u) * kConvLanes + lane];
#pragma unroll
        for (int k = 0; k < 2 * R - 1; ++k) q[k] = win[(ub + off + k) * kConvLanes + lane];
#pragma unroll
        for (int u = 0; u < R; ++u) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double d = c[u] - q[u - r + R - 1];                         // x[i] - x[i - t], i = i0 + ub + u, t = t_wave + r
                if (kEdge) {
                    const int64_t i = i0 + ub + u;
                    if (!(i < h && i - (t_wave + r) >= 0)) d = 0.0;
                }
                acc[r] += d * d;
            }
        }
    }
}

__global__ __launch_bounds__(kConvThreads) void conv_lag_partials(LagArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double conv_lds[];
    const int tid = (int)threadIdx.x, lane = tid & (kConvLanes - 1), wave = tid >> 6;
    const int r_res = (int)(blockIdx.x % (unsigned)a.period), b = (int)(blockIdx.x / (unsigned)a.period);
    const int hf = (int)(blockIdx.y / (unsigned)a.nchunk), ck = (int)(blockIdx.y - (unsigned)hf * (unsigned)a.nchunk);
    const int t0 = a.lag0 + kConvLagBlock * (int)blockIdx.z;
    const int t_wave = t0 + kConvLagsPerLane * wave;
    const int64_t row = a.nl * a.ld, base = a.first + (int64_t)hf * a.half_off;
    const int64_t ntile_i = (a.h + kConvTileSamples - 1) / kConvTileSamples;
    const int64_t ti0 = (int64_t)ck * a.tpc, ti1 = ti0 + a.tpc < ntile_i ? ti0 + a.tpc : ntile_i;
    const int span = t0 + kConvLagBlock - 1;                               // i0 - span: the first trailing sample of a tile
    const int cur_base = span < kConvPartnerRows ? span : kConvPartnerRows;
    const int nrows = cur_base + kConvTileSamples;

    double acc[kConvLagsPerLane];
#pragma unroll
    for (int r = 0; r < kConvLagsPerLane; ++r) acc[r] = 0.0;

    for (int64_t q = r_res + (int64_t)a.period * b; q < a.ntile_p; q += (int64_t)a.period * a.nb) {
        const int64_t p = q * kConvLanes + lane;
        int64_t w = 0;
        int32_t c = 0;
        const bool lane_ok = chain_lane(a.rank, p, a.np, a.ld, a.ndim, &w, &c);
        for (int64_t ti = ti0; ti < ti1; ++ti) {
            const int64_t i0 = ti * kConvTileSamples;
#pragma unroll 4
            for (int s = wave; s < nrows; s += kConvWaves) {
                const int64_t li = s < kConvPartnerRows ? i0 - span + s : i0 + (s - cur_base);
                double x = 0.0;
                if (lane_ok && li >= 0 && li < a.h) x = chain_load(a.src, a.is_float, (base + li) * row + p);
                conv_lds[s * kConvLanes + lane] = x;
            }
            __syncthreads();
            if (i0 - span >= 0 && i0 + kConvTileSamples <= a.h) conv_lag_tile<false>(conv_lds, cur_base, wave, lane, i0, a.h, t_wave, acc);
            else conv_lag_tile<true>(conv_lds, cur_base, wave, lane, i0, a.h, t_wave, acc);
            __syncthreads();
        }
    }

#pragma unroll
    for (int r = 0; r < kConvLagsPerLane; ++r) conv_lds[(kConvLagsPerLane * wave + r) * kConvLanes + lane] = acc[r];
    __syncthreads();
    const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    double* out = a.part + blk * kConvLagBlock * a.nslot;
    const int col_first = (int)(((int64_t)kConvLanes * r_res) % a.ld);     // the column of lane 0 (ld < 64)
    for (int o = tid; o < kConvLagBlock * a.nslot; o += kConvThreads) {
        const int lag = o / a.nslot, slot = o - lag * a.nslot;
        double s;
        if (a.ld >= kConvLanes) {
            s = conv_lds[lag * kConvLanes + slot];
        } else {
            s = 0.0;
            int l = slot - col_first;
            if (l < 0) l += (int)a.ld;
            for (; l < kConvLanes; l += (int)a.ld) s += conv_lds[lag * kConvLanes + l];
        }
        out[o] = s;
    }
}

// D_t of one column and one lag: workgroup (blockIdx.x = column of this source, blockIdx.y = lag index L) of one wave.  The partial sums
// of the column -- one slot in every workgroup of conv_lag_partials' grid (gx, gy) of lag block L / 32 that holds the column -- are dealt
// to the lanes in workgroup order (lane l: entries l, l + 64, ...), each lane adds its own in that order, and the 64 lane sums are added
// as a binary tree: a fixed order.
struct LagFoldArgs {
    const double* part;
    double* out;                       // [ncols][nlags_out], this source's columns from col0, this call's lags from lag_out0
    int64_t ld, nlags_out;
    int32_t gx, gy, period, nslot, col0, lag_out0;
};

__global__ __launch_bounds__(kConvLanes) void conv_lag_fold(LagFoldArgs a)
{
    const int c = (int)blockIdx.x, L = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int z = L / kConvLagBlock, lag = L - z * kConvLagBlock;
    const int64_t n = (int64_t)a.gx * a.gy;
    double s = 0.0;
    for (int64_t e = lane; e < n; e += kConvLanes) {
        int slot = c;
        if (a.ld >= kConvLanes) {
            const int r_res = (int)((e % a.gx) % a.period);
            slot = c - (int)(((int64_t)kConvLanes * r_res) % a.ld);
            if (slot < 0) slot += (int)a.ld;
            if (slot >= kConvLanes) continue;                              // this workgroup's tiles do not hold the column
        }
        s += a.part[(((int64_t)z * n + e) * kConvLagBlock + lag) * a.nslot + slot];
    }
#pragma unroll
    for (int d = kConvLanes / 2; d >= 1; d >>= 1) s += __shfl_down(s, d, kConvLanes);
    if (lane == 0) a.out[(int64_t)(a.col0 + c) * a.nlags_out + a.lag_out0 + L] = s;
}

}  // namespace kmc_conv
