// kmc_hdi_kernels.hpp -- device kernels of the highest-density interval of a stored chain (kmc_hdi.hip; include/kissmcmc_hip.h; DESIGN.md
// section 4m): the scan over a sorted column for the narrowest window of k + 1 consecutive draws.  The columns are gathered and sorted
// by the kernels of the rank statistics (kmc_rank_kernels.hpp, through kmc_rank_host.hpp); what is here reads their sorted keys.  Internal.
//
// Two kernels, every column and every probability on its own:
//   hdi_scan    workgroup (tile, column): 256 lanes take kHdiTileStarts consecutive window starts i of the column, 16 per lane, lane l of
//               the workgroup the starts tile * 4096 + r * 256 + l, so that every load is coalesced across the wave.  A lane loads key[i]
//               once and key[i + k_p] for every probability p, decodes both, subtracts in double and keeps its best (bits(w), i) per
//               probability as two 64-bit integers; a NaN width has the bits all-ones, a start with i >= N - k_p contributes the
//               identity (all-ones, all-ones).  The lanes' bests are reduced across the wave by cross-lane operations and across the
//               four waves through LDS: one partial per (column, probability, tile).
//   hdi_fold    one wave per (column, probability): the minimum of the tile partials, then i*, key[i*] and key[i* + k_p].
//
// w_i is never negative, so the order "(is NaN, width, i)" is the unsigned order of (bits, i): integer compares only, no atomics, no
// floating-point minimum.  The order is total and its minimum unique, so nothing depends on the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kmc_chain_kernels.hpp"

namespace kmc_hdi {

using namespace kmc_chain;

constexpr int kHdiThreads = 256;
constexpr int kHdiLanes = 64;
constexpr int kHdiWaves = kHdiThreads / kHdiLanes;
constexpr int kHdiStartsPerThread = 16;
constexpr int kHdiTileStarts = kHdiThreads * kHdiStartsPerThread;               // 4096 window starts: one workgroup's tile
constexpr int kHdiMaxProbs = 16;
constexpr uint64_t kHdiNone = ~(uint64_t)0;

struct HdiArgs {
    const uint64_t* keys;              // [ncols][N], every column sorted ascending
    uint64_t* part;                    // [ncols][nprob][ntiles][2]: (bits of the width, start) of the tile's best window
    uint64_t* out;                     // [ncols][nprob][3]: start (-1: none), key[start], key[start + k]
    int64_t N, ntiles;
    int32_t nprob;
    int64_t k[kHdiMaxProbs];
};

__device__ inline double hdi_value(uint64_t key) { return __longlong_as_double((long long)chain_unkey(key)); }

// (b, i) < (bb, bi) in the order of the rule
__device__ inline bool hdi_less(uint64_t b, uint64_t i, uint64_t bb, uint64_t bi) { return b < bb || (b == bb && i < bi); }

__device__ inline void hdi_wave_min(uint64_t& b, uint64_t& i)
{
#pragma unroll
    for (int d = kHdiLanes / 2; d >= 1; d >>= 1) {
        const uint64_t ob = (uint64_t)__shfl_xor((unsigned long long)b, d, kHdiLanes);
        const uint64_t oi = (uint64_t)__shfl_xor((unsigned long long)i, d, kHdiLanes);
        if (hdi_less(ob, oi, b, i)) { b = ob; i = oi; }
    }
}

// P: the probabilities the instance keeps in registers, nprob <= P of them in use
template <int P>
__global__ __launch_bounds__(kHdiThreads) void hdi_scan(HdiArgs a)
{
    __shared__ uint64_t wb[kHdiWaves][P], wi[kHdiWaves][P];
    const int tid = (int)threadIdx.x, lane = tid & (kHdiLanes - 1), wave = tid >> 6;
    const int64_t tile = blockIdx.x, c = blockIdx.y;
    const uint64_t* col = a.keys + c * a.N;
    uint64_t bb[P], bi[P];
#pragma unroll
    for (int p = 0; p < P; ++p) { bb[p] = kHdiNone; bi[p] = kHdiNone; }
    int64_t kmin = a.k[0];
#pragma unroll
    for (int p = 1; p < P; ++p)
        if (p < a.nprob && a.k[p] < kmin) kmin = a.k[p];
#pragma unroll 4
    for (int r = 0; r < kHdiStartsPerThread; ++r) {
        const int64_t i = tile * kHdiTileStarts + r * kHdiThreads + tid;
        if (i >= a.N - kmin) continue;                                         // no probability has a window that starts here
        const double lo = hdi_value(col[i]);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (p >= a.nprob || i >= a.N - a.k[p]) continue;
            const double w = hdi_value(col[i + a.k[p]]) - lo;
            const uint64_t b = w != w ? kHdiNone : (uint64_t)__double_as_longlong(w);
            if (hdi_less(b, (uint64_t)i, bb[p], bi[p])) { bb[p] = b; bi[p] = (uint64_t)i; }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (p >= a.nprob) continue;
        hdi_wave_min(bb[p], bi[p]);
        if (lane == 0) { wb[wave][p] = bb[p]; wi[wave][p] = bi[p]; }
    }
    __syncthreads();
    if (tid < a.nprob) {
        uint64_t b = wb[0][tid], i = wi[0][tid];
#pragma unroll
        for (int w = 1; w < kHdiWaves; ++w)
            if (hdi_less(wb[w][tid], wi[w][tid], b, i)) { b = wb[w][tid]; i = wi[w][tid]; }
        uint64_t* o = a.part + ((c * a.nprob + tid) * a.ntiles + tile) * 2;
        o[0] = b; o[1] = i;
    }
}

// workgroup c * nprob + p, one wave
__global__ __launch_bounds__(kHdiLanes) void hdi_fold(HdiArgs a)
{
    const int lane = (int)threadIdx.x;
    const int64_t slot = blockIdx.x, c = slot / a.nprob;
    const int p = (int)(slot - c * a.nprob);
    const uint64_t* part = a.part + slot * a.ntiles * 2;
    uint64_t b = kHdiNone, i = kHdiNone;
    for (int64_t t = lane; t < a.ntiles; t += kHdiLanes) {
        const uint64_t tb = part[2 * t], ti = part[2 * t + 1];
        if (hdi_less(tb, ti, b, i)) { b = tb; i = ti; }
    }
    hdi_wave_min(b, i);
    if (lane != 0) return;
    const int64_t k = a.k[p];
    const uint64_t* col = a.keys + c * a.N;
    uint64_t* o = a.out + slot * 3;
    const bool found = i < (uint64_t)(a.N - k);                                // (always, for 1 <= k <= N - 1: window 0 exists)
    o[0] = found ? i : kHdiNone;
    o[1] = found ? col[i] : 0;
    o[2] = found ? col[i + (uint64_t)k] : 0;
}

}  // namespace kmc_hdi
