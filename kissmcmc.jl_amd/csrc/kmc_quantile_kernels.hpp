// kmc_quantile_kernels.hpp -- device kernels of the effective sample size and Monte-Carlo standard error of quantiles (kmc_quantile.hip;
// include/kissmcmc_hip.h): the indicators x <= q_p of a stored chain as bit-packed series, and the lag counts
// D_t of those series by XOR and popcount.  Internal.
//
//   qind_pack         reads the selection along the row [sample][walker][ld] (a wave reads 64 consecutive elements of a row), one lane per
//                     (walker, column) position and word: the lane walks the 64 samples of its word and shifts the outcome of x <= thr
//                     into one 64-bit register per probability.  words[p][c][chain j][word]: bit i & 63 of word i >> 6 is I[i][j]; the
//                     bits at and beyond h are zero.  ones[p][c][j] gets the popcounts (integer atomics: a chain of several words has
//                     several lanes).
//   qind_lag_counts   D_t = #{(i, j): t <= i < h, I[i][j] != I[i - t][j]} for a run of lags.  A workgroup stages a run of
//                     kQindChunkWords consecutive words of one (p, c) in LDS; its lanes lie along the lags (so that the words a wave
//                     reads are one LDS address or two: broadcasts), and where there are fewer lags than lanes the remaining lanes split
//                     the words.  The series shifted by t is a funnel of the words t >> 6 and (t >> 6) + 1 back; XOR, mask to the
//                     valid pairs, popcount.  Per workgroup the counts are folded in LDS (32-bit integer atomics) and added to the
//                     64-bit counters [p][c][lag] by one integer atomic per lag: the totals are integers, so nothing depends on order,
//                     geometry or how the lags are cut into calls.
//
// No floating-point atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kmc_chain_kernels.hpp"

namespace kmc_quantile {

using namespace kmc_chain;

constexpr int kQindThreads = 256;
constexpr int kQindWordBits = 64;
constexpr int kQindMaxProbs = 16;
constexpr int kQindChunkWords = 2048;                                            // words of one (p, c) a workgroup stages: 16 KiB
constexpr int kQindLdsBytes = kQindChunkWords * 8 + kQindThreads * 4;
static_assert(kQindLdsBytes <= 64 * 1024, "a workgroup stays under the default LDS limit");

// ---- pack ----
// Workgroup b of a 1-D grid: position tile b % ntile_p (256 positions p = walker * ld + column of a row), then the word, then the half.
struct PackArgs {
    const void* src;                   // [sample][nl][ld], float or double
    const int32_t* rank;               // [nl]: index of a walker among the selected ones, -1: not selected
    const double* thr;                 // [nprobs][ncols]
    uint64_t* words;                   // [nprobs][ncols][m][nwords]
    unsigned long long* ones;          // [nprobs][ncols][m], zeroed
    int64_t first, half_off, h, nl, ld, np, nw, m, nwords, ntile_p;
    int32_t ndim, is_float, col0, ncols, nprobs;
};

__global__ __launch_bounds__(kQindThreads) void qind_pack(PackArgs a)
{
    const int64_t b = blockIdx.x, tp = b % a.ntile_p, rest = b / a.ntile_p, wi = rest % a.nwords, hf = rest / a.nwords;
    const int64_t p = tp * kQindThreads + threadIdx.x;
    int64_t w = 0;
    int32_t cs = 0;
    if (!chain_lane(a.rank, p, a.np, a.ld, a.ndim, &w, &cs)) return;
    const int32_t c = a.col0 + cs;
    const int64_t j = hf * a.nw + a.rank[w];
    double thr[kQindMaxProbs];
    uint64_t wd[kQindMaxProbs];
#pragma unroll
    for (int pr = 0; pr < kQindMaxProbs; ++pr) {
        thr[pr] = pr < a.nprobs ? a.thr[(int64_t)pr * a.ncols + c] : 0.0;
        wd[pr] = 0;
    }
    const int64_t i0 = wi * kQindWordBits, row = a.nl * a.ld;
    const int ns = (int)(a.h - i0 < kQindWordBits ? a.h - i0 : kQindWordBits);
    int64_t at = (a.first + hf * a.half_off + i0) * row + p;
    for (int s = 0; s < ns; ++s, at += row) {
        const double x = chain_load(a.src, a.is_float, at);
#pragma unroll
        for (int pr = 0; pr < kQindMaxProbs; ++pr) wd[pr] |= (uint64_t)(x <= thr[pr]) << s;
    }
#pragma unroll
    for (int pr = 0; pr < kQindMaxProbs; ++pr) {
        if (pr >= a.nprobs) break;
        const int64_t series = ((int64_t)pr * a.ncols + c) * a.m + j;
        a.words[series * a.nwords + wi] = wd[pr];
        const unsigned long long n = (unsigned long long)__popcll(wd[pr]);
        if (n) atomicAdd(&a.ones[series], n);
    }
}

// ---- lag counts ----
// Grid (chunk, column, probability).  wpc = m * nwords < 2^31 words per (p, c).
struct LagCountArgs {
    const uint64_t* words;             // [nprobs][ncols][m][nwords]
    unsigned long long* counts;        // [nprobs][ncols][nlags], zeroed
    int64_t h;
    uint32_t wpc, nwords;
    int32_t lag0, nlags, ncols;
};

__global__ __launch_bounds__(kQindThreads) void qind_lag_counts(LagCountArgs a)
{
    __shared__ uint64_t w[kQindChunkWords];
    __shared__ uint32_t cnt[kQindThreads];
    const int tid = (int)threadIdx.x;
    const int64_t pc = (int64_t)blockIdx.z * a.ncols + blockIdx.y;
    const uint64_t* base = a.words + pc * (int64_t)a.wpc;
    const uint32_t e0 = blockIdx.x * (uint32_t)kQindChunkWords;
    const uint32_t ne = a.wpc - e0 < (uint32_t)kQindChunkWords ? a.wpc - e0 : (uint32_t)kQindChunkWords;
    for (uint32_t i = tid; i < ne; i += kQindThreads) w[i] = base[e0 + i];
    // lt lanes along the lags (a power of two), the other nsub = 256 / lt along the words
    int lbits = 0;
    while ((1 << lbits) < a.nlags && lbits < 8) ++lbits;
    const int nlt = 1 << lbits, lt = tid & (nlt - 1);
    const uint32_t nsub = (uint32_t)(kQindThreads >> lbits), sub = (uint32_t)(tid >> lbits), kstep = nsub % a.nwords;
    const uint32_t last = a.nwords - 1;
    const int64_t tail = a.h - (int64_t)last * kQindWordBits;                   // valid bits of a chain's last word, 1 .. 64
    const uint64_t tail_mask = tail < kQindWordBits ? (((uint64_t)1 << tail) - 1) : ~(uint64_t)0;
    for (int tb = 0; tb < a.nlags; tb += nlt) {
        cnt[tid] = 0;
        __syncthreads();                                                        // (the first time round: the chunk is in place, too)
        if (tb + lt < a.nlags) {
            const uint32_t t = (uint32_t)(a.lag0 + tb + lt), q = t >> 6, r = t & 63;
            uint32_t n = 0, k = (e0 + sub) % a.nwords;
            for (uint32_t i = sub; i < ne; i += nsub) {
                if (k >= q) {                                                   // word k of a chain pairs with its words k - q and k - q - 1
                    const uint32_t e = e0 + i;
                    const uint64_t p0 = e - q >= e0 ? w[i - q] : base[e - q];
                    uint64_t sh = p0 << r;
                    if (r != 0 && k > q) {
                        const uint64_t p1 = e - q - 1 >= e0 ? w[i - q - 1] : base[e - q - 1];
                        sh |= p1 >> (64 - r);
                    }
                    uint64_t x = w[i] ^ sh;
                    if (k == q) x &= ~(uint64_t)0 << r;                         // i >= t
                    if (k == last) x &= tail_mask;                              // i < h
                    n += (uint32_t)__popcll(x);
                }
                k += kstep;
                if (k >= a.nwords) k -= a.nwords;
            }
            if (n) atomicAdd(&cnt[lt], n);
        }
        __syncthreads();
        if (tid < nlt && tb + tid < a.nlags && cnt[tid]) atomicAdd(&a.counts[pc * a.nlags + tb + tid], (unsigned long long)cnt[tid]);
        __syncthreads();
    }
}

}  // namespace kmc_quantile
