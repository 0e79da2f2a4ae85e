// kmc_hist_kernels.hpp -- device kernels of the marginal histograms (kmc_hist.hip): the 1-D histogram of every selected column of a stored
// chain in one read of it (hist1d), and the 2-D histograms of all pairs of up to 16 selected columns (hist2d).  Internal.
//
// The rule (include/kissmcmc_hip.h): with strictly increasing edges e[0..B], x falls in bin i iff e[i] <= x < e[i + 1], the last bin is
// closed (x == e[B] -> B - 1), x < e[0] is `below`, x > e[B] is `above`, a NaN is `nan`.  The bin comes from comparisons against the
// edges alone -- a binary search over e[] in LDS (hist_bin) -- never from float arithmetic, so the counts equal
// np.histogram(x, bins=e) for any edges.  Counts are integers: 32-bit LDS atomics per workgroup, flushed by 64-bit integer atomic
// adds, so the result does not depend on the launch geometry or on the order in which workgroups arrive.  No float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kmc_chain_kernels.hpp"

namespace kmc_hist {

using namespace kmc_chain;

// What one workgroup may ask of LDS: the default dynamic limit of a kernel, which needs no function attribute and leaves room for two
// workgroups per compute unit.  Edges, counters and hist2d's tile of bin indices all come out of it.
constexpr int kHistLdsBytes = 64 * 1024;
constexpr int kHistThreads = 256;
constexpr int kHistWaves = kHistThreads / 64;
constexpr int kHistMaxBins = 256;                       // hist1d
constexpr int kHistMaxBins2 = 64;                       // hist2d: a bin index is a byte, kHistOut is none
constexpr int kHistMaxDims2 = 16;                       // hist2d: selected columns (120 pairs)
constexpr int kHistTileRows = 256;                      // hist2d: rows of one tile
constexpr int kHistUnroll = 4;                          // hist1d: loads a thread has in flight
constexpr int kHistBelow = -1, kHistAbove = -2, kHistNan = -3;
constexpr uint8_t kHistOut = 255;

// bin of x among e[0..B] (see above); e may be LDS or global memory
__host__ __device__ inline int hist_bin(const double* e, int B, double x)
{
    if (x != x) return kHistNan;
    if (x < e[0]) return kHistBelow;
    if (x > e[B]) return kHistAbove;
    int lo = 0, hi = B;                                 // e[lo] <= x, and x < e[hi] or hi == B
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- hist1d ----
// The columns of the chain are cut into groups of 1 << cg_shift as in select_hist (kmc_summary_kernels.hpp), lanes along the row; `groups`
// lists the groups that hold a selected column, and the log-densities are one more group of one column (number ndim) when lp_slot >= 0.
// Workgroup blockIdx.x = g * nwg + b reads the rows b, b + nwg, ... of its group, 256 >> shift at a time.  LDS: the group's edges
// [columns][B + 1], then `copies` copies of the counters [columns][B + 3] (B bins, below, above, nan); wave w counts in copy
// w % copies, and the copies are folded at the flush.  A column that is not selected (slot < 0) loads nothing.
struct Hist1Args {
    const void* chain;                 // [sample][walker][ld], float or double
    const double* logp;                // [sample][walker] or nullptr
    const uint8_t* mask;               // [nl] or nullptr: walkers that count
    const double* edges;               // [slots][B + 1]
    const int32_t* slot_of_col;        // [ndim]: output slot of a chain column, -1: not selected
    const int32_t* groups;             // [ngroups_chain]: the column groups to read
    unsigned long long* out;           // [slots][B + 3], zero at launch
    int64_t row0, nrows, nl, ld;       // rows [row0, row0 + nrows) of the chain, row = sample * nl + walker
    int32_t ndim, is_float, nbins, cg_shift, ngroups_chain, lp_slot, nwg, copies;
};

__global__ __launch_bounds__(kHistThreads) void hist1d(Hist1Args a)
{
    extern __shared__ double hist_lds[];
    const int tid = (int)threadIdx.x;
    const int gi = (int)(blockIdx.x / (unsigned)a.nwg), b = (int)(blockIdx.x - (unsigned)gi * (unsigned)a.nwg);
    const bool is_lp = gi >= a.ngroups_chain;
    const int sh = is_lp ? 0 : a.cg_shift;
    const int c0 = is_lp ? a.ndim : (a.groups[gi] << sh);
    const int ncol = is_lp ? 1 : ((a.ndim - c0) < (1 << sh) ? (a.ndim - c0) : (1 << sh));
    const int B = a.nbins, ne = B + 1, nc = B + 3;
    double* le = hist_lds;                                                 // [ncol][ne]
    uint32_t* lc = reinterpret_cast<uint32_t*>(hist_lds + ncol * ne);      // [copies][ncol][nc]
    for (int i = tid; i < ncol * ne; i += kHistThreads) {
        const int c = i / ne, slot = is_lp ? a.lp_slot : a.slot_of_col[c0 + c];
        le[i] = slot >= 0 ? a.edges[(int64_t)slot * ne + (i - c * ne)] : 0.0;
    }
    for (int i = tid; i < a.copies * ncol * nc; i += kHistThreads) lc[i] = 0u;
    __syncthreads();

    const int c = tid & ((1 << sh) - 1), rsub = tid >> sh;
    const int64_t rp = kHistThreads >> sh;              // rows per step of this workgroup
    const int64_t nsteps = (a.nrows + rp - 1) / rp;
    const bool col_ok = c < ncol && (is_lp || a.slot_of_col[c0 + c] >= 0);
    const bool small_rows = a.nrows <= 0xffffffffll;
    const double* my_e = le + c * ne;
    uint32_t* my_c = lc + (((tid >> 6) % a.copies) * ncol + c) * nc;
    for (int64_t it = b; it < nsteps; it += (int64_t)a.nwg * kHistUnroll) {
        double v[kHistUnroll];
        bool ok[kHistUnroll];
#pragma unroll
        for (int u = 0; u < kHistUnroll; ++u) {
            const int64_t step = it + (int64_t)u * a.nwg;
            const int64_t row = step * rp + rsub;
            ok[u] = col_ok && step < nsteps && row < a.nrows;
            if (ok[u] && a.mask) {
                const int64_t w = small_rows ? (int64_t)((uint32_t)row % (uint32_t)a.nl) : row % a.nl;
                ok[u] = a.mask[w] != 0;
            }
            v[u] = 0.0;
            if (ok[u]) {
                const int64_t r = a.row0 + row;
                if (is_lp) v[u] = a.logp[r];
                else if (a.is_float) v[u] = (double)reinterpret_cast<const float*>(a.chain)[r * a.ld + c0 + c];   // exact
                else v[u] = reinterpret_cast<const double*>(a.chain)[r * a.ld + c0 + c];
            }
        }
#pragma unroll
        for (int u = 0; u < kHistUnroll; ++u) {
            if (!ok[u]) continue;
            const int bin = hist_bin(my_e, B, v[u]);
            atomicAdd(&my_c[bin >= 0 ? bin : B - 1 - bin], 1u);            // below, above, nan: B, B + 1, B + 2
        }
    }
    __syncthreads();
    for (int i = tid; i < ncol * nc; i += kHistThreads) {
        uint32_t n = 0;
        for (int k = 0; k < a.copies; ++k) n += lc[k * ncol * nc + i];
        if (!n) continue;
        const int cc = i / nc, slot = is_lp ? a.lp_slot : a.slot_of_col[c0 + cc];
        atomicAdd(&a.out[(int64_t)slot * nc + (i - cc * nc)], (unsigned long long)n);
    }
}

// ---- hist2d ----
// All pairs (a, b), a < b in list order, of nsel <= 16 selected columns, B <= 64.  The pairs are cut into groups of ppg so that a group's
// counters [pair][B][B] fit LDS next to the edges and the tile; workgroup blockIdx.x = g * nwg + b takes the tiles b, b + nwg, ... of
// kHistTileRows rows for the pairs [g * ppg, ...).  Per tile, phase one: lanes over (row, selected column), the column fastest, find every
// element's bin once and store it as a byte (kHistOut: outside, NaN, a row beyond the end or of a walker that does not count); phase two:
// lanes over (row, pair), the pair fastest -- so that the lanes of a wave add into different pairs' tables -- do one LDS atomic add each.
struct Hist2Args {
    const void* chain;
    const uint8_t* mask;
    const double* edges;               // [nsel][B + 1]
    const int32_t* dims;               // [nsel] chain columns
    const uint8_t* pair_ab;            // [npairs][2]: indices into dims
    unsigned long long* out;           // [npairs][B][B], zero at launch
    int64_t row0, nrows, nl, ld;
    int32_t is_float, nbins, nsel, sel_shift, npairs, ppg, nwg;
};

__global__ __launch_bounds__(kHistThreads) void hist2d(Hist2Args a)
{
    extern __shared__ double hist_lds[];
    const int tid = (int)threadIdx.x;
    const int g = (int)(blockIdx.x / (unsigned)a.nwg), b = (int)(blockIdx.x - (unsigned)g * (unsigned)a.nwg);
    const int B = a.nbins, ne = B + 1, p0 = g * a.ppg;
    const int np = (a.npairs - p0) < a.ppg ? (a.npairs - p0) : a.ppg;
    double* le = hist_lds;                                                 // [nsel][ne]
    uint32_t* lc = reinterpret_cast<uint32_t*>(le + a.nsel * ne);          // [np][B][B]
    uint8_t* tile = reinterpret_cast<uint8_t*>(lc + a.ppg * B * B);        // [kHistTileRows][1 << sel_shift]
    uint8_t* lab = tile + (kHistTileRows << a.sel_shift);                  // [np][2]
    for (int i = tid; i < a.nsel * ne; i += kHistThreads) le[i] = a.edges[i];
    for (int i = tid; i < np * B * B; i += kHistThreads) lc[i] = 0u;
    for (int i = tid; i < np * 2; i += kHistThreads) lab[i] = a.pair_ab[p0 * 2 + i];
    __syncthreads();

    const int64_t ntiles = (a.nrows + kHistTileRows - 1) / kHistTileRows;
    const bool small_rows = a.nrows <= 0xffffffffll;
    const int j = tid & ((1 << a.sel_shift) - 1), rsub = tid >> a.sel_shift, rstep = kHistThreads >> a.sel_shift;
    const bool col_ok = j < a.nsel;
    const int64_t col = col_ok ? a.dims[j] : 0;
    const double* my_e = le + (col_ok ? j : 0) * ne;
    for (int64_t t = b; t < ntiles; t += a.nwg) {
        const int64_t base = t * kHistTileRows;
#pragma unroll 4
        for (int r = rsub; r < kHistTileRows; r += rstep) {                // phase one
            const int64_t row = base + r;
            bool ok = col_ok && row < a.nrows;
            if (ok && a.mask) {
                const int64_t w = small_rows ? (int64_t)((uint32_t)row % (uint32_t)a.nl) : row % a.nl;
                ok = a.mask[w] != 0;
            }
            int bin = -1;
            if (ok) {
                bin = hist_bin(my_e, B, chain_load(a.chain, a.is_float, (a.row0 + row) * a.ld + col));
            }
            tile[(r << a.sel_shift) + j] = bin >= 0 ? (uint8_t)bin : kHistOut;
        }
        __syncthreads();
        const int64_t left = a.nrows - base;
        const int rows = left < kHistTileRows ? (int)left : kHistTileRows;
        for (int i = tid; i < rows * np; i += kHistThreads) {              // phase two
            const int r = i / np, p = i - r * np;
            const uint8_t ia = tile[(r << a.sel_shift) + lab[2 * p]], ib = tile[(r << a.sel_shift) + lab[2 * p + 1]];
            if (ia != kHistOut && ib != kHistOut) atomicAdd(&lc[(p * B + ia) * B + ib], 1u);
        }
        __syncthreads();
    }
    unsigned long long* go = a.out + (int64_t)p0 * B * B;
    for (int i = tid; i < np * B * B; i += kHistThreads) {
        const uint32_t n = lc[i];
        if (n) atomicAdd(&go[i], (unsigned long long)n);
    }
}

}  // namespace kmc_hist
