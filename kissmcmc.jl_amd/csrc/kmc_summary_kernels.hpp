// kmc_summary_kernels.hpp -- device kernels of the posterior summaries (kmc_summary.hip): order statistics of a stored chain by
// most-significant-digit radix select, and the arg-max of the stored log-densities.  Internal.
//
// A double maps to a 64-bit key whose unsigned order is the value order (kmc_chain_kernels.hpp: chain_key).  The select
// walks the key from its top byte down, kSelectPasses passes of kSelectBits bits.  Every (column, rank) pair is a SLOT with a prefix
// (the digits found so far) and a residual rank; a pass counts, per slot, the next digit of the elements whose higher digits equal the
// slot's prefix (select_hist), and one small workgroup per slot then finds the digit at which the cumulative count crosses the residual
// rank (select_scan).  Counts are integers: 32-bit LDS atomics per workgroup, flushed by 64-bit integer atomic adds -- the result does
// not depend on the launch geometry or on the order in which workgroups arrive.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kmc_chain_kernels.hpp"

namespace kmc_summary {

using namespace kmc_chain;

constexpr int kSelectBits = 8;                          // digit width: 256 bins, 1 KiB of 32-bit LDS counters per slot
constexpr int kSelectBins = 1 << kSelectBits;
constexpr int kSelectPasses = 64 / kSelectBits;
constexpr int kSelectSlots = 64;                        // slots of one workgroup: 64 KiB of LDS at most
constexpr int kSelectUnroll = 8;                        // loads a thread has in flight
constexpr int kMaxRanks = 16;

// The columns of the chain are cut into groups of 1 << cg_shift (a power of two, so that a group's piece of every row starts on a
// 64-byte boundary when it is 8 doubles or more); the log-densities are one more group of one column, number ndim.  Workgroup
// blockIdx.x = group * nwg + b reads the rows b, b + nwg, ... (256 >> shift rows of its group's columns at a time), so that the lanes of
// a wave read consecutive addresses along the row.
struct SelectArgs {
    const void* chain;                 // [sample][walker][ld], float or double
    const double* logp;                // [sample][walker] or nullptr
    const uint8_t* mask;               // [nl] or nullptr: walkers that count
    const uint64_t* prefix;            // [slots] key digits found so far (zero below them)
    unsigned long long* hist;          // [slots][kSelectBins], zero at launch
    int64_t row0, nrows, nl, ld;       // rows [row0, row0 + nrows) of the chain, row = sample * nl + walker
    int32_t ndim, is_float, nranks, cg_shift, ngroups_chain, pass, nwg;
};

__global__ __launch_bounds__(256) void select_hist(SelectArgs a)
{
    extern __shared__ uint32_t lh[];                   // [ncol * nranks][kSelectBins]
    const int tid = (int)threadIdx.x;
    const int g = (int)(blockIdx.x / (unsigned)a.nwg), b = (int)(blockIdx.x - (unsigned)g * (unsigned)a.nwg);
    const bool is_lp = g >= a.ngroups_chain;
    const int sh = is_lp ? 0 : a.cg_shift;
    const int c0 = is_lp ? a.ndim : (g << sh);
    const int ncol = is_lp ? 1 : ((a.ndim - c0) < (1 << sh) ? (a.ndim - c0) : (1 << sh));
    const int nslot = ncol * a.nranks;                  // <= kSelectSlots by the choice of cg_shift
    for (int i = tid; i < nslot * kSelectBins; i += 256) lh[i] = 0u;
    __syncthreads();

    const int c = tid & ((1 << sh) - 1), rsub = tid >> sh;
    const int64_t rp = 256 >> sh;                       // rows per step of this workgroup
    const int64_t nsteps = (a.nrows + rp - 1) / rp;
    const bool col_ok = c < ncol;
    const int dshift = 64 - kSelectBits * (a.pass + 1);
    const bool small_rows = a.nrows <= 0xffffffffll;
    uint64_t phi[kMaxRanks];                            // a thread keeps one column: the higher digits of its slots' prefixes, in registers
#pragma unroll
    for (int r = 0; r < kMaxRanks; ++r)
        phi[r] = (a.pass > 0 && col_ok && r < a.nranks) ? a.prefix[(int64_t)(c0 + c) * a.nranks + r] >> (dshift + kSelectBits) : 0ull;
    for (int64_t it = b; it < nsteps; it += (int64_t)a.nwg * kSelectUnroll) {
        uint64_t key[kSelectUnroll];
        bool ok[kSelectUnroll];
#pragma unroll
        for (int u = 0; u < kSelectUnroll; ++u) {
            const int64_t step = it + (int64_t)u * a.nwg;
            const int64_t row = step * rp + rsub;
            ok[u] = col_ok && step < nsteps && row < a.nrows;
            if (ok[u] && a.mask) {
                const int64_t w = small_rows ? (int64_t)((uint32_t)row % (uint32_t)a.nl) : row % a.nl;
                ok[u] = a.mask[w] != 0;
            }
            double v = 0.0;
            if (ok[u]) {
                const int64_t r = a.row0 + row;
                if (is_lp) v = a.logp[r];
                else if (a.is_float) v = (double)reinterpret_cast<const float*>(a.chain)[r * a.ld + c0 + c];   // exact
                else v = reinterpret_cast<const double*>(a.chain)[r * a.ld + c0 + c];
            }
            key[u] = chain_key((uint64_t)__double_as_longlong(v));
        }
#pragma unroll
        for (int u = 0; u < kSelectUnroll; ++u) {
            if (!ok[u]) continue;
            const uint32_t digit = (uint32_t)(key[u] >> dshift) & (kSelectBins - 1);
            if (a.pass == 0) {                          // no prefix yet: the ranks of a column share one histogram, kept in its first slot
                atomicAdd(&lh[(c * a.nranks) * kSelectBins + digit], 1u);
            } else {
                const uint64_t hi = key[u] >> (dshift + kSelectBits);
#pragma unroll
                for (int r = 0; r < kMaxRanks; ++r)
                    if (r < a.nranks && phi[r] == hi) atomicAdd(&lh[(c * a.nranks + r) * kSelectBins + digit], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* gh = a.hist + (int64_t)c0 * a.nranks * kSelectBins;
    for (int i = tid; i < nslot * kSelectBins; i += 256) {
        const uint32_t n = lh[i];
        if (n) atomicAdd(&gh[i], (unsigned long long)n);
    }
}

// One workgroup per slot: the digit d with  sum_{j<d} count_j <= k < sum_{j<=d} count_j  joins the prefix, k loses the elements below it.
// After the last pass the prefix is the key of the element of rank k; out gets its bits back as a double.
__global__ __launch_bounds__(kSelectBins) void select_scan(const unsigned long long* hist, uint64_t* prefix, int64_t* krem, double* out, int nranks, int pass)
{
    __shared__ unsigned long long cum[kSelectBins];
    const int t = (int)threadIdx.x;
    const int64_t slot = blockIdx.x;
    const int64_t src = pass == 0 ? slot - slot % nranks : slot;      // pass 0: the column's shared histogram
    const unsigned long long n = hist[src * kSelectBins + t];
    cum[t] = n;
    __syncthreads();
    for (int off = 1; off < kSelectBins; off <<= 1) {
        const unsigned long long add = t >= off ? cum[t - off] : 0ull;
        __syncthreads();
        cum[t] += add;
        __syncthreads();
    }
    const unsigned long long k = (unsigned long long)krem[slot], incl = cum[t], excl = incl - n;
    if (excl <= k && k < incl) {                        // exactly one bin: 0 <= k < the count of the elements under the prefix
        const uint64_t p = prefix[slot] | ((uint64_t)t << (64 - kSelectBits * (pass + 1)));
        prefix[slot] = p;
        krem[slot] = (int64_t)(k - excl);
        if (pass == kSelectPasses - 1) out[slot] = __longlong_as_double((long long)chain_unkey(p));
    }
}

// ---- arg-max of the stored log-densities: the largest value, ties to the smallest row index (= smallest sample, then walker), NaN ignored ----
__device__ inline bool argmax_better(double av, int64_t ai, double bv, int64_t bi)     // is (av, ai) ahead of (bv, bi)?  index -1: nothing yet
{
    if (ai < 0) return false;
    if (bi < 0) return true;
    return av > bv || (av == bv && ai < bi);
}

__device__ inline void argmax_block(double& v, int64_t& i, double* sv, int64_t* si)
{
    const int t = (int)threadIdx.x;
    sv[t] = v; si[t] = i;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off && argmax_better(sv[t + off], si[t + off], sv[t], si[t])) { sv[t] = sv[t + off]; si[t] = si[t + off]; }
        __syncthreads();
    }
    v = sv[0]; i = si[0];
}

// stage 1: every workgroup's best of the rows [row0, row0 + nrows) it strides over -> pv / pi [gridDim.x]
__global__ __launch_bounds__(256) void argmax_partial(const double* logp, const uint8_t* mask, int64_t row0, int64_t nrows, int64_t nl, double* pv, int64_t* pi)
{
    __shared__ double sv[256];
    __shared__ int64_t si[256];
    double bv = 0.0;
    int64_t bi = -1;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * 256) {
        if (mask && !mask[r % nl]) continue;
        const double v = logp[row0 + r];
        if (v != v) continue;
        if (argmax_better(v, row0 + r, bv, bi)) { bv = v; bi = row0 + r; }
    }
    argmax_block(bv, bi, sv, si);
    if (threadIdx.x == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// stage 2 (one workgroup): the best of the partial results, then that sample's row widened to double without its pad.
// res: [ndim] row, [ndim] its log-density, [ndim + 1] the row index as an integer's bits (-1: every selected entry was NaN)
__global__ __launch_bounds__(256) void argmax_final(const double* pv, const int64_t* pi, int np, const void* chain, int is_float, int64_t ld, int ndim, double* res)
{
    __shared__ double sv[256];
    __shared__ int64_t si[256];
    double bv = 0.0;
    int64_t bi = -1;
    for (int j = (int)threadIdx.x; j < np; j += 256)
        if (argmax_better(pv[j], pi[j], bv, bi)) { bv = pv[j]; bi = pi[j]; }
    argmax_block(bv, bi, sv, si);
    if (threadIdx.x == 0) { res[ndim] = bv; res[ndim + 1] = __longlong_as_double((long long)bi); }
    if (bi < 0) return;
    for (int d = (int)threadIdx.x; d < ndim; d += 256)
        res[d] = is_float ? (double)reinterpret_cast<const float*>(chain)[bi * ld + d] : reinterpret_cast<const double*>(chain)[bi * ld + d];
}

}  // namespace kmc_summary
