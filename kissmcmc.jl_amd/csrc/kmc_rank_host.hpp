// kmc_rank_host.hpp -- the sorted columns of a session's selection as a service: what the host side of the rank statistics (kmc_rank.hip)
// shares with the read-outs that need its sort (kmc_hdi.hip, kmc_quantile.hip).  One call makes room, allocates, gathers the selection's
// keys and sorts every column (the segmented radix sort of DESIGN.md section 4h); after it, order statistics are picked at a list of
// positions and quantiles are read off by the one rule of the library.  The kernels stay in kmc_rank_kernels.hpp, which kmc_rank.hip
// alone includes.  Internal.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "kmc_convergence_host.hpp"

namespace kmc_rank_host {

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_conv_host;

// the sizes one call may have, from the shape alone
kmc_status rank_limits(const ConvShape& sh, int64_t ncols);
// the value of a key
double unkey(uint64_t key);

// The quantile q among S sorted draws by the rule of the order statistics (kmc.quantile_ranks with N = S): h = q (S - 1), lo = floor(h),
// hi = min(lo + 1, S - 1), frac = h - lo, x_lo + frac (x_hi - x_lo), and x_lo itself where frac == 0 (so that an infinite neighbour
// does not make a NaN of it).
struct QuantileAt {
    int64_t lo, hi;
    double frac;
    QuantileAt(double q, int64_t S)
    {
        const double hq = q * (double)(S - 1), fl = std::floor(hq);
        lo = (int64_t)fl; hi = lo + 1 < S - 1 ? lo + 1 : S - 1; frac = hq - fl;
    }
    double between(double x_lo, double x_hi) const { return frac == 0.0 ? x_lo : x_lo + frac * (x_hi - x_lo); }
};

// The sorted columns of one session, on its stream, and the device buffers of the sort.  It must die BEFORE its session -- declared
// after it, or in a scope of its own inside a stage: the destructor drains the session's stream, which must still exist, before the keys go.
struct SortedColumns {
    uint64_t *key_a = nullptr, *key_b = nullptr, *picked = nullptr;              // the sorted keys are key_a [ncols][S]
    uint32_t* counts = nullptr;
    unsigned long long* nan_dev = nullptr;
    double *centre = nullptr, *out_z = nullptr;
    int64_t *out_rank2 = nullptr, *pos_dev = nullptr;
    size_t npos = 0;                   // positions pos_dev and picked hold
    int64_t ncols = 0, S = 0;
    hipStream_t st = nullptr;
    std::vector<int64_t> nan;          // [ncols]: the NaNs among the keys of the last gather; such a column has no order statistics
    ~SortedColumns()
    {
        if (st) (void)hipStreamSynchronize(st);
        for (void* p : {(void*)key_a, (void*)key_b, (void*)picked, (void*)counts, (void*)nan_dev, (void*)centre, (void*)out_z, (void*)out_rank2, (void*)pos_dev})
            (void)hipFree(p);
    }

    // Room, allocation, gather and sort of the opened session's selection.  The room: two key buffers (16 B) and the digit counts, 8 B per
    // transformed column (or, with `outputs`, 16 B for rank2 and z) per pooled draw, and `extra` bytes the caller takes besides.
    // `marks`: three events recorded before the gather, between gather and sort, and after the sort.
    kmc_status sort(const ConvSession& ses, int transformed, bool outputs, double extra = 0.0, const hipEvent_t* marks = nullptr);
    // ... once more, of |x - centre| about centre [ncols]
    kmc_status sort_folded(const ConvSession& ses);
    // out[e] = the key at pos[e] = c S + index of the sorted columns; every position is checked against the buffer here, on the host
    kmc_status pick_at(const std::vector<int64_t>& pos, std::vector<uint64_t>* out);
    // out[k * ncols + c] = the quantile q[k] of column c (QuantileAt), NaN for a column that holds one
    kmc_status quantiles(const double* q, int nq, double* out);
};

}  // namespace kmc_rank_host
