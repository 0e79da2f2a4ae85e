// kmc_chain_kernels.hpp -- what the device kernels that read a stored chain where it lies share (kmc_summary_kernels.hpp,
// kmc_hist_kernels.hpp, kmc_convergence_kernels.hpp, kmc_rank_kernels.hpp, kmc_hdi_kernels.hpp): the load of one element, the key whose unsigned order is the
// value order, and the decode of a position of a row for the kernels that select walkers by a rank table.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kmc_chain {

// Element `at` of a chain of floats or doubles, widened (exact).  select_hist, argmax_final and hist1d write the same expression out, the
// index repeated in both arms: from one index value shared by the arms the compiler forms their addresses another way (a vector add where
// a scalar row base served), and a read-out kernel's code changes only with a measurement.
__device__ inline double chain_load(const void* src, int is_float, int64_t at)
{
    return is_float ? (double)reinterpret_cast<const float*>(src)[at] : reinterpret_cast<const double*>(src)[at];
}

// The bits of a double as a 64-bit key that compares as an unsigned integer in value order: all bits flipped when the sign bit is set,
// else the sign bit flipped;  -inf < ... < -0.0 < +0.0 < ... < +inf, NaNs by bit pattern beyond the infinities of their sign.
__host__ __device__ inline uint64_t chain_key(uint64_t bits) { return (bits >> 63) ? ~bits : (bits ^ 0x8000000000000000ull); }
__host__ __device__ inline uint64_t chain_unkey(uint64_t key) { return (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key; }

// Position p = walker * ld + column of a row [nl][ld] of np elements, with rank[walker] the walker's index among the selected ones
// (-1: not selected).  What the lane at p reads: nothing (false) for a walker outside the selection or a padding column (column >= ndim)
// -- chain_lane_in_row, for a p known to lie in the row -- or a position past the row (chain_lane).
__device__ inline bool chain_lane_in_row(const int32_t* rank, int64_t p, int64_t ld, int32_t ndim, int64_t* walker, int32_t* col)
{
    const int64_t w = p / ld;
    const int32_t c = (int32_t)(p - w * ld);
    *walker = w;
    *col = c;
    return c < ndim && rank[w] >= 0;
}

__device__ inline bool chain_lane(const int32_t* rank, int64_t p, int64_t np, int64_t ld, int32_t ndim, int64_t* walker, int32_t* col)
{
    return p < np && chain_lane_in_row(rank, p, ld, ndim, walker, col);
}

}  // namespace kmc_chain
