// kmc_rank_host.hpp -- what the host side of the rank statistics (kmc_rank.hip) shares with the read-outs that need its sorted columns
// (kmc_hdi.hip): the work space of the segmented radix sort, its limits and room, the gather of the selection's keys and the sort
// itself.  The kernels stay in kmc_rank_kernels.hpp, which kmc_rank.hip alone includes.  Internal.
#pragma once
#include <cstdint>
#include <vector>

#include "kmc_convergence_host.hpp"

namespace kmc_rank_host {

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_conv_host;

struct RankBuffers {
    uint64_t *key_a = nullptr, *key_b = nullptr, *picked = nullptr;
    uint32_t* counts = nullptr;
    unsigned long long* nan = nullptr;
    double *centre = nullptr, *out_z = nullptr;
    int64_t* out_rank2 = nullptr;
    ~RankBuffers()
    {
        (void)hipFree(key_a); (void)hipFree(key_b); (void)hipFree(picked); (void)hipFree(counts); (void)hipFree(nan); (void)hipFree(centre);
        (void)hipFree(out_z); (void)hipFree(out_rank2);
    }
};

// the sizes one call may have, from the shape alone
kmc_status rank_limits(const ConvShape& sh, int64_t ncols);
// The work space: two key buffers (16 B), the digit counts, and 8 B per transformed column (or 16 B for rank2 and z), per pooled draw;
// `extra`: bytes the caller takes besides.
kmc_status rank_room(const ConvShape& sh, int64_t ncols, int transformed, bool outputs, double extra = 0.0);
kmc_status rank_alloc(RankBuffers& rb, int64_t ncols, int64_t S, bool outputs);
// keys of the (folded) selection into key_a; nan[c]: the NaNs among them
kmc_status gather(RankBuffers& rb, const ConvBuffers& b, const ChainView& v, const ConvShape& sh, bool with_logp, bool folded, hipStream_t st,
                  std::vector<int64_t>* nan);
// key_a sorted, every column on its own: the result is in key_a again
kmc_status sort_columns(RankBuffers& rb, int64_t ncols, int64_t S, hipStream_t st);
// the value of a key
double unkey(uint64_t key);

}  // namespace kmc_rank_host
