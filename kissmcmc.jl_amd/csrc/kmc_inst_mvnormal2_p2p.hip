// Kernel instantiations for the 2-D correlated normal (test/runtests.jl:60) log-density, PART 2 (kmc_tables.hpp):
// the peer-to-peer kernels (KMC_P2P).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(MvNormal2, 2);
}  // namespace kmc
