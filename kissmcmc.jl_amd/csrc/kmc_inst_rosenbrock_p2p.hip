// Kernel instantiations for the chained Rosenbrock (test/runtests.jl:68 at N = 2) log-density, PART 2 (kmc_tables.hpp):
// the peer-to-peer kernels (KMC_P2P).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(Rosenbrock, 2);
}  // namespace kmc
