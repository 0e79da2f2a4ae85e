// Kernel instantiations for the chained Rosenbrock (test/runtests.jl:68 at N = 2) log-density, PART 1 (kmc_tables.hpp):
// ragged row sizes and KMC_F32 rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(Rosenbrock, 1);
}  // namespace kmc
