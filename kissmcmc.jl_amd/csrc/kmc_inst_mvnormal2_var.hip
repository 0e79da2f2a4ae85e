// Kernel instantiations for the 2-D correlated normal (test/runtests.jl:60) log-density, PART 1 (kmc_tables.hpp):
// ragged row sizes and KMC_F32 rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(MvNormal2, 1);
}  // namespace kmc
