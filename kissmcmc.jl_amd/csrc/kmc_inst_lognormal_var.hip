// Kernel instantiations for the LogNormal log-density, PART 1 (kmc_tables.hpp):
// ragged row sizes and KMC_F32 rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(LogNormal, 1);
}  // namespace kmc
