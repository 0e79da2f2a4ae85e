// Kernel instantiations for the LogNormal log-density:
// the LDS-resident (islands, resident mode), one-launch-per-generation and many-chain Metropolis kernels (kmc_tables.hpp).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_LDS(LogNormal);
}  // namespace kmc
