// Kernel instantiations for the LogNormal log-density, PART 3 (kmc_tables.hpp):
// the differential-evolution move (KMC_MOVE_DE, opt-in): vector (exact and ragged rows) and generic kernels, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(LogNormal, 3);
}  // namespace kmc
