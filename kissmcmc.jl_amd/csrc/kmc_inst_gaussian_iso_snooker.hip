// Kernel instantiations for the isotropic Gaussian log-density, PART 4 and 5 (kmc_tables.hpp):
// the snooker move (KMC_MOVE_SNOOKER) and the DE / snooker mixtures (KMC_MOVE_MIX), both opt-in: vector (exact and ragged rows) and generic kernels, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(GaussianIso, 4);
KMC_INSTANTIATE_PART(GaussianIso, 5);
}  // namespace kmc
