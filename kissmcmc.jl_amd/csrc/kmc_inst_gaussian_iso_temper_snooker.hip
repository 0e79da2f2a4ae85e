// Kernel instantiations for the isotropic Gaussian log-density, parallel tempering (kmc_tables.hpp: temper_part):
// the tempered snooker and mixture kernels -- vector (exact and ragged rows) and generic, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(GaussianIso, Move::Snooker);
KMC_INSTANTIATE_TEMPER(GaussianIso, Move::Mix);
}  // namespace kmc
