// Kernel instantiations for the isotropic Gaussian log-density, parallel tempering (kmc_tables.hpp: temper_part):
// the tempered stretch and differential-evolution kernels -- vector (exact and ragged rows) and generic, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(GaussianIso, Move::Stretch);
KMC_INSTANTIATE_TEMPER(GaussianIso, Move::DE);
}  // namespace kmc
