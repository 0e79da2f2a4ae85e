// Kernel instantiations for the chained Rosenbrock log-density, parallel tempering (kmc_tables.hpp: temper_part):
// the tempered stretch and differential-evolution kernels -- vector (exact and ragged rows) and generic, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(Rosenbrock, Move::Stretch);
KMC_INSTANTIATE_TEMPER(Rosenbrock, Move::DE);
}  // namespace kmc
