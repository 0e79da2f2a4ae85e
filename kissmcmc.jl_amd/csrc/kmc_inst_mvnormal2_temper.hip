// Kernel instantiations for the 2-D correlated normal log-density, parallel tempering (kmc_tables.hpp: temper_part):
// the tempered stretch and differential-evolution kernels -- vector (exact and ragged rows) and generic, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(MvNormal2, Move::Stretch);
KMC_INSTANTIATE_TEMPER(MvNormal2, Move::DE);
}  // namespace kmc
