// Kernel instantiations for the 2-D correlated normal log-density, parallel tempering (kmc_tables.hpp: temper_part):
// the tempered snooker and mixture kernels -- vector (exact and ragged rows) and generic, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(MvNormal2, Move::Snooker);
KMC_INSTANTIATE_TEMPER(MvNormal2, Move::Mix);
}  // namespace kmc
