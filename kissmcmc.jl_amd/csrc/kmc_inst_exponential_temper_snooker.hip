// Kernel instantiations for the exponential log-density, parallel tempering (kmc_tables.hpp: temper_part):
// the tempered snooker and mixture kernels -- vector (exact and ragged rows) and generic, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(Exponential, Move::Snooker);
KMC_INSTANTIATE_TEMPER(Exponential, Move::Mix);
}  // namespace kmc
