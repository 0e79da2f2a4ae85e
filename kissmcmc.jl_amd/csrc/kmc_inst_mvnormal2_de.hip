// Kernel instantiations for the 2-D correlated normal (test/runtests.jl:60) log-density, PART 3 (kmc_tables.hpp):
// the differential-evolution move (KMC_MOVE_DE, opt-in): vector (exact and ragged rows) and generic kernels, double rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(MvNormal2, 3);
}  // namespace kmc
