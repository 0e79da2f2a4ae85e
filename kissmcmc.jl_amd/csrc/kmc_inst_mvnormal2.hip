// Kernel instantiations for the 2-D correlated normal (test/runtests.jl:60) log-density, PART 0 (kmc_tables.hpp):
// double rows of exact size on one GPU and the generic kernel; the log-pdf and initial-ball kernels.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(MvNormal2, 0);
KMC_INSTANTIATE_ROWS(MvNormal2);
}  // namespace kmc
