// Kernel instantiations for the LogNormal log-density, PART 0 (kmc_tables.hpp):
// double rows of exact size on one GPU and the generic kernel; the log-pdf and initial-ball kernels.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(LogNormal, 0);
KMC_INSTANTIATE_ROWS(LogNormal);
}  // namespace kmc
