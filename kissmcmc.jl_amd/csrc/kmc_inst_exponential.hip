// Kernel instantiations for the exponential (README.md:15) log-density, PART 0 (kmc_tables.hpp):
// double rows of exact size on one GPU and the generic kernel; the log-pdf and initial-ball kernels.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(Exponential, 0);
KMC_INSTANTIATE_ROWS(Exponential);
}  // namespace kmc
