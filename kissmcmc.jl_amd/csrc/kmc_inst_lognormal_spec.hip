// Kernel instantiations for the log-normal log-density: the phase-specialised instance of PART 0's vector kernels
// (kmc_tables.hpp: spec_part; kmc_kernels.hpp: Spec).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_SPEC(LogNormal);
}  // namespace kmc
