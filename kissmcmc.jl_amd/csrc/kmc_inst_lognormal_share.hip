// Kernel instantiations for the log-normal log-density: the workgroup-shared-draws instances of PART 0's vector kernels
// (kmc_tables.hpp: share_part; kmc_shared_draws.hpp).
#define KMC_TABLES_IMPL
#include "kmc_shared_draws.hpp"

namespace kmc {
KMC_INSTANTIATE_SHARE(LogNormal);
}  // namespace kmc
