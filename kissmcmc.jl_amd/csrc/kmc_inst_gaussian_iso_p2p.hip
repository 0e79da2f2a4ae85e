// Kernel instantiations for the isotropic Gaussian log-density, PART 2 (kmc_tables.hpp):
// the peer-to-peer kernels (KMC_P2P).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(GaussianIso, 2);
}  // namespace kmc
