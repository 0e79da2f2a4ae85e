// Kernel instantiations for the isotropic Gaussian log-density:
// the LDS-resident (islands, resident mode), one-launch-per-generation and many-chain Metropolis kernels (kmc_tables.hpp).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_LDS(GaussianIso);
}  // namespace kmc

#ifdef KMC_PROBE   // diagnostic build only (scripts/probe_generation.py): the stamps of THIS translation unit's kernels (generation_lane)
extern "C" __attribute__((visibility("default"))) int kmc_probe_read_generation(void* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kmc::g_probe), sizeof(kmc::g_probe));
}
#endif
