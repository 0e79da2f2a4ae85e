// Kernel instantiations for the isotropic Gaussian log-density: the workgroup-shared-draws instances of PART 0's vector kernels
// (kmc_tables.hpp: share_part; kmc_shared_draws.hpp).
#define KMC_TABLES_IMPL
#include "kmc_shared_draws.hpp"

namespace kmc {
KMC_INSTANTIATE_SHARE(GaussianIso);
}  // namespace kmc

#ifdef KMC_PROBE   // diagnostic build only (scripts/probe_timeline.py): the stamps of THIS translation unit's kernels (the shared-draws instances)
extern "C" __attribute__((visibility("default"))) int kmc_probe_read_share(void* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kmc::g_probe), sizeof(kmc::g_probe));
}
#endif
