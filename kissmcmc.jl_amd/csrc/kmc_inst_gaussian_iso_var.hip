// Kernel instantiations for the isotropic Gaussian log-density, PART 1 (kmc_tables.hpp):
// ragged row sizes and KMC_F32 rows, one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(GaussianIso, 1);
}  // namespace kmc

#ifdef KMC_PROBE   // diagnostic build only (scripts/probe_timeline.py R31 ...): the stamps of THIS translation unit's kernels (ragged rows)
extern "C" __attribute__((visibility("default"))) int kmc_probe_read_var(void* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kmc::g_probe), sizeof(kmc::g_probe));
}
#endif
