// Kernel instantiations for the isotropic Gaussian log-density, PART 0 (kmc_tables.hpp):
// double rows of exact size on one GPU and the generic kernel; the log-pdf and initial-ball kernels.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(GaussianIso, 0);
KMC_INSTANTIATE_ROWS(GaussianIso);
}  // namespace kmc

#ifdef KMC_PROBE   // diagnostic build only (scripts/probe_timeline.py): the stamps of THIS translation unit's kernels (part 0)
extern "C" __attribute__((visibility("default"))) int kmc_probe_read(void* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kmc::g_probe), sizeof(kmc::g_probe));
}
#endif
