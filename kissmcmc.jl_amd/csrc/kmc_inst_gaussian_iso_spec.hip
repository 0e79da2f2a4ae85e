// Kernel instantiations for the isotropic Gaussian log-density: the phase-specialised instance of PART 0's vector kernels
// (kmc_tables.hpp: spec_part; kmc_kernels.hpp: Spec).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_SPEC(GaussianIso);
}  // namespace kmc

#ifdef KMC_PROBE   // diagnostic build only (scripts/probe_timeline.py): the stamps of THIS translation unit's kernels (the credit instance)
extern "C" __attribute__((visibility("default"))) int kmc_probe_read_spec(void* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kmc::g_probe), sizeof(kmc::g_probe));
}
#endif
