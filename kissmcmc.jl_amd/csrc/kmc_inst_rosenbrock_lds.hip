// Kernel instantiations for the chained Rosenbrock (test/runtests.jl:68 at N = 2) log-density:
// the LDS-resident (islands, resident mode), one-launch-per-generation and many-chain Metropolis kernels (kmc_tables.hpp).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_LDS(Rosenbrock);
}  // namespace kmc

#ifdef KMC_PROBE   // diagnostic build only (scripts/probe_timeline.py C3): the stamps of THIS translation unit's kernels (generation_group)
extern "C" __attribute__((visibility("default"))) int kmc_probe_read_generation_rosenbrock(void* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kmc::g_probe), sizeof(kmc::g_probe));
}
#endif
