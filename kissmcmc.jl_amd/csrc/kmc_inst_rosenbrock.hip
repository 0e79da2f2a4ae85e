// Kernel instantiations for the chained Rosenbrock (test/runtests.jl:68 at N = 2) log-density, PART 0 (kmc_tables.hpp):
// double rows of exact size on one GPU and the generic kernel; the log-pdf and initial-ball kernels.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_PART(Rosenbrock, 0);
KMC_INSTANTIATE_ROWS(Rosenbrock);
}  // namespace kmc

#ifdef KMC_PROBE   // diagnostic build only (scripts/probe_timeline.py C3): this translation unit's copy of the stamps
extern "C" __attribute__((visibility("default"))) int kmc_probe_read_rosenbrock(void* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kmc::g_probe), sizeof(kmc::g_probe));
}
#endif
