// Kernel instantiations for the exponential log-density with the differential-evolution move (KMC_MOVE_DE, opt-in):
// the vector kernels (exact and ragged rows) and the generic kernel, double rows on one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
void table_de_exponential(int L, int K, int iter, bool ragged, HalfStepFn* vec, HalfStepFn* gen) { density_part<Exponential, 3>(L, K, iter, ragged, false, vec, gen); }
}  // namespace kmc
