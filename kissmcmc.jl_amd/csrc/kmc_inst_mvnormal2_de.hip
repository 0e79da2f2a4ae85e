// Kernel instantiations for the bivariate normal log-density with the differential-evolution move (KMC_MOVE_DE, opt-in):
// the vector kernels (exact and ragged rows) and the generic kernel, double rows on one GPU.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
void table_de_mvnormal2(int L, int K, int iter, bool ragged, HalfStepFn* vec, HalfStepFn* gen) { density_part<MvNormal2, 3>(L, K, iter, ragged, false, vec, gen); }
}  // namespace kmc
