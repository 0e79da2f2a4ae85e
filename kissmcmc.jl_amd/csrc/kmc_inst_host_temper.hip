// Kernel instantiations for the host-evaluated density, parallel tempering (kmc_tables.hpp: temper_part): the tempered generic
// kernels of the stretch and differential-evolution moves.  With HostEval the tempered body is LIKELIHOOD tempering of a data density
// (KMC_TEMPER_LIKELIHOOD): a PROPOSE pass for every rung, and an ACCEPT pass that reads each proposal's tree sum and prior.
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(HostEval, Move::Stretch);
KMC_INSTANTIATE_TEMPER(HostEval, Move::DE);
}  // namespace kmc
