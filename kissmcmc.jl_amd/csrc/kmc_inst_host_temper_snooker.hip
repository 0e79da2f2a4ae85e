// Kernel instantiations for the host-evaluated density, parallel tempering (kmc_tables.hpp: temper_part): the tempered generic
// kernels of the snooker move and the mixtures (likelihood tempering of a data density, see kmc_inst_host_temper.hip).
#define KMC_TABLES_IMPL
#include "kmc_tables.hpp"

namespace kmc {
KMC_INSTANTIATE_TEMPER(HostEval, Move::Snooker);
KMC_INSTANTIATE_TEMPER(HostEval, Move::Mix);
}  // namespace kmc
