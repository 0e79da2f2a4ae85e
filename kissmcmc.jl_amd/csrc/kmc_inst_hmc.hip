// Kernel instantiations of the HMC step (kmc_hmc.hpp) for the menu densities: the six register geometries of every density (MvNormal2:
// two dimensions only; Rosenbrock: from two dimensions on), and the gradient-of-rows kernels of kmc_grad_eval_host.
#include <type_traits>
#include "../../include/kissmcmc_hip.h"
#include "kmc_hmc.hpp"

namespace kmc {
namespace {

template <class D, int ND>
constexpr bool hmc_geometry_exists()
{
    if (std::is_same<D, MvNormal2>::value) return ND == 2;
    if (std::is_same<D, Rosenbrock>::value) return ND >= 2;
    return true;
}

template <class D, int ND>
void hmc_pick(HmcFn* h, GradFn* g)
{
    if constexpr (hmc_geometry_exists<D, ND>()) {
        *h = metropolis_hmc<D, ND>;
        *g = grad_rows<D, ND>;
    }
}

template <class D>
void hmc_kernels(int ndim, HmcFn* h, GradFn* g)
{
    if (ndim <= 1) hmc_pick<D, 1>(h, g);
    else if (ndim <= 2) hmc_pick<D, 2>(h, g);
    else if (ndim <= 4) hmc_pick<D, 4>(h, g);
    else if (ndim <= 8) hmc_pick<D, 8>(h, g);
    else if (ndim <= 16) hmc_pick<D, 16>(h, g);
    else if (ndim <= 32) hmc_pick<D, 32>(h, g);
}

void hmc_kernels_of(int density, int ndim, HmcFn* h, GradFn* g)
{
    *h = nullptr;
    *g = nullptr;
    if (ndim < 1 || ndim > 32) return;
    switch (density) {
    case KMC_GAUSSIAN_ISO: hmc_kernels<GaussianIso>(ndim, h, g); break;
    case KMC_EXPONENTIAL: hmc_kernels<Exponential>(ndim, h, g); break;
    case KMC_ROSENBROCK: hmc_kernels<Rosenbrock>(ndim, h, g); break;
    case KMC_LOGNORMAL: hmc_kernels<LogNormal>(ndim, h, g); break;
    case KMC_MVNORMAL2: hmc_kernels<MvNormal2>(ndim, h, g); break;
    default: break;
    }
}

}  // namespace

HmcFn hmc_lookup(int density, int ndim)
{
    HmcFn h;
    GradFn g;
    hmc_kernels_of(density, ndim, &h, &g);
    return h;
}

GradFn grad_lookup(int density, int ndim)
{
    HmcFn h;
    GradFn g;
    hmc_kernels_of(density, ndim, &h, &g);
    return g;
}

}  // namespace kmc
