"""kissmcmc.jl_amd -- MI355X-native emcee (affine-invariant ensemble sampler) hot path.

A from-scratch HIP/gfx950 implementation of the one data-parallel path of mauro3/KissMCMC.jl:
``emcee`` / ``_emcee`` (reference ``src/samplers.jl:188-293``), behind the reference's own call
surface (``emcee``, ``make_theta0s``, ``squash_walkers``).  Import as ``kissmcmc_jl_amd``.

The compute path is ``libkissmcmc_hip.so`` (C ABI: ``include/kissmcmc_hip.h``); there is no CPU
fallback -- without the library or a HIP device the sampler raises.
"""
from . import _lib
from ._lib import KmcError
from .api import emcee, emcee_counts, make_theta0s, squash_walkers
from .densities import (CDensity, DataDensity, DeviceLogPdf, Exponential, ExprDensity, GaussianIso, HostLogPdf, LogNormal, MvNormal2,
                        Rosenbrock, check_grad, grad)
from .chain_convergence import convergence, convergence_stats, error_of_estimated_mean, evaluate_convergence, lag_sums, samples_vs_tau
from .chain_convergence import normal_scores, rank_convergence, rank_plan, rank_scores
from .chain_convergence import beta_quantile, indicator_lags, indicator_moments, indicator_plan, quantile_mcse, quantile_mcse_ranks
from .chain_covariance import correlation, cov_plan, covariance
from .chain_predictive import compare_waic, pointwise_loglike, pointwise_plan, pointwise_stats, waic, waic_stats
from .chain_loo import compare_loo, loo, loo_stats, pointwise_weights, psis_plan, psis_smooth, psis_tail, relative_eff
from .diagnostics import eff_samples, int_acorr
from .moves import DEMove, DESnookerMove
from .metropolis import GaussianStep, HMCStep, HostProposal, MVNormalStep, TunedStep, cholesky_lower, metropolis, metropolis_chains
from .sampler import Sampler
from .summary import corner, credible_levels, hdi, hdi_span, hist_mode, histogram, map_sample, quantile_ranks, quantiles, summarize_run
from .tempering import geometric_betas, thermodynamic_integration

__all__ = [
    "emcee", "make_theta0s", "squash_walkers", "emcee_counts", "Sampler", "KmcError",
    "DeviceLogPdf", "GaussianIso", "Exponential", "Rosenbrock", "LogNormal", "MvNormal2", "ExprDensity", "CDensity", "DataDensity", "HostLogPdf",
    "DEMove", "DESnookerMove", "geometric_betas", "thermodynamic_integration", "cdf_g_inv", "g_pdf", "metropolis", "metropolis_chains", "GaussianStep", "HostProposal", "MVNormalStep", "TunedStep", "HMCStep", "grad", "check_grad", "cholesky_lower", "int_acorr", "eff_samples",
    "quantiles", "quantile_ranks", "map_sample", "summarize_run", "histogram", "corner", "hist_mode", "credible_levels",
    "convergence", "convergence_stats", "lag_sums", "evaluate_convergence", "error_of_estimated_mean", "samples_vs_tau",
    "rank_convergence", "rank_scores", "rank_plan", "normal_scores",
    "quantile_mcse", "indicator_lags", "beta_quantile", "quantile_mcse_ranks", "indicator_moments", "indicator_plan",
    "hdi", "hdi_span",
    "covariance", "correlation", "cov_plan",
    "waic", "pointwise_loglike", "pointwise_stats", "compare_waic", "waic_stats", "pointwise_plan",
    "loo", "compare_loo", "psis_plan", "loo_stats", "psis_smooth", "psis_tail", "relative_eff", "pointwise_weights",
]


def g_pdf(z: float, a: float) -> float:
    """Stretch-factor density, reference ``src/samplers.jl:224``."""
    return _lib.lib().kmc_g_pdf(float(z), float(a))


def cdf_g_inv(u: float, a: float) -> float:
    """Inverse CDF of ``g``, reference ``src/samplers.jl:227``."""
    return _lib.lib().kmc_cdf_g_inv(float(u), float(a))
