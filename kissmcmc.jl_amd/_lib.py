"""ctypes binding of ``libkissmcmc_hip.so`` (the C ABI in ``include/kissmcmc_hip.h``).

There is no CPU fallback: if the library is missing, or no HIP device is visible when a sampler
is created, this fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KMC_LIB_PATH selects an experiment build of the same library (see build.py); default in-tree.
LIB_PATH = os.environ.get("KMC_LIB_PATH") or os.path.join(_HERE, "libkissmcmc_hip.so")

# kmc_status
OK, ERR_A_SCALE, ERR_ODD_WALKERS, ERR_TOO_FEW_WALKERS, ERR_BAD_ARG, ERR_NONFINITE_LOGP, \
    ERR_HIP, ERR_OOM, ERR_NO_DEVICE, ERR_UNSUPPORTED = range(10)
# kmc_density
GAUSSIAN_ISO, EXPONENTIAL, ROSENBROCK, LOGNORMAL, MVNORMAL2 = range(5)
USER_DENSITY = 100
HOST_DENSITY = 101
DATA_DENSITY = 102
HOST_LOGPDF_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_void_p)
HOST_PROPOSE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_void_p)
HOST_ACCEPTED_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint8), C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p)
F64 = 0
F32 = 1       # rows and chain kept in float on the device; arithmetic and host buffers stay double
STORE_CHAIN, STORE_LOGP, MOMENTS, NO_GRAPH, P2P, ISLANDS, P2P_FINEGRAINED, P2P_PUSH = 1, 2, 4, 8, 16, 64, 128, 512
STREAM_CHAIN = 2048
CHAIN_BY_WALKER = 4096
STORE_BLOBS = 8192
# kmc_config.move
MOVE_STRETCH, MOVE_DE, MOVE_SNOOKER, MOVE_MIX = 0, 1, 3, 4
MIX_MAX = 4
TEMPS_MAX = 64  # parallel tempering: most rungs of a ladder (kmc_config.ntemps)
CONV_NEED_LAGS, CONV_TRUNCATED = 1, 2  # flags of kmc_convergence_stats
CONV_HAS_NAN = 4  # flag of kmc_*_rank_convergence: a NaN among the pooled draws of the column
TEMPER_WHOLE, TEMPER_LIKELIHOOD = 0, 1  # kmc_config.temper_mode
P2P_HANDLE_BYTES = 128
RCCL_ID_BYTES = 128

# Every symbol include/kissmcmc_hip.h declares (tests check they are all exported).
SYMBOLS = [
    "kmc_version", "kmc_device_count", "kmc_last_error", "kmc_status_string", "kmc_validate",
    "kmc_g_pdf", "kmc_cdf_g_inv", "kmc_emcee_run", "kmc_sampler_create", "kmc_sampler_destroy",
    "kmc_sampler_set_stream", "kmc_sampler_bind_positions", "kmc_sampler_p2p_export", "kmc_sampler_p2p_connect", "kmc_sampler_p2p_connect_local", "kmc_sampler_p2p_link_probe", "kmc_sampler_set_positions", "kmc_sampler_init_ball", "kmc_sampler_set_state", "kmc_sampler_run", "kmc_sampler_half_step",
    "kmc_sampler_sync", "kmc_sampler_last_run_ms", "kmc_sampler_generation", "kmc_sampler_nsamples",
    "kmc_sampler_launch_count", "kmc_sampler_describe", "kmc_sampler_device_ptr", "kmc_sampler_get_positions",
    "kmc_sampler_get_logp", "kmc_sampler_get_naccept", "kmc_sampler_get_accept_ratio",
    "kmc_sampler_get_moments", "kmc_sampler_get_chain", "kmc_sampler_get_chain_by_walker", "kmc_logpdf_eval", "kmc_logpdf_eval_host",
    "kmc_user_density_create", "kmc_user_density_create_body", "kmc_user_density_destroy", "kmc_metropolis_validate", "kmc_metropolis_run", "kmc_cholesky_lower", "kmc_int_acorr", "kmc_sampler_int_acorr",
    "kmc_sizeof_config", "kmc_sizeof_metropolis_config", "kmc_sizeof_outputs", "kmc_sizeof_metropolis_outputs", "kmc_deal_seed", "kmc_deal_perm", "kmc_sampler_deal_pack", "kmc_sampler_deal_unpack",
    "kmc_sampler_get_walker_ids", "kmc_sampler_set_walker_ids", "kmc_sampler_set_chain_host", "kmc_rccl_unique_id", "kmc_sampler_rccl_init",
    "kmc_sampler_rccl_capture", "kmc_sampler_rccl_set_capture", "kmc_rccl_version", "kmc_device_free_bytes",
    "kmc_sampler_launch_mode", "kmc_updated_budget", "kmc_set_updated_budget_mb", "kmc_debug_accept_terms",
    "kmc_debug_chain_by_walker", "kmc_debug_rows_compact", "kmc_debug_phase_spec", "kmc_debug_shared_draws", "kmc_debug_replay_variant",
    "kmc_user_density_create_body_blob", "kmc_user_density_nblob", "kmc_logpdf_blob_eval_host", "kmc_sampler_get_blobs",
    "kmc_device_cache_release", "kmc_user_density_is_separable", "kmc_host_prefault", "kmc_data_density_create",
    "kmc_sampler_get_rung_state", "kmc_sampler_set_rung_state", "kmc_sampler_get_swaps",
    "kmc_sampler_get_rung_loglike", "kmc_sampler_set_rung_loglike_sum", "kmc_sampler_get_ladder", "kmc_sampler_set_ladder",
    "kmc_sampler_order_stats", "kmc_sampler_chain_argmax", "kmc_chain_order_stats", "kmc_chain_argmax",
    "kmc_sampler_histograms", "kmc_chain_histograms", "kmc_hist_pair_plan",
    "kmc_sampler_lag_sums", "kmc_chain_lag_sums", "kmc_convergence_stats", "kmc_sampler_convergence", "kmc_chain_convergence",
    "kmc_convergence_plan",
    "kmc_rank_plan", "kmc_rank_normal_scores", "kmc_sampler_rank_scores", "kmc_chain_rank_scores", "kmc_sampler_rank_convergence",
    "kmc_chain_rank_convergence",
    "kmc_beta_quantile", "kmc_quantile_mcse_ranks", "kmc_indicator_moments", "kmc_indicator_plan", "kmc_sampler_indicator_lags",
    "kmc_chain_indicator_lags", "kmc_sampler_quantile_mcse", "kmc_chain_quantile_mcse",
    "kmc_sampler_hdi", "kmc_chain_hdi", "kmc_hdi_span",
    "kmc_sampler_covariance", "kmc_chain_covariance", "kmc_cov_plan", "kmc_cov_correlation",
    "kmc_sampler_pointwise_stats", "kmc_chain_pointwise_stats", "kmc_sampler_pointwise_loglike", "kmc_chain_pointwise_loglike",
    "kmc_pointwise_plan", "kmc_waic_stats",
    "kmc_sampler_psis_loo", "kmc_chain_psis_loo", "kmc_sampler_psis_tail", "kmc_chain_psis_tail", "kmc_psis_plan", "kmc_loo_stats",
    "kmc_psis_smooth_host",
    "kmc_user_density_set_grad", "kmc_grad_eval_host",
    "kmc_sampler_relative_eff", "kmc_chain_relative_eff", "kmc_sampler_pointwise_weights", "kmc_chain_pointwise_weights",
    "kmc_sampler_psis_loo_reff", "kmc_chain_psis_loo_reff", "kmc_sampler_psis_tail_reff", "kmc_chain_psis_tail_reff",
]


class Config(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32),
        ("density", C.c_int32),
        ("params", C.c_double * 8),
        ("nwalkers", C.c_int64),
        ("ndim", C.c_int64),
        ("ngenerations", C.c_int64),
        ("nburnin", C.c_int64),
        ("nthin", C.c_int64),
        ("a_scale", C.c_double),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("device", C.c_int32),
        ("shard_rank", C.c_int32),
        ("shard_count", C.c_int32),
        ("user_density", C.c_void_p),
        ("island_gens", C.c_int32),
        ("island_size", C.c_int32),
        ("host_logpdf", C.c_void_p),
        ("host_user", C.c_void_p),
        ("host_accepted", C.c_void_p),
        ("deal_rank", C.c_int32),
        ("deal_count", C.c_int32),
        ("temper_mode", C.c_int32),     # TEMPER_WHOLE or TEMPER_LIKELIHOOD (a DataDensity with a ladder)
        ("temper_pad_", C.c_int32),
        ("adapt_until", C.c_int64),     # adaptive ladder: the sweeps of generations < adapt_until adapt it (0: nburnin)
        ("adapt_lag", C.c_double),
        ("adapt_time", C.c_double),
        ("adapt", C.c_int32),           # 1: on
        ("adapt_pad_", C.c_int32),
        ("snooker_gamma", C.c_double),
        ("mix_count", C.c_int32),
        # (the header's mix_move[4] ... mix_sigma[4], spelled out member by member like the Julia mirror)
        ("mix_move0", C.c_int32), ("mix_move1", C.c_int32), ("mix_move2", C.c_int32), ("mix_move3", C.c_int32),
        ("mix_pad0_", C.c_int32), ("mix_pad1_", C.c_int32), ("mix_pad2_", C.c_int32),
        ("mix_weight0", C.c_double), ("mix_weight1", C.c_double), ("mix_weight2", C.c_double), ("mix_weight3", C.c_double),
        ("mix_gamma0", C.c_double), ("mix_gamma1", C.c_double), ("mix_gamma2", C.c_double), ("mix_gamma3", C.c_double),
        ("mix_sigma0", C.c_double), ("mix_sigma1", C.c_double), ("mix_sigma2", C.c_double), ("mix_sigma3", C.c_double),
        ("betas", C.c_void_p),          # parallel tempering: const double* [ntemps], copied at creation
        ("ntemps", C.c_int32),
        ("swap_every", C.c_int32),
        ("move", C.c_int32),
        ("move_pad_", C.c_int32),
        ("de_gamma0", C.c_double),
        ("de_sigma", C.c_double),
    ]


class Outputs(C.Structure):
    _fields_ = [
        ("chain", C.POINTER(C.c_double)),
        ("chain_logp", C.POINTER(C.c_double)),
        ("accept_ratio", C.POINTER(C.c_double)),
        ("naccept", C.POINTER(C.c_int64)),
        ("final_pos", C.POINTER(C.c_double)),
        ("final_logp", C.POINTER(C.c_double)),
        ("sum", C.POINTER(C.c_double)),
        ("sumsq", C.POINTER(C.c_double)),
        ("nmoment", C.c_int64),
        ("nsamples", C.c_int64),
        ("device_ms", C.c_double),
        ("blobs", C.POINTER(C.c_double)),
    ]


class MetropolisConfig(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32),
        ("density", C.c_int32),
        ("params", C.c_double * 8),
        ("nchains", C.c_int64),
        ("ndim", C.c_int64),
        ("niter", C.c_int64),
        ("nburnin", C.c_int64),
        ("nthin", C.c_int64),
        ("step", C.POINTER(C.c_double)),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("device", C.c_int32),
        ("user_density", C.c_void_p),
        ("host_logpdf", C.c_void_p),
        ("host_user", C.c_void_p),
        ("host_accepted", C.c_void_p),
        ("host_propose", C.c_void_p),
        ("chol", C.POINTER(C.c_double)),
        ("tune_rounds", C.c_int32),
        ("tune_scale", C.c_double),
        ("hmc_nleap", C.c_int32),       # 0: off; leapfrog steps per iteration of the HMC step (`step` then holds the step sizes)
        ("hmc_jitter", C.c_double),     # in [0, 1)
    ]


class MetropolisOutputs(C.Structure):
    _fields_ = [
        ("chain", C.POINTER(C.c_double)),
        ("chain_logp", C.POINTER(C.c_double)),
        ("accept_ratio", C.POINTER(C.c_double)),
        ("naccept", C.POINTER(C.c_int64)),
        ("final_pos", C.POINTER(C.c_double)),
        ("final_logp", C.POINTER(C.c_double)),
        ("chain_sum", C.POINTER(C.c_double)),
        ("chain_sumsq", C.POINTER(C.c_double)),
        ("nsamples", C.c_int64),
        ("device_ms", C.c_double),
        ("blobs", C.POINTER(C.c_double)),
        ("final_blob", C.POINTER(C.c_double)),
        ("chol_out", C.POINTER(C.c_double)),
        ("tune_skipped", C.c_int64),
        ("tune_ms", C.c_double),
    ]


class KmcError(RuntimeError):
    """A non-zero ``kmc_status``; ``.status`` holds the code."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own HIP/HSA runtime.  If this library (linked against
    # /opt/rocm) initialises HIP before torch's copies are loaded, torch later finds no GPU; loading
    # torch's libraries first keeps both usable in one process.  Pure C-ABI users are unaffected.
    if "no-torch-preload" not in os.environ.get("KMC_DEBUG", "").split(","):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m kissmcmc_jl_amd.build` "
            "(hipcc --offload-arch=gfx950). The emcee hot path has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int64)
    vp = C.c_void_p
    cfgp = C.POINTER(Config)
    L.kmc_version.restype = C.c_int
    L.kmc_device_count.restype = C.c_int
    L.kmc_last_error.restype = C.c_char_p
    L.kmc_status_string.restype = C.c_char_p
    L.kmc_status_string.argtypes = [C.c_int]
    L.kmc_validate.argtypes = [cfgp]
    L.kmc_g_pdf.restype = C.c_double
    L.kmc_g_pdf.argtypes = [C.c_double, C.c_double]
    L.kmc_cdf_g_inv.restype = C.c_double
    L.kmc_cdf_g_inv.argtypes = [C.c_double, C.c_double]
    L.kmc_emcee_run.argtypes = [cfgp, dp, C.POINTER(Outputs)]
    L.kmc_sampler_create.argtypes = [cfgp, C.POINTER(vp)]
    L.kmc_sampler_destroy.restype = None
    L.kmc_sampler_destroy.argtypes = [vp]
    L.kmc_sampler_set_stream.argtypes = [vp, vp]
    L.kmc_sampler_bind_positions.argtypes = [vp, vp]
    L.kmc_sampler_p2p_export.argtypes = [vp, vp]
    L.kmc_sampler_p2p_connect.argtypes = [vp, vp]
    L.kmc_sampler_p2p_connect_local.argtypes = [vp, C.POINTER(C.c_void_p)]
    L.kmc_sampler_p2p_link_probe.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.kmc_sampler_set_positions.argtypes = [vp, dp]
    L.kmc_sampler_init_ball.argtypes = [vp, dp, dp, C.c_uint64, C.c_int, C.c_int]
    L.kmc_sampler_set_state.argtypes = [vp, dp, dp, ip, C.c_int64]
    L.kmc_sampler_get_rung_state.argtypes = [vp, dp, dp, ip, dp]
    L.kmc_sampler_set_rung_state.argtypes = [vp, dp, dp, ip, C.POINTER(C.c_uint64), dp, C.c_int64]
    L.kmc_sampler_get_swaps.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kmc_sampler_get_rung_loglike.argtypes = [vp, dp, dp, dp]
    L.kmc_sampler_set_rung_loglike_sum.argtypes = [vp, dp]
    L.kmc_sampler_get_ladder.argtypes = [vp, dp, dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.kmc_sampler_set_ladder.argtypes = [vp, dp, dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.kmc_sampler_run.argtypes = [vp, C.c_int64]
    L.kmc_sampler_half_step.argtypes = [vp, C.c_int]
    L.kmc_sampler_sync.argtypes = [vp]
    L.kmc_sampler_last_run_ms.argtypes = [vp, dp]
    L.kmc_sampler_generation.restype = C.c_int64
    L.kmc_sampler_generation.argtypes = [vp]
    L.kmc_sampler_nsamples.restype = C.c_int64
    L.kmc_sampler_nsamples.argtypes = [vp]
    L.kmc_sampler_launch_count.restype = C.c_int64
    L.kmc_sampler_launch_count.argtypes = [vp]
    L.kmc_sampler_describe.argtypes = [vp, C.c_char_p, C.c_int64]
    L.kmc_sampler_device_ptr.restype = vp
    L.kmc_sampler_device_ptr.argtypes = [vp, C.c_int]
    L.kmc_sampler_get_positions.argtypes = [vp, dp]
    L.kmc_sampler_get_logp.argtypes = [vp, dp]
    L.kmc_sampler_get_naccept.argtypes = [vp, ip]
    L.kmc_sampler_get_accept_ratio.argtypes = [vp, dp]
    L.kmc_sampler_get_moments.argtypes = [vp, dp, dp, ip]
    L.kmc_sampler_get_chain.argtypes = [vp, dp, dp]
    L.kmc_sampler_get_chain_by_walker.argtypes = [vp, dp, dp]
    L.kmc_logpdf_eval.argtypes = [cfgp, vp, vp, C.c_int64, vp]
    L.kmc_logpdf_eval_host.argtypes = [cfgp, dp, dp, C.c_int64]
    L.kmc_user_density_create.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.kmc_user_density_create_body.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.kmc_user_density_set_grad.argtypes = [vp, C.c_char_p]
    L.kmc_grad_eval_host.argtypes = [cfgp, dp, dp, C.c_int64]
    L.kmc_user_density_create_body_blob.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.kmc_data_density_create.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_int64, C.c_int32, C.POINTER(vp)]
    L.kmc_user_density_is_separable.restype = C.c_int
    L.kmc_user_density_is_separable.argtypes = [vp]
    L.kmc_user_density_nblob.restype = C.c_int
    L.kmc_user_density_nblob.argtypes = [vp]
    L.kmc_logpdf_blob_eval_host.argtypes = [cfgp, dp, dp, dp, C.c_int64]
    L.kmc_sampler_get_blobs.argtypes = [vp, dp, dp, C.c_int]
    L.kmc_user_density_destroy.restype = None
    L.kmc_user_density_destroy.argtypes = [vp]
    L.kmc_metropolis_validate.argtypes = [C.POINTER(MetropolisConfig)]
    L.kmc_metropolis_run.argtypes = [C.POINTER(MetropolisConfig), dp, C.POINTER(MetropolisOutputs)]
    L.kmc_cholesky_lower.argtypes = [dp, C.c_int, dp, C.POINTER(C.c_int)]
    L.kmc_int_acorr.argtypes = [dp, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int, dp, dp]
    L.kmc_sampler_int_acorr.argtypes = [vp, C.c_double, dp, dp]
    bp = C.POINTER(C.c_uint8)
    L.kmc_sampler_order_stats.argtypes = [vp, C.c_int64, bp, ip, C.c_int32, dp, dp, ip]
    L.kmc_sampler_chain_argmax.argtypes = [vp, C.c_int64, bp, ip, ip, dp, dp]
    L.kmc_chain_order_stats.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, ip, C.c_int32, C.c_int, dp, dp, ip]
    L.kmc_chain_argmax.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int, ip, ip, dp, dp]
    i32p = C.POINTER(C.c_int32)
    L.kmc_sampler_histograms.argtypes = [vp, C.c_int64, bp, i32p, C.c_int32, dp, C.c_int32, C.c_int32, ip, ip, ip, ip]
    L.kmc_chain_histograms.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, i32p, C.c_int32, dp, C.c_int32, C.c_int, ip, ip, ip, ip]
    L.kmc_hist_pair_plan.argtypes = [C.c_int32, C.c_int32, i32p, i32p, i32p]
    L.kmc_sampler_lag_sums.argtypes = [vp, C.c_int64, bp, C.c_int32, C.c_int32, C.c_int64, C.c_int64, dp, dp, dp, ip, ip]
    L.kmc_chain_lag_sums.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int32, C.c_int64, C.c_int64, C.c_int, dp, dp, dp, ip, ip]
    L.kmc_convergence_stats.argtypes = [C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, C.c_int64, C.c_int64, dp, dp, dp, dp, dp, dp, dp, ip, i32p]
    L.kmc_sampler_convergence.argtypes = [vp, C.c_int64, bp, C.c_int32, C.c_int32, C.c_int64, dp, dp, dp, dp, dp, dp, dp, ip, i32p, ip, ip, ip]
    L.kmc_chain_convergence.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int32, C.c_int64, C.c_int, dp, dp, dp, dp, dp, dp, dp, ip, i32p, ip, ip, ip]
    L.kmc_convergence_plan.argtypes = [i32p, i32p, i32p, i32p]
    L.kmc_rank_plan.argtypes = [i32p, i32p, i32p, i32p]
    L.kmc_rank_normal_scores.argtypes = [ip, C.c_int64, C.c_int64, dp]
    L.kmc_sampler_rank_scores.argtypes = [vp, C.c_int64, bp, C.c_int32, C.c_int32, C.c_int32, ip, dp, dp, ip, ip, ip]
    L.kmc_chain_rank_scores.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int32, C.c_int32, C.c_int, ip, dp, dp, ip, ip, ip]
    L.kmc_sampler_rank_convergence.argtypes = [vp, C.c_int64, bp, C.c_int32, C.c_int32, C.c_int64] + [dp] * 10 + [ip, i32p, ip, ip, ip]
    L.kmc_chain_rank_convergence.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int32, C.c_int64, C.c_int] + [dp] * 10 + [ip, i32p, ip, ip, ip]
    u64p = C.POINTER(C.c_uint64)
    L.kmc_beta_quantile.argtypes = [C.c_double, C.c_double, C.c_double, dp]
    L.kmc_quantile_mcse_ranks.argtypes = [C.c_int64, C.c_double, C.c_double, dp, dp, ip, ip]
    L.kmc_indicator_moments.argtypes = [C.c_int64, C.c_int64, dp, dp]
    L.kmc_indicator_plan.argtypes = [i32p, i32p, i32p, i32p]
    L.kmc_sampler_indicator_lags.argtypes = [vp, C.c_int64, bp, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int64, C.c_int64, ip, u64p, ip, ip]
    L.kmc_chain_indicator_lags.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int32, C.c_int32, dp, C.c_int64, C.c_int64, C.c_int,
                                           ip, u64p, ip, ip]
    L.kmc_sampler_quantile_mcse.argtypes = [vp, C.c_int64, bp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, dp] + [dp] * 5 + [ip, i32p, ip, ip, ip]
    L.kmc_chain_quantile_mcse.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int32, C.c_int64, C.c_int32, dp, C.c_int] + [dp] * 5 + \
        [ip, i32p, ip, ip, ip]
    L.kmc_sampler_hdi.argtypes = [vp, C.c_int64, bp, C.c_int32, dp, C.c_int32, dp, dp, ip, ip, ip, ip]
    L.kmc_chain_hdi.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, dp, C.c_int32, C.c_int, dp, dp, ip, ip, ip, ip]
    L.kmc_hdi_span.argtypes = [C.c_int64, C.c_double, ip, ip]
    L.kmc_sampler_covariance.argtypes = [vp, C.c_int64, bp, C.c_int32, dp, dp, ip, ip]
    L.kmc_chain_covariance.argtypes = [dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int, dp, dp, ip, ip]
    L.kmc_cov_plan.argtypes = [C.c_int64, i32p, i32p, i32p, i32p]
    L.kmc_cov_correlation.argtypes = [C.c_int64, dp, dp, dp]
    held_out = [dp, C.c_int64, C.c_int32]
    host_chain = [vp, dp, dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, bp, C.c_int64]
    L.kmc_sampler_pointwise_stats.argtypes = [vp, C.c_int64, bp, C.c_int64] + held_out + [dp, ip, ip]
    L.kmc_chain_pointwise_stats.argtypes = host_chain + held_out + [C.c_int, dp, ip, ip]
    L.kmc_sampler_pointwise_loglike.argtypes = [vp, C.c_int64, bp, C.c_int64] + held_out + [C.c_int64, C.c_int64, dp, ip]
    L.kmc_chain_pointwise_loglike.argtypes = host_chain + held_out + [C.c_int64, C.c_int64, C.c_int, dp, ip]
    L.kmc_pointwise_plan.argtypes = [C.c_int64, C.c_int64, ip, ip, i32p, i32p, ip]
    L.kmc_waic_stats.argtypes = [C.c_int64, C.c_int64, dp, dp, dp, dp, dp]
    psis_sel = [C.c_double, C.c_int64, C.c_int64, C.c_int64]         # r_eff, obs_first, obs_count, workspace_bytes
    L.kmc_sampler_psis_loo.argtypes = [vp, C.c_int64, bp, C.c_int64] + psis_sel + [dp, dp, ip, ip]
    L.kmc_chain_psis_loo.argtypes = host_chain + psis_sel + [C.c_int, dp, dp, ip, ip]
    L.kmc_sampler_psis_tail.argtypes = [vp, C.c_int64, bp, C.c_int64] + psis_sel + [dp, dp, dp, i32p, ip, ip]
    L.kmc_chain_psis_tail.argtypes = host_chain + psis_sel + [C.c_int, dp, dp, dp, i32p, ip, ip]
    L.kmc_psis_plan.argtypes = [C.c_int64, C.c_int64, C.c_double, C.c_int64, ip, ip, ip, ip]
    L.kmc_loo_stats.argtypes = [C.c_int64, C.c_int64, dp, dp, dp, dp]
    L.kmc_psis_smooth_host.argtypes = [C.c_int64, dp, C.c_double, dp, dp, dp, dp]
    reff_sel = [C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64]   # obs_first, obs_count, split, max_lag, workspace_bytes
    L.kmc_sampler_relative_eff.argtypes = [vp, C.c_int64, bp, C.c_int64] + reff_sel + [dp, dp, ip, i32p, ip, ip, ip, ip]
    L.kmc_chain_relative_eff.argtypes = host_chain + reff_sel + [C.c_int, dp, dp, ip, i32p, ip, ip, ip, ip]
    L.kmc_sampler_pointwise_weights.argtypes = [vp, C.c_int64, bp, C.c_int64] + held_out + [C.c_int64, C.c_int64, dp, dp, ip]
    L.kmc_chain_pointwise_weights.argtypes = host_chain + held_out + [C.c_int64, C.c_int64, C.c_int, dp, dp, ip]
    psis_reff = [dp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64]   # r_eff_j, split, max_lag, obs_first, obs_count, workspace_bytes
    L.kmc_sampler_psis_loo_reff.argtypes = [vp, C.c_int64, bp, C.c_int64] + psis_reff + [dp, dp, dp, ip, ip, ip, ip]
    L.kmc_chain_psis_loo_reff.argtypes = host_chain + psis_reff + [C.c_int, dp, dp, dp, ip, ip, ip, ip]
    L.kmc_sampler_psis_tail_reff.argtypes = [vp, C.c_int64, bp, C.c_int64] + psis_reff + [dp, dp, dp, i32p, ip, dp, ip, ip, ip]
    L.kmc_chain_psis_tail_reff.argtypes = host_chain + psis_reff + [C.c_int, dp, dp, dp, i32p, ip, dp, ip, ip, ip]
    L.kmc_deal_seed.restype = C.c_uint64
    L.kmc_deal_seed.argtypes = [C.c_uint64, C.c_int32]
    L.kmc_deal_perm.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int64, ip, ip]
    L.kmc_sampler_deal_pack.argtypes = [vp, C.c_int64, vp]
    L.kmc_sampler_deal_unpack.argtypes = [vp, vp]
    L.kmc_sampler_get_walker_ids.argtypes = [vp, ip]
    L.kmc_sampler_set_walker_ids.argtypes = [vp, ip]
    L.kmc_sampler_set_chain_host.argtypes = [vp, dp, dp]
    L.kmc_rccl_unique_id.argtypes = [vp]
    L.kmc_sampler_rccl_init.argtypes = [vp, vp]
    L.kmc_sampler_rccl_capture.argtypes = [vp, C.POINTER(C.c_int)]
    L.kmc_sampler_rccl_set_capture.argtypes = [vp, C.c_int]
    L.kmc_rccl_version.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int64]
    L.kmc_device_free_bytes.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.kmc_device_cache_release.argtypes = []
    L.kmc_device_cache_release.restype = None
    L.kmc_host_prefault.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    L.kmc_host_prefault.restype = None
    L.kmc_sampler_launch_mode.restype = C.c_int
    L.kmc_sampler_launch_mode.argtypes = [vp, C.POINTER(C.c_int)]
    L.kmc_updated_budget.restype = None
    L.kmc_updated_budget.argtypes = [ip, ip]
    L.kmc_set_updated_budget_mb.restype = None
    L.kmc_set_updated_budget_mb.argtypes = [C.c_double]
    L.kmc_debug_accept_terms.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_double, C.c_int64, C.c_int, ip, dp, dp, dp]
    L.kmc_debug_chain_by_walker.argtypes = [vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, dp, C.c_int64, C.c_int]
    L.kmc_debug_rows_compact.argtypes = [dp, C.c_int64, C.c_int64, C.c_int64, dp, C.c_int64, C.c_int]
    L.kmc_debug_phase_spec.restype = C.c_int
    L.kmc_debug_phase_spec.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.kmc_debug_shared_draws.restype = C.c_int
    L.kmc_debug_shared_draws.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.kmc_debug_replay_variant.restype = C.c_int
    L.kmc_debug_replay_variant.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int]
    # layout drift between this mirror and the library fails here, at load, not inside the first real call
    for fn, T in ((L.kmc_sizeof_config, Config), (L.kmc_sizeof_metropolis_config, MetropolisConfig),
                  (L.kmc_sizeof_outputs, Outputs), (L.kmc_sizeof_metropolis_outputs, MetropolisOutputs)):
        if fn() != C.sizeof(T):
            raise ImportError(f"{LIB_PATH}: struct layout mismatch ({fn.__name__}() = {fn()}, the ctypes mirror {T.__name__} is {C.sizeof(T)} bytes): "
                              "rebuild the library or update kissmcmc_jl_amd/_lib.py from include/kissmcmc_hip.h")
    _lib = L
    return L


def check(status: int) -> None:
    if status != OK:
        L = lib()
        msg = L.kmc_last_error().decode() or L.kmc_status_string(status).decode()
        raise KmcError(status, msg)
