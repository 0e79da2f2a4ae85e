"""Parallel tempering: the ladder of inverse temperatures a tempered :class:`~kissmcmc_jl_amd.Sampler` takes
(``betas=`` / ``ntemps=``; ``kmc_config.betas``, ``ntemps``, ``swap_every`` in ``include/kissmcmc_hip.h``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def geometric_betas(ntemps: int, beta_min: float) -> np.ndarray:
    """``ntemps`` inverse temperatures from 1 down to ``beta_min`` in equal ratios: ``beta_t = beta_min ** (t / (ntemps - 1))``,
    with ``betas[0] == 1.0`` and ``betas[-1] == beta_min`` exactly."""
    ntemps = int(ntemps)
    beta_min = float(beta_min)
    if not 2 <= ntemps <= _lib.TEMPS_MAX:
        raise ValueError(f"ntemps must be 2 .. {_lib.TEMPS_MAX}")
    if not (0.0 < beta_min < 1.0) or not np.isfinite(beta_min):
        raise ValueError("beta_min must lie strictly between 0 and 1")
    b = beta_min ** (np.arange(ntemps, dtype=np.float64) / (ntemps - 1))
    b[0], b[-1] = 1.0, beta_min
    if not np.all(np.diff(b) < 0):
        raise ValueError("beta_min is too close to 1 for this many rungs: the ladder is not strictly decreasing")
    return b


def check_betas(betas) -> np.ndarray:
    """The ladder as a contiguous float64 array, or ``ValueError`` naming what is wrong with it (the library checks the same)."""
    b = np.ascontiguousarray(np.asarray(betas, dtype=np.float64))
    if b.ndim != 1 or not 2 <= b.size <= _lib.TEMPS_MAX:
        raise ValueError(f"betas must be a 1-D sequence of 2 .. {_lib.TEMPS_MAX} inverse temperatures")
    if not np.all(np.isfinite(b)) or not np.all(b > 0):
        raise ValueError("betas must be finite and > 0")
    if b[0] != 1.0:
        raise ValueError("betas[0] must be 1 (rung 0 samples the target itself)")
    if not np.all(np.diff(b) < 0):
        raise ValueError("betas must be strictly decreasing")
    return b


def apply_tempering(cfg, betas=None, ntemps=None, beta_min=None, swap_every=1):
    """Fill ``cfg.betas / ntemps / swap_every``; returns the array ``cfg.betas`` points into (keep it alive until the sampler
    exists: the library copies it at creation), or ``None`` when tempering is off."""
    if betas is None and not ntemps:
        if beta_min is not None:
            raise ValueError("beta_min needs ntemps")
        cfg.betas, cfg.ntemps, cfg.swap_every = None, 0, 0
        return None
    if betas is None:
        if beta_min is None:
            raise ValueError("ntemps needs beta_min (the ladder is geometric_betas(ntemps, beta_min)), or pass betas")
        b = geometric_betas(ntemps, beta_min)
    else:
        b = check_betas(betas)
        if ntemps and int(ntemps) != b.size:
            raise ValueError("ntemps does not match len(betas)")
    if int(swap_every) != swap_every or int(swap_every) < 0:
        raise ValueError("swap_every must be an integer >= 0 (0: never)")
    cfg.betas = b.ctypes.data_as(C.c_void_p)
    cfg.ntemps = int(b.size)
    cfg.swap_every = int(swap_every)
    return b
