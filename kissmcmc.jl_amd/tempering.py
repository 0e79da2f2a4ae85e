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


TEMPER_MODES = {None: _lib.TEMPER_WHOLE, "whole": _lib.TEMPER_WHOLE, "likelihood": _lib.TEMPER_LIKELIHOOD}


def check_betas(betas, prior_rung: bool = False) -> np.ndarray:
    """The ladder as a contiguous float64 array, or ``ValueError`` naming what is wrong with it (the library checks the same).
    ``prior_rung`` (``temper="likelihood"``): the last beta may be 0, the rung that samples the prior."""
    b = np.ascontiguousarray(np.asarray(betas, dtype=np.float64))
    if b.ndim != 1 or not 2 <= b.size <= _lib.TEMPS_MAX:
        raise ValueError(f"betas must be a 1-D sequence of 2 .. {_lib.TEMPS_MAX} inverse temperatures")
    positive = b[:-1] if (prior_rung and b[-1] == 0.0) else b
    if not np.all(np.isfinite(b)) or not np.all(positive > 0):
        raise ValueError("betas must be finite and > 0" + (" (only the last one may be 0)" if prior_rung else
                                                           " (a rung with beta = 0 needs temper=\"likelihood\")"))
    if b[0] != 1.0:
        raise ValueError("betas[0] must be 1 (rung 0 samples the target itself)")
    if not np.all(np.diff(b) < 0):
        raise ValueError("betas must be strictly decreasing")
    return b


def apply_tempering(cfg, betas=None, ntemps=None, beta_min=None, swap_every=1, temper=None):
    """Fill ``cfg.betas / ntemps / swap_every / temper_mode``; returns the array ``cfg.betas`` points into (keep it alive until the
    sampler exists: the library copies it at creation), or ``None`` when tempering is off.  ``temper``: ``None`` / ``"whole"`` (rung
    ``t`` samples ``exp(betas[t] * logpdf)``) or ``"likelihood"`` (a :class:`DataDensity`: ``prior + betas[t] * S``)."""
    if temper not in TEMPER_MODES:
        raise ValueError("temper must be None, \"whole\" or \"likelihood\"")
    cfg.temper_mode = TEMPER_MODES[temper]
    if betas is None and not ntemps:
        if beta_min is not None:
            raise ValueError("beta_min needs ntemps")
        if temper == "likelihood":
            raise ValueError("temper=\"likelihood\" needs a ladder: betas=, or ntemps= and beta_min=")
        cfg.betas, cfg.ntemps, cfg.swap_every = None, 0, 0
        return None
    if betas is None:
        if beta_min is None:
            raise ValueError("ntemps needs beta_min (the ladder is geometric_betas(ntemps, beta_min)), or pass betas")
        b = geometric_betas(ntemps, beta_min)
    else:
        b = check_betas(betas, prior_rung=temper == "likelihood")
        if ntemps and int(ntemps) != b.size:
            raise ValueError("ntemps does not match len(betas)")
    if int(swap_every) != swap_every or int(swap_every) < 0:
        raise ValueError("swap_every must be an integer >= 0 (0: never)")
    cfg.betas = b.ctypes.data_as(C.c_void_p)
    cfg.ntemps = int(b.size)
    cfg.swap_every = int(swap_every)
    return b


ADAPT_LAG, ADAPT_TIME = 10000.0, 100.0     # ptemcee's adaptation_lag and adaptation_time


def apply_adapt(cfg, adapt=None):
    """Fill ``cfg.adapt / adapt_until / adapt_lag / adapt_time`` from ``adapt``: ``None`` / ``False`` (off), ``True`` (the defaults:
    ``lag=10000``, ``time=100``, until the end of burn-in) or a dict with any of ``lag``, ``time``, ``until`` (``None`` or 0: ``nburnin``).  Returns the dict in
    force, or ``None`` when off.  The library checks the values (``KMC_ERR_BAD_ARG``, "adaptive ladder: ...")."""
    cfg.adapt, cfg.adapt_until, cfg.adapt_lag, cfg.adapt_time = 0, 0, 0.0, 0.0
    if adapt is None or adapt is False:
        return None
    if adapt is True:
        adapt = {}
    if not isinstance(adapt, dict) or not set(adapt) <= {"lag", "time", "until"}:
        raise ValueError("adapt must be None, True or a dict with any of lag=, time=, until=")
    out = dict(lag=float(adapt.get("lag", ADAPT_LAG)), time=float(adapt.get("time", ADAPT_TIME)),
               until=None if adapt.get("until") is None else int(adapt["until"]))
    if out["until"] == 0:                  # (kmc_config.adapt_until == 0 means nburnin, in every binding)
        out["until"] = None
    cfg.adapt, cfg.adapt_lag, cfg.adapt_time = 1, out["lag"], out["time"]
    cfg.adapt_until = 0 if out["until"] is None else out["until"]
    return out


def adapt_ladder(betas, S, A, k, lag=ADAPT_LAG, time=ADAPT_TIME):
    """One update of the adaptive ladder's rule, restated in numpy (``include/kissmcmc_hip.h`` above ``kmc_sampler_get_ladder``):
    ``betas`` [T >= 3], the state ``S`` [T - 2] (``S[j - 1] = log(1 / betas[j] - 1 / betas[j - 1])`` when the ladder was created),
    the round's swap acceptance ``A`` [T - 1] per neighbouring pair and the round number ``k``.  Returns ``(betas', S', skipped)``:
    new arrays, equal to the old ones with ``skipped = 1`` when the candidate ladder is not finite and strictly decreasing between
    ``betas[0] = 1`` and ``betas[-1]``, which never move.  The operations and their order are the device's; only ``exp`` is to
    rounding, once per rung, and that difference does not accumulate because ``S`` is never derived from the betas again."""
    b = np.array(betas, dtype=np.float64)
    S = np.array(S, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    T = b.size
    if b.ndim != 1 or T < 3 or S.shape != (T - 2,) or A.shape != (T - 1,):
        raise ValueError("adapt_ladder: betas [T >= 3], S [T - 2] and A [T - 1]")
    lag, time = float(lag), float(time)
    kappa = (lag / (float(k) + lag)) / time
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        S1 = S + kappa * (A[:-1] - A[1:])
        tau, b1 = 1.0, np.empty(T - 2)
        for j in range(T - 2):
            tau = tau + np.exp(S1[j])
            b1[j] = 1.0 / tau
        full = np.concatenate(([1.0], b1, [b[-1]]))
        ok = bool(np.all(np.isfinite(b1)) and np.all(full[1:] < full[:-1]))
    if not ok:
        return b, S, 1
    b[1:-1] = b1
    return b, S1, 0


def thermodynamic_integration(betas, mean_loglike):
    """``(logZ, err)``: the trapezoid of ``mean_loglike`` = ``<S>_beta`` over the ladder ``betas``, in ascending beta -- the
    thermodynamic integral ``log Z = int_0^1 <S>_beta dbeta`` of a likelihood-tempered ladder (``Sampler.rung_loglike_mean()``) --
    and ``|logZ - logZ of every second rung|`` (counted from ``beta = 1`` down), ptemcee's estimate of the discretisation error.
    ``Z`` is the evidence when the prior is normalised and the ladder reaches ``beta = 0``; a ladder that stops at ``beta_min``
    gives the integral from there.  Pure numpy: no device."""
    b = np.asarray(betas, dtype=np.float64)
    m = np.asarray(mean_loglike, dtype=np.float64)
    if b.ndim != 1 or b.shape != m.shape or b.size < 2:
        raise ValueError("betas and mean_loglike must be 1-D sequences of the same length (>= 2)")
    order = np.argsort(-b, kind="stable")                  # from beta = 1 down, whatever order the ladder was given in
    b, m = b[order], m[order]
    if np.any(np.diff(b) >= 0):
        raise ValueError("betas must be distinct")

    def trapezoid(x, y):
        x, y = x[::-1], y[::-1]                            # ascending beta
        return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x)))

    b2, m2 = b[::2], m[::2]
    if b2[-1] != b[-1]:                                    # every second rung, and the lowest one: the same interval
        b2, m2 = np.append(b2, b[-1]), np.append(m2, m[-1])
    logz = trapezoid(b, m)
    return logz, abs(logz - trapezoid(b2, m2))
