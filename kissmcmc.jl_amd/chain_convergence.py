"""Convergence across chains: split-R-hat, the effective sample size and the Monte-Carlo standard error of the mean, with the
``evaluate_convergence``, ``error_of_estimated_mean`` and ``samples_vs_tau`` of reference ``src/analysis.jl:79-95, :209-226, :242-248``.

That file is entirely commented out in the reference, and the package its ``evaluate_convergence`` calls (MCMCDiagnostics.jl) is not
part of it, so there is no behaviour to be compatible with: the formulas of BDA3 (Gelman et al. 2014, pp. 284-287) as written down in
``include/kissmcmc_hip.h`` are the definition.  The chain means, chain variances and the lag sums of the variogram are computed on the
GPU where the chain lies (``kmc_sampler_lag_sums`` / ``kmc_chain_lag_sums``); what follows from them is a pure host stage in a fixed
order of operations (``kmc_convergence_stats``).

Input layout of the module-level functions: what ``emcee`` / ``metropolis_chains`` return, ``thetas[walker][sample]`` (scalar walkers)
or ``thetas[walker][sample][dim]``, and ``logdensities[walker][sample]``.  Every selected walker is a chain; with ``split`` (the
default) each is cut into two halves.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .summary import _HostProvider, _p, walker_mask

COLUMNS = ("mean", "std", "rhat", "ess", "mcse", "lag", "truncated", "m", "h")


def convergence_stats(m: int, h: int, chain_mean, chain_var, lagsum, max_lag: int):
    """The host stage (``kmc_convergence_stats``; needs no device): from ``chain_mean[ncols, m]``, ``chain_var[ncols, m]`` and
    ``lagsum[ncols, nlags]`` (the lag sums ``D_1 .. D_nlags``) a dict of per-column arrays ``mean, W, B, var_plus, rhat, ess, mcse``,
    ``T`` (int64) and ``flags`` (int32; bit 0: the truncation rule has not fired within the lags given, bit 1: nor up to
    ``max_lag``)."""
    cm = np.ascontiguousarray(chain_mean, dtype=np.float64)
    cv = np.ascontiguousarray(chain_var, dtype=np.float64)
    lag = np.ascontiguousarray(lagsum, dtype=np.float64)
    if cm.ndim != 2 or cv.shape != cm.shape or lag.ndim != 2 or lag.shape[0] != cm.shape[0]:
        raise ValueError("chain_mean and chain_var must be [ncols, m], lagsum [ncols, nlags]")
    ncols = cm.shape[0]
    out = {k: np.empty(ncols) for k in ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse")}
    out["T"] = np.empty(ncols, dtype=np.int64)
    out["flags"] = np.empty(ncols, dtype=np.int32)
    _lib.check(_lib.lib().kmc_convergence_stats(int(m), int(h), ncols, _p(cm, C.c_double), _p(cv, C.c_double), _p(lag, C.c_double), lag.shape[1],
                                                int(max_lag), *[_p(out[k], C.c_double) for k in ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse")],
                                                _p(out["T"], C.c_int64), _p(out["flags"], C.c_int32)))
    return out


def lag_plan():
    """The tile of the lag kernel (``kmc_convergence_plan``): dict ``lag_block, tile_samples, lanes, lds_bytes``."""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.lib().kmc_convergence_plan(*[C.byref(x) for x in v]))
    return dict(zip(("lag_block", "tile_samples", "lanes", "lds_bytes"), [x.value for x in v]))


def _max_lag_arg(max_lag):
    """None is the library's 0 (its default); anything else goes through as given, so that the library refuses what lies outside
    [3, h - 1] -- an explicit 0 included."""
    return 0 if max_lag is None else (int(max_lag) if int(max_lag) != 0 else -1)


def _count(mask, nwalkers):
    return nwalkers if mask is None else int(np.count_nonzero(mask))


def _lag_buffers(ncols, nw, nlags, split, moments):
    m = max(1, (2 if split else 1) * nw)
    cm = np.empty((ncols, m)) if moments else None
    cv = np.empty((ncols, m)) if moments else None
    return cm, cv, np.empty((ncols, max(0, int(nlags))))


def _lag_result(cm, cv, lag, m, h, lag0):
    return {"chain_mean": cm, "chain_var": cv, "lagsum": lag, "lag0": int(lag0), "m": m.value, "h": h.value}


def sampler_lag_sums(s, lag0=1, nlags=0, first_sample=0, walkers=None, split=True, logp=False, moments=True):
    """The device stage on the chain a :class:`Sampler` holds (``kmc_sampler_lag_sums``); see :func:`lag_sums`."""
    mask = walker_mask(walkers, s.nlocal)
    cm, cv, lag = _lag_buffers(s.ndim + (1 if logp else 0), _count(mask, s.nlocal), nlags, split, moments)
    m, h = C.c_int64(), C.c_int64()
    _lib.check(s._L.kmc_sampler_lag_sums(s._h, int(first_sample), _p(mask, C.c_uint8), int(bool(split)), int(bool(logp)), int(lag0), int(nlags),
                                         _p(cm, C.c_double), _p(cv, C.c_double), _p(lag, C.c_double), C.byref(m), C.byref(h)))
    return _lag_result(cm, cv, lag, m, h, lag0)


def lag_sums(thetas, logdensities=None, lag0=1, nlags=0, first_sample=0, walkers=None, split=True, moments=True, device=0):
    """The device stage of the diagnostics (``kmc_chain_lag_sums``): a dict ``chain_mean[ncols, m]``, ``chain_var[ncols, m]`` (None
    with ``moments=False``), ``lagsum[ncols, nlags]`` with ``lagsum[c, k] = D_(lag0 + k)``, the sum over chains ``j`` and samples
    ``i >= t`` of ``(x[i, j] - x[i - t, j])**2``, and ``m``, ``h``.  Chain ``j = half * nw + k`` for the k-th selected walker.  Each
    number is the sum of its terms in an order the library chooses: equal bits from equal calls, no float atomics."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    cm, cv, lag = _lag_buffers(p.ndim + (0 if p.logp is None else 1), _count(p.mask, p.nwalkers), nlags, split, moments)
    m, h = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().kmc_chain_lag_sums(_p(p.chain, C.c_double), _p(p.logp, C.c_double), p.nsamples, p.nwalkers, p.ndim, p.first,
                                             _p(p.mask, C.c_uint8), int(bool(split)), int(lag0), int(nlags), p.device, _p(cm, C.c_double),
                                             _p(cv, C.c_double), _p(lag, C.c_double), C.byref(m), C.byref(h)))
    return _lag_result(cm, cv, lag, m, h, lag0)


def _full_buffers(ncols):
    out = {k: np.empty(ncols) for k in ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse")}
    out["T"] = np.empty(ncols, dtype=np.int64)
    out["flags"] = np.empty(ncols, dtype=np.int32)
    out["info"] = np.zeros(4, dtype=np.int64)
    args = [_p(out[k], C.c_double) for k in ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse")] + [_p(out["T"], C.c_int64), _p(out["flags"], C.c_int32)]
    return out, args


def sampler_convergence_raw(s, first_sample=0, walkers=None, split=True, logp=False, max_lag=None):
    """Everything ``kmc_sampler_convergence`` returns: the arrays of :func:`convergence_stats` plus ``m``, ``h`` and ``info`` (lags
    computed, blocks of 32 lags run, bytes of the chain loaded by the lag kernel and by the moment kernels)."""
    mask = walker_mask(walkers, s.nlocal)
    out, args = _full_buffers(s.ndim + (1 if logp else 0))
    m, h = C.c_int64(), C.c_int64()
    _lib.check(s._L.kmc_sampler_convergence(s._h, int(first_sample), _p(mask, C.c_uint8), int(bool(split)), int(bool(logp)), _max_lag_arg(max_lag), *args,
                                            C.byref(m), C.byref(h), _p(out["info"], C.c_int64)))
    out["m"], out["h"] = m.value, h.value
    return out


def chain_convergence_raw(thetas, logdensities=None, first_sample=0, walkers=None, split=True, max_lag=None, device=0):
    """The same for a chain in host memory (``kmc_chain_convergence``)."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    out, args = _full_buffers(p.ndim + (0 if p.logp is None else 1))
    m, h = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().kmc_chain_convergence(_p(p.chain, C.c_double), _p(p.logp, C.c_double), p.nsamples, p.nwalkers, p.ndim, p.first,
                                                _p(p.mask, C.c_uint8), int(bool(split)), _max_lag_arg(max_lag), p.device, *args, C.byref(m), C.byref(h),
                                                _p(out["info"], C.c_int64)))
    out["m"], out["h"] = m.value, h.value
    return out


def columns(raw):
    """The public dict of columns from what the library returned: ``mean, std = sqrt(var_plus), rhat, ess, mcse, lag`` (the ``T`` of
    the truncation rule), ``truncated`` (the rule had not fired at ``max_lag``), ``m``, ``h``."""
    with np.errstate(invalid="ignore"):
        std = np.sqrt(raw["var_plus"])
    return {"mean": raw["mean"], "std": std, "rhat": raw["rhat"], "ess": raw["ess"], "mcse": raw["mcse"], "lag": raw["T"],
            "truncated": (raw["flags"] & _lib.CONV_TRUNCATED) != 0, "m": raw["m"], "h": raw["h"]}


def convergence(thetas, logdensities=None, first_sample: int = 0, walkers=None, split: bool = True, max_lag=None, device: int = 0):
    """Split-R-hat, effective sample size and Monte-Carlo standard error per dimension of ``thetas[walker][sample](dim)`` (and, as a
    last column, of ``logdensities`` when given), over the samples ``>= first_sample`` of the walkers ``walkers``: a dict of columns
    ``mean, std, rhat, ess, mcse, lag, truncated`` and the numbers ``m`` (chains) and ``h`` (samples per chain).

    Every selected walker is a chain, cut into halves with ``split``.  ``rhat = sqrt(var_plus / W)`` compares the variance between
    the chains with the variance within them; ``ess = m h / (1 + 2 sum_{t <= T} rho_t)`` with the autocorrelations ``rho_t`` from the
    variogram and ``T`` the first odd lag at which ``rho_(T+1) + rho_(T+2) < 0``, or ``truncated`` at ``max_lag`` (default
    ``min(h - 1, 1024)``); ``mcse = std / sqrt(ess)``.  A constant column gives NaN; NaN in the chain propagates.

    The walkers of ONE emcee ensemble are not independent (https://dfm.io/posts/autocorr/: "you should not compute the G-R statistic
    using multiple chains in the same emcee ensemble"), so R-hat over them is optimistic: for R-hat use separate runs
    (:func:`evaluate_convergence`) or the independent chains of ``metropolis_chains``."""
    return columns(chain_convergence_raw(thetas, logdensities, first_sample, walkers, split, max_lag, device))


def _as3(thetas):
    th = np.asarray(thetas, dtype=np.float64)
    if th.ndim == 2:
        th = th[:, :, None]
    if th.ndim != 3:
        raise ValueError("thetas must be [walker][sample] or [walker][sample][dim]")
    return th


def evaluate_convergence(*runs, indices=None, walkernr=None, split: bool = True, device: int = 0):
    """Reference ``src/analysis.jl:79-95`` (commented out there): ``(Rs, sample_size, nthin)`` -- R-hat (should be < 1.1) and the
    total effective sample size of all chains combined, per dimension of ``indices`` (all by default), and the average thinning
    factor ``round(n * nwalkers / mean(sample_size))`` (-1 when that is NaN).

    ``runs`` are the ``thetas`` of separate runs of one posterior; their walkers are concatenated, and with ``walkernr`` only walker
    ``walkernr`` of each run is used (the reference's choice).  The reference's warning stands: the walkers of one emcee ensemble are
    not independent, so R-hat over the walkers of a single run is optimistic -- "this needs input from two separate emcee runs", or
    Metropolis chains.  See :func:`convergence` for the definition (the reference's MCMCDiagnostics.jl is not followed)."""
    if not runs:
        raise ValueError("at least one run")
    ths = [_as3(t) for t in runs]
    if walkernr is not None:
        ths = [t[int(walkernr):int(walkernr) + 1] for t in ths]
    if any(t.shape[1:] != ths[0].shape[1:] for t in ths):
        raise ValueError("the runs must have the same number of samples and dimensions")
    th = np.concatenate(ths, axis=0)
    out = convergence(th, split=split, device=device)
    idx = np.arange(th.shape[2]) if indices is None else np.atleast_1d(np.asarray(indices, dtype=np.int64))
    Rs, sample_size = out["rhat"][idx], out["ess"][idx]
    nthin = th.shape[1] * th.shape[0] / np.mean(sample_size)
    return Rs, sample_size, -1 if np.isnan(nthin) else int(round(float(nthin)))


def error_of_estimated_mean(thetas, device: int = 0):
    """Reference ``src/analysis.jl:242-248``: ``(mean, error of the mean, std)`` per dimension -- the error is the Monte-Carlo standard
    error ``std / sqrt(ess)`` of :func:`convergence`."""
    out = convergence(thetas, device=device)
    return out["mean"], out["mcse"], out["std"]


def samples_vs_tau(thetas, device: int = 0):
    """Reference ``src/analysis.jl:209-226``: the integrated autocorrelation time of ten log-spaced prefixes of the chain, ``(N,
    taus[len(N), ndim])``, as plotted in https://emcee.readthedocs.io/en/latest/tutorials/autocorr/ (plot ``taus`` against ``N``
    and add the line ``N / 50``)."""
    from .diagnostics import int_acorr
    th = _as3(thetas)
    N = np.round(np.logspace(2, np.log10(th.shape[1]), 10)).astype(np.int64)       # :210
    taus, NN = [], []
    for n in N:
        if n > 3:                                                                  # :217
            tau, _ = int_acorr(th[:, :n], warn=False, device=device)               # :218
            taus.append(tau)
            NN.append(int(min(n, th.shape[1])))
    return np.array(NN, dtype=np.int64), np.array(taus).reshape(len(NN), th.shape[2])
