"""Posterior summaries: quantiles, the MAP sample and ``summarize_run`` (reference ``src/analysis.jl:9-42``).

That file is entirely commented out in the reference, so ``summarize_run`` is followed as written and there is no live behaviour
to be bit-compatible with.  The order statistics (and with them every quantile) and the arg-max of the log-densities are computed
on the GPU where the chain lies (``kmc_sampler_order_stats`` / ``kmc_sampler_chain_argmax``; ``kmc_chain_*`` for a chain in host
memory): exact, by radix select over the keys described in ``include/kissmcmc_hip.h``; the chain does not cross to the host.

Input layout of the module-level functions: what ``emcee`` / ``metropolis_chains`` return, ``thetas[walker][sample]`` (scalar
walkers) or ``thetas[walker][sample][dim]``, and ``logdensities[walker][sample]``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

MAX_RANKS = 16          # per call of the library (kmc_sampler_order_stats)


def quantile_ranks(q, n: int):
    """For ``q`` in [0, 1] and ``n`` sorted values: ``(lo, hi, frac)`` with ``h = q (n - 1)``, ``lo = floor(h)``,
    ``hi = min(lo + 1, n - 1)``, ``frac = h - lo`` -- the quantile is ``x[lo] + frac (x[hi] - x[lo])`` (numpy's "linear")."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    if q.ndim != 1 or np.any(~((q >= 0.0) & (q <= 1.0))):
        raise ValueError("q must be a scalar or a 1-D sequence of values in [0, 1]")
    h = q * (n - 1)
    lo = np.floor(h).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    return lo, hi, h - lo


def interpolate(x_lo, x_hi, frac):
    """``x_lo + frac (x_hi - x_lo)``, and exactly ``x_lo`` where ``frac == 0`` (also when the two are infinite).
    ``x_*``: ``[nq, ...]``, ``frac``: ``[nq]``."""
    x_lo, x_hi = np.asarray(x_lo, dtype=np.float64), np.asarray(x_hi, dtype=np.float64)
    f = np.asarray(frac, dtype=np.float64).reshape((-1,) + (1,) * (x_lo.ndim - 1))
    with np.errstate(invalid="ignore"):
        return np.where(f == 0.0, x_lo, x_lo + f * (x_hi - x_lo))


def walker_mask(walkers, nwalkers: int):
    """``walkers`` (None, a boolean mask of length ``nwalkers`` or an array of walker indices) as the library's byte mask, or None."""
    if walkers is None:
        return None
    w = np.asarray(walkers)
    if w.dtype == np.bool_:
        if w.shape != (nwalkers,):
            raise ValueError(f"a boolean walker mask must have shape ({nwalkers},)")
        return np.ascontiguousarray(w, dtype=np.uint8)
    idx = w.astype(np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= nwalkers):
        raise IndexError("walker index out of range")
    m = np.zeros(nwalkers, dtype=np.uint8)
    m[idx] = 1
    return m


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


class _SamplerProvider:
    """Order statistics and arg-max of the chain a :class:`Sampler` holds on the device."""

    def __init__(self, sampler, first_sample=0, walkers=None):
        self.s, self.first = sampler, int(first_sample)
        self.ndim = sampler.ndim
        self.mask = walker_mask(walkers, sampler.nlocal)
        nw = sampler.nlocal if self.mask is None else int(np.count_nonzero(self.mask))
        self.n = max(0, sampler.samples_done - self.first) * nw

    def order_stats(self, ranks, logp=False):
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        th = np.empty((ranks.size, self.ndim))
        lp = np.empty(ranks.size) if logp else None
        n = C.c_int64()
        _lib.check(self.s._L.kmc_sampler_order_stats(self.s._h, self.first, _p(self.mask, C.c_uint8), _p(ranks, C.c_int64), ranks.size,
                                                     _p(th, C.c_double), _p(lp, C.c_double), C.byref(n)))
        self.n = n.value
        return th, lp

    def argmax(self):
        th = np.empty(self.ndim)
        lp, k, w = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(self.s._L.kmc_sampler_chain_argmax(self.s._h, self.first, _p(self.mask, C.c_uint8), C.byref(k), C.byref(w),
                                                      _p(th, C.c_double), C.byref(lp)))
        return th, lp.value, k.value, w.value


class _HostProvider:
    """The same on a chain in host memory (``kmc_chain_order_stats`` / ``kmc_chain_argmax`` upload it)."""

    def __init__(self, thetas, logdensities=None, first_sample=0, walkers=None, device=0):
        th = np.asarray(thetas, dtype=np.float64)
        if th.ndim == 2:
            th = th[:, :, None]
        if th.ndim != 3:
            raise ValueError("thetas must be [walker][sample] or [walker][sample][dim]")
        self.nwalkers, self.nsamples, self.ndim = th.shape
        self.chain = np.ascontiguousarray(th.transpose(1, 0, 2))                   # [sample][walker][dim], the device chain layout
        self.logp = None
        if logdensities is not None:
            lp = np.asarray(logdensities, dtype=np.float64)
            if lp.shape != (self.nwalkers, self.nsamples):
                raise ValueError("logdensities must be [walker][sample], like thetas")
            self.logp = np.ascontiguousarray(lp.T)
        self.first, self.device = int(first_sample), int(device)
        self.mask = walker_mask(walkers, self.nwalkers)
        nw = self.nwalkers if self.mask is None else int(np.count_nonzero(self.mask))
        self.n = max(0, self.nsamples - self.first) * nw

    def order_stats(self, ranks, logp=False):
        if logp and self.logp is None:
            raise ValueError("no logdensities were given")
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        th = np.empty((ranks.size, self.ndim))
        lp = np.empty(ranks.size) if logp else None
        n = C.c_int64()
        _lib.check(_lib.lib().kmc_chain_order_stats(_p(self.chain, C.c_double), _p(self.logp, C.c_double), self.nsamples, self.nwalkers, self.ndim,
                                                    self.first, _p(self.mask, C.c_uint8), _p(ranks, C.c_int64), ranks.size, self.device,
                                                    _p(th, C.c_double), _p(lp, C.c_double), C.byref(n)))
        self.n = n.value
        return th, lp

    def argmax(self):
        if self.logp is None:
            raise ValueError("no logdensities were given")
        th = np.empty(self.ndim)
        lp, k, w = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().kmc_chain_argmax(_p(self.chain, C.c_double), _p(self.logp, C.c_double), self.nsamples, self.nwalkers, self.ndim,
                                               self.first, _p(self.mask, C.c_uint8), self.device, C.byref(k), C.byref(w), _p(th, C.c_double),
                                               C.byref(lp)))
        return th, lp.value, k.value, w.value


def quantiles_from(provider, q, logp=False):
    """Quantiles ``q`` from a provider of order statistics (``.n``, ``.ndim``, ``.order_stats(ranks, logp)``): the two order
    statistics of every quantile come from the provider (at most :data:`MAX_RANKS` distinct ranks per call), the interpolation
    ``x_lo + frac (x_hi - x_lo)`` is done here.  Returns ``[len(q), ndim]``, and ``[len(q)]`` for the log-densities when asked."""
    if provider.n < 1:
        provider.order_stats(np.zeros(1, dtype=np.int64), logp)      # the library's own refusal of an empty selection
        raise ValueError("the selection is empty")
    lo, hi, frac = quantile_ranks(q, provider.n)
    ranks = np.unique(np.concatenate([lo, hi]))
    th = np.empty((ranks.size, provider.ndim))
    lp = np.empty(ranks.size) if logp else None
    for i in range(0, ranks.size, MAX_RANKS):
        t, l = provider.order_stats(ranks[i:i + MAX_RANKS], logp)
        th[i:i + MAX_RANKS] = t
        if logp:
            lp[i:i + MAX_RANKS] = l
    ilo, ihi = np.searchsorted(ranks, lo), np.searchsorted(ranks, hi)
    out = interpolate(th[ilo], th[ihi], frac)
    return (out, interpolate(lp[ilo], lp[ihi], frac)) if logp else out


def quantiles(thetas, q, logdensities=None, first_sample: int = 0, walkers=None, device: int = 0):
    """Quantiles ``q`` (values in [0, 1]) per dimension of ``thetas[walker][sample](dim)``, over the samples ``>= first_sample`` of
    the walkers ``walkers`` (all; a boolean mask or indices): ``[len(q), ndim]``; with ``logdensities`` also their quantiles,
    ``[len(q)]``.  The order statistics are exact (selected on the GPU); the value is numpy's ``linear`` quantile,
    ``x_lo + frac (x_hi - x_lo)`` of :func:`quantile_ranks`."""
    return quantiles_from(_HostProvider(thetas, logdensities, first_sample, walkers, device), q, logp=logdensities is not None)


def map_sample(thetas, logdensities, first_sample: int = 0, walkers=None, device: int = 0):
    """The stored sample of the largest log-density: ``(theta[ndim], logp, sample, walker)``; ties go to the smallest sample, then the
    smallest walker; NaN log-densities are ignored."""
    return _HostProvider(thetas, logdensities, first_sample, walkers, device).argmax()


def summary_columns(names, median, mean, std, mode=None, theta_true=None, eff_samples=None):
    """The table of ``summarize_run`` (reference ``src/analysis.jl:14-38``) as a dict of columns, in the reference's order:
    ``var, [err,] median, mean, mode, std[, eff_samples]``."""
    median, mean, std = (np.asarray(a, dtype=np.float64) for a in (median, mean, std))
    nt = median.size
    names = [str(i + 1) for i in range(nt)] if names is None else [str(v) for v in names]          # :9 names=["$i" for i=1:nt]
    if len(names) != nt:
        raise ValueError("one name per dimension")
    cols = {"var": names}
    if theta_true is not None and np.size(theta_true) > 0:                                         # :13
        t = np.asarray(theta_true, dtype=np.float64).ravel()
        if t.size != nt:
            raise ValueError("theta_true must have one value per dimension")
        cols["err"] = np.abs(t - median)                                                           # :21
    cols["median"] = median
    cols["mean"] = mean
    cols["mode"] = None if mode is None else np.asarray(mode, dtype=np.float64)                   # :24, :35
    cols["std"] = std
    if eff_samples is not None:
        cols["eff_samples"] = np.asarray(eff_samples)                                              # :26, :37
    return cols


def summarize_run(thetas, logdensities=None, theta_true=None, names=None, eff_samples=None, provider=None, device: int = 0):
    """Summary statistics of a run, reference ``src/analysis.jl:9-42`` (commented out there; followed as written): a dict of columns
    ``var`` (the names, ``"1" .. "ndim"`` by default), ``err = |theta_true - median|`` (only with ``theta_true``), ``median``,
    ``mean``, ``mode``, ``std`` (Julia's: n - 1 in the denominator) and ``eff_samples`` (only when given, passed through).

    ``mode`` is the MAP sample -- the stored sample of the largest log-density -- when ``logdensities`` are given, else None.  (The
    reference takes ``mode`` as an argument; its line 24 tests ``mod==nothing``, the function ``mod``, where line 35 tests
    ``mode==nothing``: read as ``mode``.)  The median and the MAP sample come from the device; ``provider`` replaces the device as
    the source of order statistics and arg-max (tests)."""
    th = np.asarray(thetas, dtype=np.float64)
    if th.ndim == 2:
        th = th[:, :, None]
    if th.ndim != 3:
        raise ValueError("thetas must be [walker][sample] or [walker][sample][dim]")
    if provider is None:
        provider = _HostProvider(th, logdensities, device=device)
    flat = th.reshape(-1, th.shape[2])
    median = quantiles_from(provider, [0.5])[0]
    mode = provider.argmax()[0] if logdensities is not None else None
    std = flat.std(axis=0, ddof=1) if flat.shape[0] > 1 else np.full(flat.shape[1], np.nan)
    return summary_columns(names, median, flat.mean(axis=0), std, mode, theta_true, eff_samples)
