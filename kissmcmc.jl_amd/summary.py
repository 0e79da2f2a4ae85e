"""Posterior summaries: quantiles, the MAP sample and ``summarize_run`` (reference ``src/analysis.jl:9-42``).

That file is entirely commented out in the reference, so ``summarize_run`` is followed as written and there is no live behaviour
to be bit-compatible with.  The order statistics (and with them every quantile) and the arg-max of the log-densities are computed
on the GPU where the chain lies (``kmc_sampler_order_stats`` / ``kmc_sampler_chain_argmax``; ``kmc_chain_*`` for a chain in host
memory): exact, by radix select over the keys described in ``include/kissmcmc_hip.h``; the chain does not cross to the host.

So are the marginal histograms of a corner plot (:func:`histogram`, :func:`corner`; ``kmc_sampler_histograms`` /
``kmc_chain_histograms``): every selected column's 1-D histogram and every pair's 2-D histogram, exact integer counts by numpy's
binning rule.

And the highest-density intervals (:func:`hdi`; ``kmc_sampler_hdi`` / ``kmc_chain_hdi``): every column sorted on the device by the
sort of the rank statistics and scanned there for the narrowest window of ``floor(p N) + 1`` consecutive draws; both ends are elements
of the chain.

Input layout of the module-level functions: what ``emcee`` / ``metropolis_chains`` return, ``thetas[walker][sample]`` (scalar
walkers) or ``thetas[walker][sample][dim]``, and ``logdensities[walker][sample]``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

MAX_RANKS = 16          # per call of the library (kmc_sampler_order_stats)
MAX_BINS, MAX_BINS_2D, MAX_DIMS_2D = 256, 64, 16       # kmc_sampler_histograms


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


def _hist_buffers(dims, edges, logp, pairs):
    """The arrays one histogram call of the library takes and fills."""
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    ncols = dims.size + (1 if logp else 0)
    if edges.ndim != 2 or edges.shape[0] != ncols or edges.shape[1] < 2:
        raise ValueError(f"edges must be [{ncols}, nbins + 1]")
    B = edges.shape[1] - 1
    c2 = np.zeros((dims.size * (dims.size - 1) // 2, B, B), dtype=np.int64) if pairs else None
    return dims, edges, np.zeros((ncols, B), dtype=np.int64), np.zeros((ncols, 3), dtype=np.int64), c2


class _Provider:
    """The read-outs of a stored chain, written once for the two routes to it.  A route gives ``ndim``, ``nwalkers``, ``nsamples`` (stored)
    and ``call(name, ins, outs, logp, logp_at)``: ``kmc_sampler_<name>`` or ``kmc_chain_<name>`` with the route's leading arguments,
    the call's own inputs ``ins`` and outputs ``outs``; ``logp``: the log-densities take part."""

    def _select(self, first_sample, walkers):
        self.first = int(first_sample)
        self.mask = walker_mask(walkers, self.nwalkers)
        self.nselected = self.nwalkers if self.mask is None else int(np.count_nonzero(self.mask))
        self.n = max(0, self.nsamples - self.first) * self.nselected

    def require_logp(self, logp):
        pass

    def order_stats(self, ranks, logp=False):
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        th = np.empty((ranks.size, self.ndim))
        lp = np.empty(ranks.size) if logp else None
        n = C.c_int64()
        self.call("order_stats", [_p(ranks, C.c_int64), ranks.size], [_p(th, C.c_double), _p(lp, C.c_double), C.byref(n)], logp)
        self.n = n.value
        return th, lp

    def argmax(self):
        th = np.empty(self.ndim)
        lp, k, w = C.c_double(), C.c_int64(), C.c_int64()
        self.call("argmax", [], [C.byref(k), C.byref(w), _p(th, C.c_double), C.byref(lp)], True)
        return th, lp.value, k.value, w.value

    def histograms(self, dims, edges, logp=False, pairs=False):
        """``(counts1[ncols, B], outside[ncols, 3], counts2[npairs, B, B] | None)`` for the chain columns ``dims`` (and the
        log-densities as the last column with ``logp``) and ``edges[ncols, B + 1]``."""
        self.require_logp(logp)
        dims, edges, c1, out, c2 = _hist_buffers(dims, edges, logp, pairs)
        n = C.c_int64()
        self.call("histograms", [_p(dims, C.c_int32), dims.size, _p(edges, C.c_double), edges.shape[1] - 1],
                  [_p(c1, C.c_int64), _p(out, C.c_int64), _p(c2, C.c_int64), C.byref(n)], logp, logp_at=4)
        self.n = n.value
        return c1, out, c2


    def hdi(self, probs, logp=False):
        """``(lo[nprob, ncols], hi[nprob, ncols], start[nprob, ncols], nan_count[ncols], info[6])`` of ``kmc_sampler_hdi`` /
        ``kmc_chain_hdi`` for the probabilities ``probs``; the log-densities are the last column with ``logp``."""
        self.require_logp(logp)
        probs = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        ncols = self.ndim + (1 if logp else 0)
        lo, hi = np.full((probs.size, ncols), np.nan), np.full((probs.size, ncols), np.nan)
        start, nan_count, info = np.full((probs.size, ncols), -1, dtype=np.int64), np.zeros(ncols, dtype=np.int64), np.zeros(6, dtype=np.int64)
        n = C.c_int64()
        self.call("hdi", [_p(probs, C.c_double), probs.size],
                  [_p(lo, C.c_double), _p(hi, C.c_double), _p(start, C.c_int64), C.byref(n), _p(nan_count, C.c_int64), _p(info, C.c_int64)],
                  logp, logp_at=0)
        self.n = n.value
        return lo, hi, start, nan_count, info


class _SamplerProvider(_Provider):
    """The chain a :class:`Sampler` holds on the device (``kmc_sampler_*``)."""

    def __init__(self, sampler, first_sample=0, walkers=None):
        self.s, self.ndim, self.nwalkers, self.nsamples = sampler, sampler.ndim, sampler.nlocal, sampler.samples_done
        self._select(first_sample, walkers)

    def call(self, name, ins, outs, logp=False, logp_at=None):
        """Leading arguments: the handle, ``first``, the mask; ``with_logp`` goes in front of ``ins[logp_at]`` where the call has it."""
        ins = list(ins) if logp_at is None else list(ins[:logp_at]) + [int(bool(logp))] + list(ins[logp_at:])
        fn = getattr(self.s._L, "kmc_sampler_" + ("chain_argmax" if name == "argmax" else name))
        _lib.check(fn(self.s._h, self.first, _p(self.mask, C.c_uint8), *ins, *outs))


class _HostProvider(_Provider):
    """A chain in host memory, uploaded for the call (``kmc_chain_*``)."""

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
        self.device = int(device)
        self._select(first_sample, walkers)

    def require_logp(self, logp):
        if logp and self.logp is None:
            raise ValueError("no logdensities were given")

    def call(self, name, ins, outs, logp=False, logp_at=None):
        """Leading arguments: chain, log-densities (when they take part), sizes, ``first``, the mask; ``device`` follows ``ins``."""
        self.require_logp(logp)
        fn = getattr(_lib.lib(), "kmc_chain_" + name)
        _lib.check(fn(_p(self.chain, C.c_double), _p(self.logp if logp else None, C.c_double), self.nsamples, self.nwalkers, self.ndim, self.first,
                      _p(self.mask, C.c_uint8), *ins, self.device, *outs))


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


# ---- highest-density intervals ----------------------------------------------------------------------------------------------------

MAX_PROBS = 16          # per call of the library (kmc_sampler_hdi)


def hdi_span(n: int, prob: float):
    """``(k, nwindows)`` for ``n`` draws and the probability ``prob``: ``k = floor(prob * n)`` in double and ``nwindows = n - k``, with
    the library's refusals (``kmc_hdi_span``; needs no device): ``prob`` finite in (0, 1), ``n >= 2``, ``1 <= k <= n - 1``."""
    k, w = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().kmc_hdi_span(int(n), float(prob), C.byref(k), C.byref(w)))
    return k.value, w.value


def hdi_from(provider, prob=0.94, logp=False, with_info=False):
    """:func:`hdi` from a provider (``.hdi(probs, logp)``)."""
    scalar = np.ndim(prob) == 0
    probs = np.atleast_1d(np.asarray(prob, dtype=np.float64))
    if probs.ndim != 1:
        raise ValueError("prob must be a scalar or a 1-D sequence of probabilities")
    lo, hi, start, nan_count, info = provider.hdi(probs, logp)
    k = np.array([hdi_span(provider.n, p)[0] for p in probs.tolist()], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        width = hi - lo
    out = {"lo": lo, "hi": hi, "width": width, "start": start, "k": k}
    if scalar:
        out = {key: v[0] for key, v in out.items()}
        out["k"] = int(out["k"])
    out.update(n=provider.n, has_nan=nan_count > 0)
    if with_info:
        out.update(nan_count=nan_count, info=info)
    return out


def hdi(thetas, prob=0.94, logdensities=None, first_sample: int = 0, walkers=None, device: int = 0):
    """Highest-density intervals per dimension of ``thetas[walker][sample](dim)`` (and, as a last column, of ``logdensities`` when
    given), over the samples ``>= first_sample`` of the walkers ``walkers``: the narrowest interval ``[x_(i), x_(i + k)]`` of the
    sorted draws with ``k = floor(prob * N)``, the smallest ``i`` among equal widths (ArviZ's unimodal rule; ``include/kissmcmc_hip.h``
    has the definition), sorted and scanned on the GPU.  A dict ``lo, hi, width, start, k, n, has_nan``: arrays ``[ncols]`` for a
    scalar ``prob``, ``[nprob, ncols]`` for a sequence of up to 16; both ends are elements of the chain, bit for bit; a column that
    holds a NaN gets NaN ends, ``start = -1`` and ``has_nan``."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return hdi_from(p, prob, logp=p.logp is not None)


# ---- marginal histograms and the corner table ------------------------------------------------------------------------------------

def pair_list(ndims: int):
    """The pairs ``(a, b)``, ``a < b``, of positions in a list of ``ndims`` dimensions, in the library's order:
    ``(0, 1), (0, 2), ..., (1, 2), ...``."""
    return [(a, b) for a in range(ndims) for b in range(a + 1, ndims)]


def hist_edges(provider, bins, range=None, quantile_range=None, dims=None, logp=False):
    """``(dims, edges[ncols, B + 1])`` for a histogram call: the selected chain columns (all by default) and, with ``logp``, the
    log-densities as the last column.  ``bins``: a bin count, an edge array ``[B + 1]`` shared by all columns, or ``[ncols, B + 1]``.
    With a count the limits are ``range`` (``(lo, hi)`` or ``[ncols, 2]``), else the quantiles ``quantile_range = (q_lo, q_hi)``, else
    each column's minimum and maximum, both exact, from the provider's order statistics; equal limits are widened by 0.5 either way
    and ``edges = np.linspace(lo, hi, B + 1)``, as ``np.histogram`` does."""
    dims = np.arange(provider.ndim) if dims is None else np.atleast_1d(np.asarray(dims, dtype=np.int64))
    if dims.ndim != 1 or dims.size == 0:
        raise ValueError("dims must be a non-empty list of dimensions")
    if np.any(dims < 0) or np.any(dims >= provider.ndim):
        raise IndexError(f"dimension outside [0, {provider.ndim})")
    ncols = dims.size + (1 if logp else 0)
    if np.ndim(bins) > 0:
        e = np.asarray(bins, dtype=np.float64)
        if e.ndim == 1:
            e = np.broadcast_to(e, (ncols, e.size))
        if e.ndim != 2 or e.shape[0] != ncols or e.shape[1] < 2:
            raise ValueError(f"bin edges must be [nbins + 1] or [{ncols}, nbins + 1]")
        return dims, np.ascontiguousarray(e)
    B = int(bins)
    if B < 1:
        raise ValueError("bins must be at least 1")
    if range is not None:
        lim = np.asarray(range, dtype=np.float64)
        lim = np.broadcast_to(lim, (ncols, 2)) if lim.shape == (2,) else lim
        if lim.shape != (ncols, 2):
            raise ValueError(f"range must be (lo, hi) or [{ncols}, 2]")
        lo, hi = lim[:, 0].copy(), lim[:, 1].copy()
    else:
        if quantile_range is not None:
            if len(quantile_range) != 2:
                raise ValueError("quantile_range must be (q_lo, q_hi)")
            got = quantiles_from(provider, list(quantile_range), logp=logp)
            th, lp = got if logp else (got, None)
        else:
            if provider.n < 1:
                provider.order_stats(np.zeros(1, dtype=np.int64), logp)      # the library's own refusal of an empty selection
                raise ValueError("the selection is empty")
            th, lp = provider.order_stats(np.array([0, provider.n - 1], dtype=np.int64), logp)
        lo, hi = th[0, dims], th[1, dims]
        if logp:
            lo, hi = np.append(lo, lp[0]), np.append(hi, lp[1])
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("the range of a column is not finite")            # (np.histogram: "autodetected range ... is not finite")
    if np.any(lo > hi):
        raise ValueError("max must be larger than min in range")
    same = lo == hi
    lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)        # numpy's _get_outer_edges
    return dims, np.stack([np.linspace(l, h, B + 1) for l, h in zip(lo.tolist(), hi.tolist())])


def histogram_from(provider, bins=40, range=None, quantile_range=None, dims=None, logp=False):
    """:func:`histogram` from a provider (``.n``, ``.ndim``, ``.order_stats(ranks, logp)``, ``.histograms(dims, edges, logp, pairs)``)."""
    dims, edges = hist_edges(provider, bins, range, quantile_range, dims, logp)
    counts, outside, _ = provider.histograms(dims, edges, logp, False)
    return counts, edges, outside


def corner_from(provider, bins=32, range=None, quantile_range=None, dims=None):
    """:func:`corner` from a provider."""
    dims, edges = hist_edges(provider, bins, range, quantile_range, dims, False)
    counts, outside, h2 = provider.histograms(dims, edges, False, True)
    pairs = [(int(dims[a]), int(dims[b])) for a, b in pair_list(dims.size)]
    return {"dims": dims.tolist(), "pairs": pairs, "edges": edges, "hist1d": counts, "outside": outside, "hist2d": h2, "n": provider.n}


def histogram(thetas, bins=40, range=None, quantile_range=None, dims=None, logdensities=None, first_sample: int = 0, walkers=None,
              device: int = 0):
    """1-D marginal histograms of ``thetas[walker][sample](dim)``, counted on the GPU in one read of the chain:
    ``(counts[ncols, B], edges[ncols, B + 1], outside[ncols, 3])``, ``int64`` counts, one row per dimension of ``dims`` (all by
    default, in the order given) and, with ``logdensities``, one more for them.  An element ``x`` is in bin ``i`` iff
    ``e[i] <= x < e[i + 1]``, the last bin closed; ``outside`` counts what lies below ``e[0]``, above ``e[B]`` and the NaNs.
    With a bin count and no range the result is ``np.histogram(column, bins=B)``, counts and edges; see :func:`hist_edges` for
    ``bins``, ``range`` and ``quantile_range``.  The selection is that of :func:`quantiles`."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return histogram_from(p, bins, range, quantile_range, dims, logp=logdensities is not None)


def corner(thetas, bins=32, range=None, quantile_range=None, dims=None, first_sample: int = 0, walkers=None, device: int = 0):
    """The numbers of a corner plot, counted on the GPU: a dict ``dims`` (the selected dimensions, 2 to 16), ``pairs`` (the pairs of
    dimensions ``(a, b)`` in list order: first with second, first with third, ...), ``edges[ndims, B + 1]``, ``hist1d[ndims, B]``,
    ``outside[ndims, 3]``, ``hist2d[npairs, B, B]`` (``np.histogram2d(x_a, x_b, bins=[e_a, e_b])``, ``B <= 64``) and ``n``, the number
    of selected samples.  ``bins``, ``range`` and ``quantile_range`` as in :func:`histogram`."""
    return corner_from(_HostProvider(thetas, None, first_sample, walkers, device), bins, range, quantile_range, dims)


def hist_mode(counts, edges):
    """The centre of the fullest bin, the first one on ties: a scalar for ``counts[B]``, ``edges[B + 1]``; one value per row for
    ``counts[ncols, B]``, ``edges[ncols, B + 1]``."""
    c, e = np.asarray(counts), np.asarray(edges, dtype=np.float64)
    if c.ndim == 1:
        i = int(np.argmax(c))
        return 0.5 * (e[i] + e[i + 1])
    i = np.argmax(c, axis=1)
    r = np.arange(c.shape[0])
    return 0.5 * (e[r, i] + e[r, i + 1])


def credible_levels(hist2d, levels=(0.393, 0.865)):
    """For contour drawing: per level ``p`` the largest count ``t`` such that the bins with at least ``t`` counts -- the super-level
    set -- hold at least the share ``p`` of the histogram's mass (0.393 and 0.865: the 1- and 2-sigma contours of a 2-D Gaussian).
    Returns an array like ``levels``."""
    h = np.sort(np.asarray(hist2d).ravel())[::-1]
    cum = np.cumsum(h)
    if h.size == 0 or cum[-1] <= 0:
        raise ValueError("the histogram is empty")
    p = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if np.any(~((p > 0.0) & (p <= 1.0))):
        raise ValueError("levels must lie in (0, 1]")
    idx = np.minimum(np.searchsorted(cum, p * cum[-1], side="left"), h.size - 1)
    return h[idx]


def summary_columns(names, median, mean, std, mode=None, theta_true=None, eff_samples=None, convergence=None, hdi=None):
    """The table of ``summarize_run`` (reference ``src/analysis.jl:14-38``) as a dict of columns, in the reference's order:
    ``var, [err,] median, mean, mode, std[, eff_samples]``; then ``rhat, ess, mcse`` when ``convergence`` (the dict of
    :func:`kissmcmc_jl_amd.convergence`) is given, and ``rhat_rank, ess_bulk, ess_tail`` when it holds them (``rank=True``); then
    ``hdi_lo, hdi_hi`` when ``hdi`` (the dict of :func:`kissmcmc_jl_amd.hdi` for one probability) is given."""
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
    if convergence is not None:
        for k in ("rhat", "ess", "mcse", "rhat_rank", "ess_bulk", "ess_tail"):
            if k in convergence:
                cols[k] = np.asarray(convergence[k], dtype=np.float64)[:nt]
    if hdi is not None:
        cols["hdi_lo"], cols["hdi_hi"] = hdi["lo"][:nt], hdi["hi"][:nt]
    return cols


def summarize_run(thetas, logdensities=None, theta_true=None, names=None, eff_samples=None, provider=None, device: int = 0,
                  convergence=False, covariance=False, hdi=None, quantile_mcse=False):
    """Summary statistics of a run, reference ``src/analysis.jl:9-42`` (commented out there; followed as written): a dict of columns
    ``var`` (the names, ``"1" .. "ndim"`` by default), ``err = |theta_true - median|`` (only with ``theta_true``), ``median``,
    ``mean``, ``mode``, ``std`` (Julia's: n - 1 in the denominator) and ``eff_samples`` (only when given, passed through).

    ``mode`` is the MAP sample -- the stored sample of the largest log-density -- when ``logdensities`` are given, else None.  (The
    reference takes ``mode`` as an argument; its line 24 tests ``mod==nothing``, the function ``mod``, where line 35 tests
    ``mode==nothing``: read as ``mode``.)  The median and the MAP sample come from the device; ``provider`` replaces the device as
    the source of order statistics and arg-max (tests).

    ``convergence=True`` adds the columns ``rhat``, ``ess`` and ``mcse`` of :func:`kissmcmc_jl_amd.convergence` (split chains, every
    walker a chain; computed on the device); ``convergence="rank"`` also ``rhat_rank``, ``ess_bulk`` and ``ess_tail`` of
    :func:`kissmcmc_jl_amd.rank_convergence`.  ``covariance=True`` adds the matrices ``cov`` and ``corr`` of
    :func:`kissmcmc_jl_amd.covariance` (of the dimensions; summed on the device).  ``hdi=0.94`` adds the columns ``hdi_lo`` and
    ``hdi_hi`` of :func:`kissmcmc_jl_amd.hdi` for that probability.  ``quantile_mcse=True`` adds the column ``median_mcse``, the
    Monte-Carlo standard error of the median of :func:`kissmcmc_jl_amd.quantile_mcse` (split chains, every walker a chain)."""
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
    conv = None
    if convergence:
        from .chain_convergence import convergence as _convergence
        conv = _convergence(th, device=device, rank=convergence == "rank")
    intervals = None if hdi is None else hdi_from(provider, float(hdi))
    cols = summary_columns(names, median, flat.mean(axis=0), std, mode, theta_true, eff_samples, conv, intervals)
    if quantile_mcse:
        from .chain_convergence import quantile_mcse as _quantile_mcse
        cols["median_mcse"] = _quantile_mcse(th, [0.5], device=device)["mcse"][0]
    if covariance:
        from .chain_covariance import covariance as _covariance
        c = _covariance(th, device=device)
        cols.update(cov=c["cov"], corr=c["corr"])
    return cols
