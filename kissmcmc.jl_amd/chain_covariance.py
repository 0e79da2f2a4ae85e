"""The posterior covariance and correlation matrix of a stored chain, summed on the device where the chain lies.

``mean[c]`` and ``cov[a][b] = sum_r (x[r][a] - mean[a]) (x[r][b] - mean[b]) / (n - 1)`` over the selected rows (``kmc_sampler_covariance``
/ ``kmc_chain_covariance``: two passes, the cross products on the double-precision matrix instruction; ``include/kissmcmc_hip.h`` has
the definition), then ``corr[a][b] = cov[a][b] / (sqrt(cov[a][a]) sqrt(cov[b][b]))`` on the host in a fixed order of operations
(``kmc_cov_correlation``).

Input layout of the module-level functions: what ``emcee`` / ``metropolis_chains`` return, ``thetas[walker][sample]`` (scalar walkers)
or ``thetas[walker][sample][dim]``, and ``logdensities[walker][sample]``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .summary import _HostProvider, _SamplerProvider, _p

MAX_COLS = 1024         # of one matrix (kmc_sampler_covariance)


def cov_plan(ncols: int):
    """The cut of the product kernel for ``ncols`` columns (``kmc_cov_plan``; needs no device): dict ``tile_cols, strip_tiles,
    nstrips, rows_per_wave_block``."""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.lib().kmc_cov_plan(int(ncols), *[C.byref(x) for x in v]))
    return dict(zip(("tile_cols", "strip_tiles", "nstrips", "rows_per_wave_block"), [x.value for x in v]))


def correlation(cov):
    """The host stage (``kmc_cov_correlation``; needs no device): ``(corr[C, C], std[C])`` of ``cov[C, C]`` with ``std = sqrt(diag)``
    and ``corr[a, b] = cov[a, b] / (std[a] * std[b])``, the diagonal exactly 1.0 where the variance is finite and positive; a constant
    column gives NaN."""
    c = np.ascontiguousarray(cov, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 1:
        raise ValueError("cov must be a square matrix")
    corr, std = np.empty_like(c), np.empty(c.shape[0])
    _lib.check(_lib.lib().kmc_cov_correlation(c.shape[0], _p(c, C.c_double), _p(corr, C.c_double), _p(std, C.c_double)))
    return corr, std


def covariance_raw_from(p, logp=False):
    """``mean, cov, n`` and ``info`` (rows walked, partial sums per entry, strips, bytes of the chain loaded) from a provider
    (``summary._SamplerProvider``, ``summary._HostProvider``): ``kmc_sampler_covariance`` / ``kmc_chain_covariance``."""
    ncols = p.ndim + (1 if logp else 0)
    mean, cov = np.full(ncols, np.nan), np.full((ncols, ncols), np.nan)
    n, info = C.c_int64(), np.zeros(4, dtype=np.int64)
    p.call("covariance", [], [_p(mean, C.c_double), _p(cov, C.c_double), C.byref(n), _p(info, C.c_int64)], logp, logp_at=0)
    return {"mean": mean, "cov": cov, "n": n.value, "info": info}


def covariance_from(p, logp=False):
    """:func:`covariance` from a provider."""
    raw = covariance_raw_from(p, logp)
    corr, std = correlation(raw["cov"])
    return {"mean": raw["mean"], "cov": raw["cov"], "corr": corr, "std": std, "n": raw["n"]}


def sampler_covariance(s, first_sample=0, walkers=None, logp=False):
    """:func:`covariance` on the chain a :class:`Sampler` holds (``kmc_sampler_covariance``)."""
    return covariance_from(_SamplerProvider(s, first_sample, walkers), logp)


def covariance(thetas, logdensities=None, first_sample: int = 0, walkers=None, device: int = 0):
    """The covariance matrix of the posterior sample ``thetas[walker][sample](dim)`` (and, as a last column, of ``logdensities`` when
    given), over the samples ``>= first_sample`` of the walkers ``walkers``, summed on the GPU: a dict ``mean[C]``, ``cov[C, C]``
    (``n - 1`` in the denominator, centred on ``mean``; symmetric bit for bit), ``corr[C, C]``, ``std[C]`` and ``n``, the number of
    rows.  At most 1024 columns, at least 2 rows.  NaN and inf in a selected row propagate into the entries of their columns and into
    no others; a constant column has NaN correlations.  Equal calls return equal bits."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return covariance_from(p, p.logp is not None)
