"""Pointwise log-likelihoods of a :class:`DataDensity` over a stored chain, and WAIC, on the device where the chain, the observations
and the compiled term are.

``l[r][j] = term(x_r, d_j)`` over the selected rows ``r`` (the stored samples ``first_sample, first_sample + thin, ...`` of the walkers
``walkers``) and the observations ``j`` is reduced per observation in two passes (``kmc_sampler_pointwise_stats`` /
``kmc_chain_pointwise_stats``): ``M_j = max_r l``, ``S1_j = sum_r l``, then ``E_j = sum_r exp(l - M_j)`` and
``V_j = sum_r (l - S1_j / n)^2``.  The host stage (``kmc_waic_stats``) turns them into ``lppd_j = M_j + (log E_j - log n)``,
``p_waic_j = V_j / (n - 1)``, ``elpd_j = lppd_j - p_waic_j`` and their totals; ``include/kissmcmc_hip.h`` has the definitions.  The
``n - 1`` is BDA3's and the R package ``loo``'s; ArviZ divides by ``n``.

Input layout of the module-level functions: what ``emcee`` returns, ``thetas[walker][sample]`` (scalar walkers) or
``thetas[walker][sample][dim]``; or the pair ``(chain[sample][walker][dim], logp)`` that :meth:`Sampler.chain` returns.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .densities import DataDensity
from .summary import _HostProvider, _SamplerProvider, _p

TOTALS = ("lppd", "p_waic", "elpd_waic", "se", "waic", "n_high", "n_nan")


def pointwise_plan(n: int, ndata: int):
    """The cut of the two passes for ``n`` rows and ``ndata`` observations (``kmc_pointwise_plan``; needs no device): dict ``run_len,
    nruns, lanes_per_run, slots, nwaves``.  Run ``r`` covers the rows ``[r run_len, min(n, (r + 1) run_len))``; wave ``w`` carries the
    runs ``w slots .. w slots + slots - 1``."""
    v = [C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()]
    _lib.check(_lib.lib().kmc_pointwise_plan(int(n), int(ndata), *[C.byref(x) for x in v]))
    return dict(zip(("run_len", "nruns", "lanes_per_run", "slots", "nwaves"), [x.value for x in v]))


def waic_stats(stats, n: int):
    """The host stage (``kmc_waic_stats``; needs no device): from ``stats[4, J]`` (``M, S1, E, V``) of ``n`` rows a dict ``elpd_waic, se,
    p_waic, lppd, waic, n_high, n_nan, n`` and the arrays ``lppd_j, p_waic_j, elpd_j``."""
    st = np.ascontiguousarray(stats, dtype=np.float64)
    if st.ndim != 2 or st.shape[0] != 4 or st.shape[1] < 1:
        raise ValueError("stats must be [4, J]")
    J = st.shape[1]
    lp, pw, el, tot = np.empty(J), np.empty(J), np.empty(J), np.empty(len(TOTALS))
    _lib.check(_lib.lib().kmc_waic_stats(J, int(n), _p(st, C.c_double), _p(lp, C.c_double), _p(pw, C.c_double), _p(el, C.c_double),
                                         _p(tot, C.c_double)))
    w = dict(zip(TOTALS, tot.tolist()))
    w["n_high"], w["n_nan"] = int(w["n_high"]), int(w["n_nan"])
    w.update(n=int(n), lppd_j=lp, p_waic_j=pw, elpd_j=el)
    return w


def compare_waic(w_a, w_b):
    """The difference of two models' ``elpd_waic`` over the same observations, from the pointwise arrays of two :func:`waic` results
    (needs no device): dict ``elpd_diff = sum_j (elpd_a_j - elpd_b_j)`` (positive: ``a`` predicts better), ``se =
    sqrt(J var(elpd_a_j - elpd_b_j))`` with the sample variance (``J - 1``), and ``J``."""
    return _elpd_difference(w_a["elpd_j"], w_b["elpd_j"])


def _elpd_difference(elpd_a_j, elpd_b_j):
    """``elpd_diff``, ``se`` and ``J`` of two models' pointwise elpd (:func:`compare_waic`, ``compare_loo``)."""
    a, b = np.asarray(elpd_a_j, dtype=np.float64), np.asarray(elpd_b_j, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("the two results are not over the same observations")
    d = a - b
    J = d.size
    return {"elpd_diff": float(d.sum()), "se": float(np.sqrt(J * d.var(ddof=1))) if J > 1 else float("nan"), "J": J}


def _held_out(data):
    """``(array | None, ndata2, ncols2)`` of the ``data=`` argument."""
    if data is None:
        return None, 0, 0
    D = np.asarray(data, dtype=np.float64)
    if D.ndim == 1:
        D = D[:, None]
    if D.ndim != 2:
        raise ValueError("data must be a [ndata, ncols] array")
    return np.ascontiguousarray(D), D.shape[0], D.shape[1]


def _host_provider(pdf, thetas, first_sample, walkers, device):
    if getattr(pdf, "user_handle", None) is None:        # (a runtime-compiled density that is not a DataDensity: the library refuses it)
        raise TypeError("the pointwise log-likelihood needs a DataDensity: other densities have no per-observation term")
    if isinstance(thetas, tuple):                     # Sampler.chain(): (chain[sample][walker][dim], logp)
        thetas = np.asarray(thetas[0], dtype=np.float64).transpose(1, 0, 2)
    p = _HostProvider(thetas, None, first_sample, walkers, device)
    p.pdf = pdf
    p.params = np.zeros(6)
    p.params[:len(pdf.params())] = pdf.params()
    return p


def _nrows(p, thin):
    if thin < 1:
        return 0
    return -(-max(0, p.nsamples - p.first) // int(thin)) * p.nselected


def _call(p, which, thin, data, tail_in, outs):
    """``kmc_sampler_pointwise_<which>`` or ``kmc_chain_pointwise_<which>`` with the route's leading arguments."""
    D, nd2, nc2 = data
    mid = [int(thin), _p(D, C.c_double), nd2, nc2] + list(tail_in)
    if isinstance(p, _SamplerProvider):
        _lib.check(getattr(p.s._L, "kmc_sampler_pointwise_" + which)(p.s._h, p.first, _p(p.mask, C.c_uint8), *mid, *outs))
    else:
        _lib.check(getattr(_lib.lib(), "kmc_chain_pointwise_" + which)(p.pdf.user_handle, _p(p.params, C.c_double), _p(p.chain, C.c_double),
                                                                       p.nsamples, p.nwalkers, p.ndim, p.first, _p(p.mask, C.c_uint8),
                                                                       *mid, p.device, *outs))


def pointwise_stats_from(p, pdf, thin=1, data=None):
    """``stats[4, J]``, ``n`` and ``info`` (rows, runs, terms evaluated, rows of a run, nanoseconds of pass 1 and of pass 2 on the device)
    from a provider."""
    held = _held_out(data)
    J = held[1] if held[0] is not None else (pdf.data.shape[0] if isinstance(pdf, DataDensity) else 1)
    stats = np.full((4, max(J, 1)), np.nan)
    n, info = C.c_int64(), np.zeros(6, dtype=np.int64)
    _call(p, "stats", thin, held, [], [_p(stats, C.c_double), C.byref(n), _p(info, C.c_int64)])
    return {"stats": stats, "n": n.value, "info": info}


def waic_from(p, pdf, thin=1, data=None):
    raw = pointwise_stats_from(p, pdf, thin, data)
    return waic_stats(raw["stats"], raw["n"])


def loglike_from(p, pdf, thin=1, obs=None, data=None):
    held = _held_out(data)
    J = held[1] if held[0] is not None else (pdf.data.shape[0] if isinstance(pdf, DataDensity) else 1)
    first, stop = (0, J) if obs is None else (int(obs[0]), int(obs[1]))
    count = stop - first
    out = np.empty((max(_nrows(p, thin), 1), max(count, 1)))
    n = C.c_int64()
    _call(p, "loglike", thin, held, [first, count], [_p(out, C.c_double), C.byref(n)])
    return out


def sampler_waic(s, first_sample=0, thin=1, walkers=None, data=None):
    """:func:`waic` on the chain a :class:`Sampler` holds (``kmc_sampler_pointwise_stats``)."""
    return waic_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, data)


def sampler_pointwise_loglike(s, first_sample=0, thin=1, walkers=None, obs=None, data=None):
    """:func:`pointwise_loglike` on the chain a :class:`Sampler` holds (``kmc_sampler_pointwise_loglike``)."""
    return loglike_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, obs, data)


def pointwise_stats(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, data=None, device: int = 0):
    """The per-observation statistics themselves (``kmc_chain_pointwise_stats``): dict ``stats[4, J]`` (``M, S1, E, V``), ``n``, ``info``."""
    return pointwise_stats_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, data)


def waic(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, data=None, device: int = 0):
    """WAIC of the :class:`DataDensity` ``pdf`` over the posterior sample ``thetas[walker][sample](dim)`` (uploaded first): the rows are
    the samples ``first_sample, first_sample + thin, ...`` of the walkers ``walkers``, at least 2.  A dict ``elpd_waic, se, p_waic, lppd,
    waic (= -2 elpd_waic), n_high`` (observations with ``p_waic_j > 0.4``), ``n_nan`` (observations with a NaN among their terms),
    ``n`` and the arrays ``lppd_j, p_waic_j, elpd_j``.  ``p_waic_j`` is the sample variance of the terms (``n - 1``, as BDA3 and ``loo``;
    ArviZ divides by ``n``).  With ``data=`` the observations are that held-out array ``[J', ncols]`` instead of the density's own:
    ``lppd`` is then the log predictive density of the test set.  Equal calls return equal bits, and :meth:`Sampler.waic` equals this
    on the downloaded chain bit for bit."""
    return waic_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, data)


def pointwise_loglike(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, obs=None, data=None, device: int = 0):
    """The matrix ``l[r, j] = term(x_r, d_j)`` over the selected rows and the observations ``obs = (first, stop)`` (default: all), as
    a dense ``[n, stop - first]`` array (``kmc_chain_pointwise_loglike``): what PSIS-LOO outside the library starts from.  It must
    fit the device's free memory; thin, or ask for a range of observations at a time."""
    return loglike_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, obs, data)
