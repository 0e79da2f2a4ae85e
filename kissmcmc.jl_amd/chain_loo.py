"""PSIS-LOO -- Pareto-smoothed importance-sampling leave-one-out cross-validation (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson,
Gelman, Yao & Gabry 2024) -- of a :class:`DataDensity` over a stored chain, on the device where the chain, the observations and the
compiled term are.  The ``[rows][observations]`` matrix never exists: every pass recomputes the terms.

``include/kissmcmc_hip.h`` has the definition, step by step; in short, per observation ``j`` over the ``n`` selected rows: the shifted log
ratios ``x_r = min_r l - l_r``; the ``M = ceil(min(0.2 n, 3 sqrt(n / r_eff)))`` largest of them strictly above the cut-off are the tail; a
generalised Pareto is fitted to the tail (Zhang & Stephens, as ArviZ's ``_gpdfit``), its shape is ``pareto_k``; the tail's weights are
replaced by the fit's order statistics; ``elpd_loo_j`` is the log of the weighted mean of the likelihood.

The selection (``first_sample``, ``thin``, ``walkers``) and the input layouts are those of :mod:`.chain_predictive`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .chain_predictive import _elpd_difference, _host_provider
from .densities import DataDensity
from .summary import _SamplerProvider, _p

TOTALS = ("elpd_loo", "se", "p_loo", "looic", "lppd", "n_nan")
INFO = ("n", "tail_len", "blocks", "obs_per_block", "ns_min", "ns_select", "ns_gather", "ns_fit", "terms_per_pass", "log1p_evals", "ns_stats",
        "nruns")


def psis_plan(n: int, ndata: int, r_eff: float = 1.0, workspace: int = 0):
    """The cut of a PSIS-LOO call over ``n`` rows of a density with ``ndata`` observations (``kmc_psis_plan``; needs no device): dict
    ``tail_len`` (``M``), ``m_est`` (the grid of the largest fit), ``obs_per_block`` (observations whose tail buffer and counters fit
    ``workspace`` bytes; 0: 1 GiB) and ``passes`` (recompute passes per block)."""
    v = [C.c_int64() for _ in range(4)]
    _lib.check(_lib.lib().kmc_psis_plan(int(n), int(ndata), float(r_eff), int(workspace), *[C.byref(x) for x in v]))
    return dict(zip(("tail_len", "m_est", "obs_per_block", "passes"), [x.value for x in v]))


def loo_stats(stats, lppd_j, n: int):
    """The host stage (``kmc_loo_stats``; needs no device): from ``stats[4, J]`` (``elpd_loo_j, pareto_k, n_tail_j, sigma_j``) and
    ``lppd_j[J]`` of ``n`` rows the dict :func:`loo` returns, without ``tail_len``."""
    st = np.ascontiguousarray(stats, dtype=np.float64)
    lp = np.ascontiguousarray(lppd_j, dtype=np.float64)
    if st.ndim != 2 or st.shape[0] != 4 or st.shape[1] < 1 or lp.shape != (st.shape[1],):
        raise ValueError("stats must be [4, J] and lppd_j [J]")
    J = st.shape[1]
    pl, tot = np.empty(J), np.empty(10)
    _lib.check(_lib.lib().kmc_loo_stats(J, int(n), _p(st, C.c_double), _p(lp, C.c_double), _p(pl, C.c_double), _p(tot, C.c_double)))
    w = dict(zip(TOTALS, tot[:6].tolist()))
    w["n_nan"] = int(w["n_nan"])
    nt = st[2]
    w.update(n=int(n), k_counts=tuple(int(c) for c in tot[6:10]), elpd_loo_j=st[0].copy(), p_loo_j=pl, pareto_k=st[1].copy(),
             n_tail_j=np.where(np.isnan(nt), -1, nt).astype(np.int64), lppd_j=lp.copy())
    return w


def psis_smooth(sorted_tail_x, xc: float):
    """Fit and smoothing of one observation's tail on the host (``kmc_psis_smooth_host``; needs no device), with the arithmetic and the
    summation order of the device's fit kernel: ``sorted_tail_x`` ascending within ``(xc, 0]``.  Dict ``k, sigma, s`` (the smoothed log
    ratios in the tail's order; the tail itself when it has fewer than 5 entries) and ``sums = (sum exp(s_i), sum exp(s_i - x_i))``."""
    x = np.ascontiguousarray(sorted_tail_x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("the tail must be a vector")
    k, sigma, s, sums = C.c_double(), C.c_double(), np.empty(max(x.size, 1)), np.empty(2)
    _lib.check(_lib.lib().kmc_psis_smooth_host(x.size, _p(x, C.c_double), float(xc), C.byref(k), C.byref(sigma), _p(s, C.c_double),
                                               _p(sums, C.c_double)))
    return {"k": k.value, "sigma": sigma.value, "s": s[:x.size], "sums": (float(sums[0]), float(sums[1]))}


def compare_loo(w_a, w_b):
    """The difference of two models' ``elpd_loo`` over the same observations, from the pointwise arrays of two :func:`loo` results
    (needs no device): :func:`compare_waic`'s rule on ``elpd_loo_j`` -- dict ``elpd_diff`` (positive: ``a`` predicts better), ``se``,
    ``J``."""
    return _elpd_difference(w_a["elpd_loo_j"], w_b["elpd_loo_j"])


def _range(pdf, obs):
    J = pdf.data.shape[0] if isinstance(pdf, DataDensity) else 1
    if obs is None:
        return 0, J
    return int(obs[0]), int(obs[1])


def _call(p, which, thin, r_eff, first, count, workspace, outs):
    sel = [int(thin), float(r_eff), first, count, int(workspace or 0)]
    if isinstance(p, _SamplerProvider):
        _lib.check(getattr(p.s._L, "kmc_sampler_psis_" + which)(p.s._h, p.first, _p(p.mask, C.c_uint8), *sel, *outs))
    else:
        _lib.check(getattr(_lib.lib(), "kmc_chain_psis_" + which)(p.pdf.user_handle, _p(p.params, C.c_double), _p(p.chain, C.c_double), p.nsamples,
                                                                  p.nwalkers, p.ndim, p.first, _p(p.mask, C.c_uint8), *sel, p.device, *outs))


def loo_from(p, pdf, thin=1, r_eff=1.0, obs=None, workspace=None, with_info=False):
    first, count = _range(pdf, obs)
    stats, lppd = np.full((4, max(count, 1)), np.nan), np.full(max(count, 1), np.nan)
    n, info = C.c_int64(), np.zeros(len(INFO), dtype=np.int64)
    _call(p, "loo", thin, r_eff, first, count, workspace, [_p(stats, C.c_double), _p(lppd, C.c_double), C.byref(n), _p(info, C.c_int64)])
    w = loo_stats(stats, lppd, n.value)
    w["tail_len"] = int(info[1])
    if with_info:
        w["info"] = dict(zip(INFO, info.tolist()))
    return w


def tail_from(p, pdf, thin=1, r_eff=1.0, obs=None, workspace=None):
    first, count = _range(pdf, obs)
    nrows = -(-max(0, p.nsamples - p.first) // int(thin)) * p.nselected if thin >= 1 else 0
    try:
        M = psis_plan(nrows, max(pdf.data.shape[0], 1) if isinstance(pdf, DataDensity) else 1, r_eff)["tail_len"]
    except _lib.KmcError:
        M = 1                                                                    # (the call below refuses with the library's own words)
    tail = np.full((max(count, 1), M), np.nan)
    m, xc, nt = np.full(max(count, 1), np.nan), np.full(max(count, 1), np.nan), np.zeros(max(count, 1), dtype=np.int32)
    tl, n = C.c_int64(M), C.c_int64()
    _call(p, "tail", thin, r_eff, first, count, workspace,
          [_p(tail, C.c_double), _p(m, C.c_double), _p(xc, C.c_double), _p(nt, C.c_int32), C.byref(tl), C.byref(n)])
    return {"tail": tail, "m_j": m, "xc_j": xc, "n_tail_j": nt.astype(np.int64), "tail_len": tl.value, "n": n.value}


def _scalar_r_eff(r_eff):
    if np.ndim(r_eff) != 0:
        raise ValueError("r_eff must be one number: a per-observation r_eff is not built")
    return float(r_eff)


def sampler_loo(s, first_sample=0, thin=1, walkers=None, r_eff=1.0, obs=None, workspace=None, with_info=False):
    """:func:`loo` on the chain a :class:`Sampler` holds (``kmc_sampler_psis_loo``)."""
    return loo_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, _scalar_r_eff(r_eff), obs, workspace, with_info)


def sampler_psis_tail(s, first_sample=0, thin=1, walkers=None, r_eff=1.0, obs=None, workspace=None):
    """:func:`psis_tail` on the chain a :class:`Sampler` holds (``kmc_sampler_psis_tail``)."""
    return tail_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, _scalar_r_eff(r_eff), obs, workspace)


def loo(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, r_eff: float = 1.0, obs=None, workspace=None, device: int = 0,
        with_info: bool = False):
    """PSIS-LOO of the :class:`DataDensity` ``pdf`` over the posterior sample ``thetas[walker][sample](dim)`` (uploaded first): the rows are
    the samples ``first_sample, first_sample + thin, ...`` of the walkers ``walkers``, at least 5.  ``r_eff`` is one number, the relative
    efficiency of the chain (ESS / n) that sets the tail length; ``obs = (first, count)`` restricts the observations, and the totals are
    then over that range; ``workspace`` is the bytes of device work space a block of observations may take (default 1 GiB).

    A dict: the scalars ``elpd_loo, se, p_loo, looic (= -2 elpd_loo), lppd, n, tail_len, n_nan`` (observations whose outputs are NaN: a
    NaN among their terms, no finite minimum, or a fit without a positive scale); ``k_counts``, the observations with ``pareto_k <= 0.5``,
    in ``(0.5, 0.7]``, in ``(0.7, 1]`` and above 1 (``+inf``, a tail of fewer than 5, counts there); and the arrays ``elpd_loo_j, p_loo_j,
    pareto_k, n_tail_j`` (-1 for a NaN observation) and ``lppd_j`` (from :func:`waic`'s passes over the same rows).  Held-out data has
    no leave-one-out: there is no ``data=``.  Equal calls return equal bits, a selection gives the bits of the call on the rows copied
    out, :meth:`Sampler.loo` equals this on the downloaded chain bit for bit, and an observation's outputs depend neither on ``obs`` nor
    on ``workspace``."""
    return loo_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, _scalar_r_eff(r_eff), obs, workspace, with_info)


def psis_tail(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, r_eff: float = 1.0, obs=None, workspace=None, device: int = 0):
    """The exact part of :func:`loo` read out (``kmc_chain_psis_tail``): dict ``tail[count, tail_len]`` (each observation's tail ``x``
    ascending, padded with NaN), ``m_j`` (the shift), ``xc_j`` (the cut-off), ``n_tail_j`` (-1, with NaN everywhere else, for a NaN
    observation), ``tail_len`` and ``n``."""
    return tail_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, _scalar_r_eff(r_eff), obs, workspace)
