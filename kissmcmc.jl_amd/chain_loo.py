"""PSIS-LOO -- Pareto-smoothed importance-sampling leave-one-out cross-validation (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson,
Gelman, Yao & Gabry 2024) -- of a :class:`DataDensity` over a stored chain, on the device where the chain, the observations and the
compiled term are.  The ``[rows][observations]`` matrix never exists: every pass recomputes the terms.

``include/kissmcmc_hip.h`` has the definition, step by step; in short, per observation ``j`` over the ``n`` selected rows: the shifted log
ratios ``x_r = min_r l - l_r``; the ``M = ceil(min(0.2 n, 3 sqrt(n / r_eff)))`` largest of them strictly above the cut-off are the tail; a
generalised Pareto is fitted to the tail (Zhang & Stephens, as ArviZ's ``_gpdfit``), its shape is ``pareto_k``; the tail's weights are
replaced by the fit's order statistics; ``elpd_loo_j`` is the log of the weighted mean of the likelihood.  ``r_eff`` is one number, or
``"chain"``: then ``r_eff_j = ess_j / (m h)`` of the series ``exp(l - max_r l)`` by the convergence diagnostics' own estimator
(:func:`relative_eff`) and observation ``j`` gets its own tail length; ``r_eff_j=`` supplies one number per observation instead.

The selection (``first_sample``, ``thin``, ``walkers``) and the input layouts are those of :mod:`.chain_predictive`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .chain_convergence import _max_lag_arg
from .chain_predictive import _elpd_difference, _held_out, _host_provider, _nrows
from .densities import DataDensity
from .summary import _SamplerProvider, _p

TOTALS = ("elpd_loo", "se", "p_loo", "looic", "lppd", "n_nan")
INFO = ("n", "tail_len", "blocks", "obs_per_block", "ns_min", "ns_select", "ns_gather", "ns_fit", "terms_per_pass", "log1p_evals", "ns_stats",
        "nruns")
INFO_REFF = INFO + ("ns_weights", "ns_ess", "groups", "n_reff_nan")
REFF_INFO = ("n", "groups", "ns_pass1", "ns_weights", "ns_ess", "h")


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


def _r_eff_mode(r_eff, r_eff_j, count):
    """The relative efficiency as the calls take it: one number (``r_eff``: the scalar calls), ``None`` (``r_eff="chain"``: computed per
    observation from the chain) or an array of one entry per observation asked for (``r_eff_j``)."""
    if r_eff_j is not None:
        a = np.ascontiguousarray(r_eff_j, dtype=np.float64)
        if a.ndim != 1 or a.size != count:
            raise ValueError(f"r_eff_j must have one entry per observation asked for ({count}); its shape is {a.shape}")
        return a
    if isinstance(r_eff, str):
        if r_eff != "chain":
            raise ValueError('r_eff must be a number or "chain"')
        return None
    if np.ndim(r_eff) != 0:
        raise ValueError('r_eff must be one number or "chain": a per-observation r_eff goes in r_eff_j=')
    return float(r_eff)


def _call(p, which, thin, r_eff, first, count, workspace, outs, split=True, max_lag=None):
    if isinstance(r_eff, float):
        sel = [int(thin), r_eff, first, count, int(workspace or 0)]
    else:
        which += "_reff"
        sel = [int(thin), _p(r_eff, C.c_double), int(bool(split)), _max_lag_arg(max_lag), first, count, int(workspace or 0)]
    if isinstance(p, _SamplerProvider):
        _lib.check(getattr(p.s._L, "kmc_sampler_psis_" + which)(p.s._h, p.first, _p(p.mask, C.c_uint8), *sel, *outs))
    else:
        _lib.check(getattr(_lib.lib(), "kmc_chain_psis_" + which)(p.pdf.user_handle, _p(p.params, C.c_double), _p(p.chain, C.c_double), p.nsamples,
                                                                  p.nwalkers, p.ndim, p.first, _p(p.mask, C.c_uint8), *sel, p.device, *outs))


def _reff_outs(count):
    return np.full(max(count, 1), np.nan), np.zeros(max(count, 1), dtype=np.int64), C.c_int64()


def loo_from(p, pdf, thin=1, r_eff=1.0, obs=None, workspace=None, with_info=False, split=True, max_lag=None, r_eff_j=None):
    first, count = _range(pdf, obs)
    r = _r_eff_mode(r_eff, r_eff_j, count)
    stats, lppd = np.full((4, max(count, 1)), np.nan), np.full(max(count, 1), np.nan)
    n, info = C.c_int64(), np.zeros(len(INFO_REFF), dtype=np.int64)
    outs = [_p(stats, C.c_double), _p(lppd, C.c_double)]
    if isinstance(r, float):
        _call(p, "loo", thin, r, first, count, workspace, outs + [C.byref(n), _p(info, C.c_int64)])
        ru, tl, nn = np.full(max(count, 1), r), np.full(max(count, 1), info[1], dtype=np.int64), C.c_int64(0)
    else:
        ru, tl, nn = _reff_outs(count)
        _call(p, "loo", thin, r, first, count, workspace, outs + [_p(ru, C.c_double), _p(tl, C.c_int64), C.byref(nn), C.byref(n), _p(info, C.c_int64)],
              split, max_lag)
    w = loo_stats(stats, lppd, n.value)
    w.update(tail_len=int(info[1]), r_eff_j=ru, tail_len_j=tl, n_reff_nan=nn.value)
    if with_info:
        w["info"] = dict(zip(INFO_REFF if not isinstance(r, float) else INFO, info.tolist()))
    return w


def tail_from(p, pdf, thin=1, r_eff=1.0, obs=None, workspace=None, split=True, max_lag=None, r_eff_j=None):
    first, count = _range(pdf, obs)
    r = _r_eff_mode(r_eff, r_eff_j, count)
    nrows = _nrows(p, thin)
    if isinstance(r, float):
        try:
            M = psis_plan(nrows, max(pdf.data.shape[0], 1) if isinstance(pdf, DataDensity) else 1, r)["tail_len"]
        except _lib.KmcError:
            M = 1                                                                # (the call below refuses with the library's own words)
    else:
        M = max(1, min(4096, -(-nrows // 5)))                                    # (max_j M_j <= min(4096, ceil(0.2 n)) whatever r_eff_j is)
    tail = np.full((max(count, 1), M), np.nan)
    m, xc, nt = np.full(max(count, 1), np.nan), np.full(max(count, 1), np.nan), np.zeros(max(count, 1), dtype=np.int32)
    tl, n = C.c_int64(M), C.c_int64()
    outs = [_p(tail, C.c_double), _p(m, C.c_double), _p(xc, C.c_double), _p(nt, C.c_int32), C.byref(tl)]
    if isinstance(r, float):
        _call(p, "tail", thin, r, first, count, workspace, outs + [C.byref(n)])
        ru, tlj, nn = np.full(max(count, 1), r), np.full(max(count, 1), tl.value, dtype=np.int64), C.c_int64(0)
    else:
        ru, tlj, nn = _reff_outs(count)
        _call(p, "tail", thin, r, first, count, workspace, outs + [_p(ru, C.c_double), _p(tlj, C.c_int64), C.byref(nn), C.byref(n)], split, max_lag)
        tail = tail.reshape(-1)[:max(count, 1) * max(tl.value, 1)].reshape(max(count, 1), max(tl.value, 1)).copy()   # (rows of tail_len on return)
    return {"tail": tail, "m_j": m, "xc_j": xc, "n_tail_j": nt.astype(np.int64), "tail_len": tl.value, "n": n.value, "r_eff_j": ru, "tail_len_j": tlj,
            "n_reff_nan": nn.value}


def relative_eff_from(p, pdf, thin=1, obs=None, split=True, max_lag=None, workspace=None, with_info=False):
    first, count = _range(pdf, obs)
    k = max(count, 1)
    r, ess, T, flags = np.full(k, np.nan), np.full(k, np.nan), np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int32)
    m, h, n, info = C.c_int64(), C.c_int64(), C.c_int64(), np.zeros(len(REFF_INFO), dtype=np.int64)
    sel = [int(thin), first, count, int(bool(split)), _max_lag_arg(max_lag), int(workspace or 0)]
    outs = [_p(r, C.c_double), _p(ess, C.c_double), _p(T, C.c_int64), _p(flags, C.c_int32), C.byref(m), C.byref(h), C.byref(n), _p(info, C.c_int64)]
    if isinstance(p, _SamplerProvider):
        _lib.check(p.s._L.kmc_sampler_relative_eff(p.s._h, p.first, _p(p.mask, C.c_uint8), *sel, *outs))
    else:
        _lib.check(_lib.lib().kmc_chain_relative_eff(p.pdf.user_handle, _p(p.params, C.c_double), _p(p.chain, C.c_double), p.nsamples, p.nwalkers,
                                                     p.ndim, p.first, _p(p.mask, C.c_uint8), *sel, p.device, *outs))
    w = {"r_eff_j": r, "ess_j": ess, "lag": T, "truncated": (flags & _lib.CONV_TRUNCATED) != 0, "m": m.value, "h": h.value, "n": n.value}
    if with_info:
        w["info"] = dict(zip(REFF_INFO, info.tolist()))
    return w


def weights_from(p, pdf, thin=1, obs=None, data=None):
    D, nd2, nc2 = _held_out(data)
    J = nd2 if D is not None else (pdf.data.shape[0] if isinstance(pdf, DataDensity) else 1)
    first, stop = (0, J) if obs is None else (int(obs[0]), int(obs[1]))
    count = stop - first
    v, M = np.empty((max(_nrows(p, thin), 1), max(count, 1))), np.full(max(count, 1), np.nan)
    n = C.c_int64()
    mid = [int(thin), _p(D, C.c_double), nd2, nc2, first, count]
    outs = [_p(v, C.c_double), _p(M, C.c_double), C.byref(n)]
    if isinstance(p, _SamplerProvider):
        _lib.check(p.s._L.kmc_sampler_pointwise_weights(p.s._h, p.first, _p(p.mask, C.c_uint8), *mid, *outs))
    else:
        _lib.check(_lib.lib().kmc_chain_pointwise_weights(p.pdf.user_handle, _p(p.params, C.c_double), _p(p.chain, C.c_double), p.nsamples, p.nwalkers,
                                                          p.ndim, p.first, _p(p.mask, C.c_uint8), *mid, p.device, *outs))
    return v, M


def sampler_loo(s, first_sample=0, thin=1, walkers=None, r_eff=1.0, obs=None, workspace=None, with_info=False, split=True, max_lag=None, r_eff_j=None):
    """:func:`loo` on the chain a :class:`Sampler` holds (``kmc_sampler_psis_loo``, ``kmc_sampler_psis_loo_reff``)."""
    return loo_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, r_eff, obs, workspace, with_info, split, max_lag, r_eff_j)


def sampler_psis_tail(s, first_sample=0, thin=1, walkers=None, r_eff=1.0, obs=None, workspace=None, split=True, max_lag=None, r_eff_j=None):
    """:func:`psis_tail` on the chain a :class:`Sampler` holds (``kmc_sampler_psis_tail``, ``kmc_sampler_psis_tail_reff``)."""
    return tail_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, r_eff, obs, workspace, split, max_lag, r_eff_j)


def sampler_relative_eff(s, first_sample=0, thin=1, walkers=None, obs=None, split=True, max_lag=None, workspace=None, with_info=False):
    """:func:`relative_eff` on the chain a :class:`Sampler` holds (``kmc_sampler_relative_eff``)."""
    return relative_eff_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, obs, split, max_lag, workspace, with_info)


def sampler_pointwise_weights(s, first_sample=0, thin=1, walkers=None, obs=None, data=None):
    """:func:`pointwise_weights` on the chain a :class:`Sampler` holds (``kmc_sampler_pointwise_weights``)."""
    return weights_from(_SamplerProvider(s, first_sample, walkers), s.pdf, thin, obs, data)


def loo(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, r_eff=1.0, obs=None, workspace=None, device: int = 0,
        with_info: bool = False, split: bool = True, max_lag=None, r_eff_j=None):
    """PSIS-LOO of the :class:`DataDensity` ``pdf`` over the posterior sample ``thetas[walker][sample](dim)`` (uploaded first): the rows are
    the samples ``first_sample, first_sample + thin, ...`` of the walkers ``walkers``, at least 5.  ``r_eff`` is the relative efficiency
    (ESS / n) of the importance weights that sets the tail length: one number for all observations (default 1.0), or ``"chain"`` to
    compute it per observation; ``r_eff_j`` gives it as an array with one entry per observation asked for instead (an array in ``r_eff``
    itself stays refused).  ``"chain"`` computes it from the chain (:func:`relative_eff`, with ``split``
    and ``max_lag``; an observation whose ``r_eff_j`` is NaN gets the tail length of 1.0 and counts in ``n_reff_nan``).  For an
    ensemble chain the computed values are usually well below 1, so tails are longer and the limit of 4096 draws is met sooner (``n =
    200 000`` with ``r_eff = 0.1`` asks for 4 243: thin).  ``obs = (first, count)`` restricts the observations, and the totals are
    then over that range; ``workspace`` is the bytes of device work space a block of observations may take (default 1 GiB).

    A dict: the scalars ``elpd_loo, se, p_loo, looic (= -2 elpd_loo), lppd, n, tail_len`` (the largest tail length), ``n_nan``
    (observations whose outputs are NaN: a NaN among their terms, no finite minimum, or a fit without a positive scale), ``n_reff_nan``;
    ``k_counts``, the observations with ``pareto_k <= 0.5``, in ``(0.5, 0.7]``, in ``(0.7, 1]`` and above 1 (``+inf``, a tail of fewer
    than 5, counts there); and the arrays ``elpd_loo_j, p_loo_j, pareto_k, n_tail_j`` (-1 for a NaN observation), ``lppd_j`` (from
    :func:`waic`'s passes over the same rows), ``r_eff_j`` (as computed, NaN kept, or as given) and ``tail_len_j``.  Held-out data has
    no leave-one-out: there is no ``data=``.  Equal calls return equal bits, a selection gives the bits of the call on the rows copied
    out, :meth:`Sampler.loo` equals this on the downloaded chain bit for bit, an observation's outputs depend neither on ``obs`` nor
    on ``workspace``, an ``r_eff_j`` of equal entries returns the bits of that number, and ``"chain"`` the bits of its own ``r_eff_j`` (NaN
    replaced by 1) given back.  Not built: ArviZ's one ``r_eff`` from the parameters' ESS, ``mcse_elpd_loo``, moment matching."""
    return loo_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, r_eff, obs, workspace, with_info, split, max_lag, r_eff_j)


def psis_tail(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, r_eff=1.0, obs=None, workspace=None, device: int = 0,
              split: bool = True, max_lag=None, r_eff_j=None):
    """The exact part of :func:`loo` read out (``kmc_chain_psis_tail``, ``kmc_chain_psis_tail_reff``): dict ``tail[count, tail_len]`` (each
    observation's tail ``x`` ascending, padded with NaN), ``m_j`` (the shift), ``xc_j`` (the cut-off), ``n_tail_j`` (-1, with NaN
    everywhere else, for a NaN observation), ``tail_len`` (the largest), ``n``, and ``r_eff_j, tail_len_j, n_reff_nan`` as :func:`loo`;
    ``r_eff`` and ``r_eff_j`` are :func:`loo`'s."""
    return tail_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, r_eff, obs, workspace, split, max_lag, r_eff_j)


def relative_eff(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, obs=None, split: bool = True, max_lag=None, workspace=None,
                 device: int = 0, with_info: bool = False):
    """The relative efficiency of PSIS-LOO's importance weights, per observation (``kmc_chain_relative_eff``): ``r_eff_j = ess_j / (m h)``
    with ``ess``, ``m``, ``h`` those of :func:`convergence` on the series ``v[k][j] = exp(l[k][j] - max_r l[r][j])`` of the selected
    rows -- ``loo``'s ``relative_eff(exp(log_lik))`` under this library's BDA3 estimator.  A dict ``r_eff_j, ess_j, lag, truncated``
    (arrays over ``obs = (first, count)``, default all) and ``m, h, n``.  ``r_eff_j`` is NaN for a constant column or one with a NaN,
    and may exceed 1.  An observation's bits depend neither on ``obs`` nor on ``workspace``."""
    return relative_eff_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, obs, split, max_lag, workspace, with_info)


def pointwise_weights(pdf, thetas, first_sample: int = 0, thin: int = 1, walkers=None, obs=None, data=None, device: int = 0):
    """The series behind :func:`relative_eff`, read out (``kmc_chain_pointwise_weights``): ``(v, M_j)`` with ``v[n, stop - first] =
    exp(l - M_j)`` dense over the observations ``obs = (first, stop)`` (as :func:`pointwise_loglike`; default all) and ``M_j`` the
    exact column maxima.  A column whose ``M_j`` is NaN or ``-inf`` is all NaN; the arg-max rows are exactly 1.0."""
    return weights_from(_host_provider(pdf, thetas, first_sample, walkers, device), pdf, thin, obs, data)
