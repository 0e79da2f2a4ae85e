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

The rank-normalised form (Vehtari et al. 2021; :func:`rank_convergence`, ``convergence(..., rank=True)``) ranks every pooled draw of a
column on the device (``kmc_sampler_rank_scores`` / ``kmc_chain_rank_scores``: a segmented radix sort and two binary searches a draw),
turns the ranks into normal scores and applies the same statistics to them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .summary import _HostProvider, _SamplerProvider, _p

COLUMNS = ("mean", "std", "rhat", "ess", "mcse", "lag", "truncated", "m", "h")


def _stats_buffers(ncols):
    """The per-column outputs of the statistics, and their pointers in the order of the C calls."""
    out = {k: np.empty(ncols) for k in ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse")}
    out["T"] = np.empty(ncols, dtype=np.int64)
    out["flags"] = np.empty(ncols, dtype=np.int32)
    args = [_p(out[k], C.c_double) for k in ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse")] + [_p(out["T"], C.c_int64), _p(out["flags"], C.c_int32)]
    return out, args


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
    out, args = _stats_buffers(ncols)
    _lib.check(_lib.lib().kmc_convergence_stats(int(m), int(h), ncols, _p(cm, C.c_double), _p(cv, C.c_double), _p(lag, C.c_double), lag.shape[1],
                                                int(max_lag), *args))
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


def _lag_buffers(ncols, nw, nlags, split, moments):
    m = max(1, (2 if split else 1) * nw)
    cm = np.empty((ncols, m)) if moments else None
    cv = np.empty((ncols, m)) if moments else None
    return cm, cv, np.empty((ncols, max(0, int(nlags))))


def lag_sums_from(p, lag0=1, nlags=0, split=True, logp=False, moments=True):
    """:func:`lag_sums` from a provider (``summary._SamplerProvider``, ``summary._HostProvider``): ``kmc_sampler_lag_sums`` /
    ``kmc_chain_lag_sums``."""
    cm, cv, lag = _lag_buffers(p.ndim + (1 if logp else 0), p.nselected, nlags, split, moments)
    m, h = C.c_int64(), C.c_int64()
    p.call("lag_sums", [int(bool(split)), int(lag0), int(nlags)], [_p(cm, C.c_double), _p(cv, C.c_double), _p(lag, C.c_double), C.byref(m), C.byref(h)],
           logp, logp_at=1)
    return {"chain_mean": cm, "chain_var": cv, "lagsum": lag, "lag0": int(lag0), "m": m.value, "h": h.value}


def sampler_lag_sums(s, lag0=1, nlags=0, first_sample=0, walkers=None, split=True, logp=False, moments=True):
    """The device stage on the chain a :class:`Sampler` holds (``kmc_sampler_lag_sums``); see :func:`lag_sums`."""
    return lag_sums_from(_SamplerProvider(s, first_sample, walkers), lag0, nlags, split, logp, moments)


def lag_sums(thetas, logdensities=None, lag0=1, nlags=0, first_sample=0, walkers=None, split=True, moments=True, device=0):
    """The device stage of the diagnostics (``kmc_chain_lag_sums``): a dict ``chain_mean[ncols, m]``, ``chain_var[ncols, m]`` (None
    with ``moments=False``), ``lagsum[ncols, nlags]`` with ``lagsum[c, k] = D_(lag0 + k)``, the sum over chains ``j`` and samples
    ``i >= t`` of ``(x[i, j] - x[i - t, j])**2``, and ``m``, ``h``.  Chain ``j = half * nw + k`` for the k-th selected walker.  Each
    number is the sum of its terms in an order the library chooses: equal bits from equal calls, no float atomics."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return lag_sums_from(p, lag0, nlags, split, p.logp is not None, moments)


def _raw(p, name, out, args, split, logp, max_lag):
    """One of the two whole-diagnostic calls: ``split``, ``with_logp`` / ``device`` by the route, ``max_lag``, the outputs, ``m``, ``h``, ``info``."""
    m, h = C.c_int64(), C.c_int64()
    p.call(name, [int(bool(split)), _max_lag_arg(max_lag)], args + [C.byref(m), C.byref(h), _p(out["info"], C.c_int64)], logp, logp_at=1)
    out["m"], out["h"] = m.value, h.value
    return out


def _full_buffers(ncols):
    out, args = _stats_buffers(ncols)
    out["info"] = np.zeros(4, dtype=np.int64)
    return out, args


def convergence_raw_from(p, split=True, logp=False, max_lag=None):
    """Everything ``kmc_sampler_convergence`` / ``kmc_chain_convergence`` returns: the arrays of :func:`convergence_stats` plus ``m``, ``h``
    and ``info`` (lags computed, blocks of 32 lags run, bytes of the chain loaded by the lag kernel and by the moment kernels)."""
    return _raw(p, "convergence", *_full_buffers(p.ndim + (1 if logp else 0)), split, logp, max_lag)


def sampler_convergence_raw(s, first_sample=0, walkers=None, split=True, logp=False, max_lag=None):
    """:func:`convergence_raw_from` on the chain a :class:`Sampler` holds."""
    return convergence_raw_from(_SamplerProvider(s, first_sample, walkers), split, logp, max_lag)


def chain_convergence_raw(thetas, logdensities=None, first_sample=0, walkers=None, split=True, max_lag=None, device=0):
    """The same for a chain in host memory."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return convergence_raw_from(p, split, p.logp is not None, max_lag)


RANK_COLUMNS = ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "median", "q05", "q95")


def rank_plan():
    """The shape of the sort behind the ranks (``kmc_rank_plan``): dict ``tile_keys, digit_bits, passes, lds_bytes``."""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.lib().kmc_rank_plan(*[C.byref(x) for x in v]))
    return dict(zip(("tile_keys", "digit_bits", "passes", "lds_bytes"), [x.value for x in v]))


def normal_scores(rank2, S: int):
    """The host form of the score (``kmc_rank_normal_scores``; needs no device): ``z = Phi^-1((rank2 / 2 - 0.375) / (S + 0.25))`` for
    ``rank2 = #{y < x} + #{y <= x} + 1`` in ``[2, 2 S]``, by Wichura's AS 241 in the operation order of
    ``statistics.NormalDist().inv_cdf``.  Returns an array shaped like ``rank2``."""
    r = np.ascontiguousarray(rank2, dtype=np.int64)
    z = np.empty(r.shape)
    _lib.check(_lib.lib().kmc_rank_normal_scores(_p(r, C.c_int64), r.size, int(S), _p(z, C.c_double)))
    return z


def _score_buffers(ncols, nw, n, split, folded):
    h = max(0, n // 2 if split else n)
    m = (2 if split else 1) * nw
    return (np.zeros((ncols, m, h), dtype=np.int64), np.full((ncols, m, h), np.nan), np.full(ncols, np.nan) if folded else None,
            np.zeros(ncols, dtype=np.int64))


def rank_scores_from(p, split=True, folded=False, logp=False):
    """:func:`rank_scores` from a provider: ``kmc_sampler_rank_scores`` / ``kmc_chain_rank_scores``."""
    rank2, z, centre, nan_count = _score_buffers(p.ndim + (1 if logp else 0), p.nselected, p.nsamples - p.first, split, folded)
    m, h = C.c_int64(), C.c_int64()
    p.call("rank_scores", [int(bool(split)), int(bool(folded))],
           [_p(rank2, C.c_int64), _p(z, C.c_double), _p(centre, C.c_double), _p(nan_count, C.c_int64), C.byref(m), C.byref(h)], logp, logp_at=1)
    return {"rank2": rank2, "z": z, "centre": centre, "nan_count": nan_count, "S": m.value * h.value, "m": m.value, "h": h.value}


def sampler_rank_scores(s, first_sample=0, walkers=None, split=True, folded=False, logp=False):
    """:func:`rank_scores` on the chain a :class:`Sampler` holds (``kmc_sampler_rank_scores``)."""
    return rank_scores_from(_SamplerProvider(s, first_sample, walkers), split, folded, logp)


def rank_scores(thetas, logdensities=None, first_sample: int = 0, walkers=None, split: bool = True, folded: bool = False, device: int = 0):
    """The exact ranks of the pooled draws and their normal scores, ranked on the device (``kmc_chain_rank_scores``): a dict
    ``rank2[ncols, m, h]`` (int64: ``#{y < x} + #{y <= x} + 1`` among the ``S = m h`` draws of the column that belong to a chain, so
    that ``rank2 / 2`` is the average 1-based rank -- also what a rank plot needs), ``z[ncols, m, h]`` (the normal score of
    :func:`normal_scores`), ``centre`` (with ``folded``: the medians the draws were folded about, ``|x - median|`` being what is ranked;
    else None), ``nan_count[ncols]``, ``S``, ``m``, ``h``.  Order is by value (``-0.0`` ties with ``+0.0``, infinities are ordinary
    values); a column that holds a NaN gets ``rank2 = 0`` and ``z = NaN``.  Chains as in :func:`convergence`."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return rank_scores_from(p, split, folded, p.logp is not None)


def _rank_buffers(ncols):
    out = {k: np.empty(ncols) for k in RANK_COLUMNS}
    out["T"] = np.zeros((4, ncols), dtype=np.int64)
    out["flags"] = np.zeros(ncols, dtype=np.int32)
    out["info"] = np.zeros(4, dtype=np.int64)
    return out, [_p(out[k], C.c_double) for k in RANK_COLUMNS] + [_p(out["T"], C.c_int64), _p(out["flags"], C.c_int32)]


def rank_convergence_raw_from(p, split=True, logp=False, max_lag=None):
    """Everything ``kmc_sampler_rank_convergence`` / ``kmc_chain_rank_convergence`` returns: the columns of :data:`RANK_COLUMNS`,
    ``T[4, ncols]``, ``flags``, ``m``, ``h`` and ``info`` (lags computed, bytes the two sorts moved, bytes the lag kernel and the moment
    kernels loaded)."""
    return _raw(p, "rank_convergence", *_rank_buffers(p.ndim + (1 if logp else 0)), split, logp, max_lag)


def sampler_rank_convergence_raw(s, first_sample=0, walkers=None, split=True, logp=False, max_lag=None):
    """:func:`rank_convergence_raw_from` on the chain a :class:`Sampler` holds."""
    return rank_convergence_raw_from(_SamplerProvider(s, first_sample, walkers), split, logp, max_lag)


def chain_rank_convergence_raw(thetas, logdensities=None, first_sample=0, walkers=None, split=True, max_lag=None, device=0):
    """The same for a chain in host memory."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return rank_convergence_raw_from(p, split, p.logp is not None, max_lag)


def rank_columns(raw):
    """The public dict of the rank-normalised diagnostics from what the library returned: the columns of :data:`RANK_COLUMNS`,
    ``lag[4, ncols]`` (the ``T`` of the truncation rule for the bulk scores, the folded scores, ``I05`` and ``I95``), ``truncated``,
    ``has_nan``, ``m``, ``h``."""
    out = {k: raw[k] for k in RANK_COLUMNS}
    out.update(lag=raw["T"], truncated=(raw["flags"] & _lib.CONV_TRUNCATED) != 0, has_nan=(raw["flags"] & _lib.CONV_HAS_NAN) != 0,
               m=raw["m"], h=raw["h"])
    return out


def rank_convergence(thetas, logdensities=None, first_sample: int = 0, walkers=None, split: bool = True, max_lag=None, device: int = 0):
    """Rank-normalised R-hat with bulk and tail effective sample sizes (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021), the
    ranks taken on the device: a dict of per-column arrays ``rhat = max(rhat_bulk, rhat_folded)``, ``rhat_bulk`` (the R-hat of
    :func:`convergence` on the normal scores ``z`` of the ranks of the draws), ``rhat_folded`` (the same on the scores of
    ``|x - median|``: it sees chains that share a mean but differ in scale), ``ess_bulk`` (the ess of ``z``), ``ess_tail =
    min(ess_q05, ess_q95)`` (the ess of the indicators ``x <= q05`` and ``x <= q95``: what the ends of a 90 % interval are worth),
    ``median, q05, q95`` (exact, by the rule of :func:`quantile_ranks`), ``lag[4, ncols]``, ``truncated``, ``has_nan`` and ``m``,
    ``h``.  A column that holds a NaN gets NaN throughout and ``has_nan``.  The ess is the variogram estimator of
    :func:`convergence` with its truncation rule, not Stan's.  Chains and arguments as in :func:`convergence`."""
    return rank_columns(chain_rank_convergence_raw(thetas, logdensities, first_sample, walkers, split, max_lag, device))


# ---- the ess and the Monte-Carlo standard error of quantiles ------------------------------------------------------------------------

MAX_PROBS = 16          # per call of the library (kmc_sampler_quantile_mcse, kmc_sampler_indicator_lags)
QUANTILE_COLUMNS = ("quantile", "ess", "mcse", "lower", "upper")


def beta_quantile(prob: float, A: float, B: float) -> float:
    """The quantile function of the Beta distribution (``kmc_beta_quantile``; needs no device): the ``x`` with ``I_x(A, B) = prob``, for
    ``0 < prob < 1`` and finite ``A, B >= 1``, by the fixed algorithm written down in ``include/kissmcmc_hip.h``."""
    x = C.c_double()
    _lib.check(_lib.lib().kmc_beta_quantile(float(prob), float(A), float(B), C.byref(x)))
    return x.value


def quantile_mcse_ranks(S: int, p: float, ess: float):
    """The rank interval behind the MCSE of the quantile ``p`` among ``S`` draws of effective size ``ess``
    (``kmc_quantile_mcse_ranks``; needs no device): ``(a, b, i1, i2)`` with ``a, b`` the Beta quantiles at ``Phi(-1)``, ``Phi(1)`` for
    ``A = ess p + 1``, ``B = ess (1 - p) + 1`` and the 0-based ``i1 = max(floor(a S), 1) - 1``, ``i2 = min(ceil(b S), S) - 1``.  An
    ``ess`` that is NaN or ``<= 0`` gives ``(nan, nan, -1, -1)``."""
    a, b, i1, i2 = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().kmc_quantile_mcse_ranks(int(S), float(p), float(ess), C.byref(a), C.byref(b), C.byref(i1), C.byref(i2)))
    return a.value, b.value, i1.value, i2.value


def indicator_moments(h: int, k: int):
    """``(mu, s2)`` of a chain of ``h`` indicator samples with ``k`` ones (``kmc_indicator_moments``; needs no device)."""
    mu, s2 = C.c_double(), C.c_double()
    _lib.check(_lib.lib().kmc_indicator_moments(int(h), int(k), C.byref(mu), C.byref(s2)))
    return mu.value, s2.value


def indicator_plan():
    """The tile shape of the indicator kernels (``kmc_indicator_plan``): dict ``word_bits, threads, chunk_words, lds_bytes``."""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.lib().kmc_indicator_plan(*[C.byref(x) for x in v]))
    return dict(zip(("word_bits", "threads", "chunk_words", "lds_bytes"), [x.value for x in v]))


def indicator_lags_from(p, thresholds, lag0=1, nlags=0, split=True, logp=False):
    """:func:`indicator_lags` from a provider: ``kmc_sampler_indicator_lags`` / ``kmc_chain_indicator_lags``."""
    ncols = p.ndim + (1 if logp else 0)
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    if thr.ndim == 1:
        thr = thr[None, :]
    if thr.ndim != 2 or thr.shape[1] != ncols:
        raise ValueError(f"thresholds must be [nprobs, {ncols}]")
    nprobs, mm = thr.shape[0], max(1, (2 if split else 1) * p.nselected)
    ones = np.zeros((nprobs, ncols, mm), dtype=np.int64)
    counts = np.zeros((nprobs, ncols, max(0, int(nlags))), dtype=np.uint64)
    m, h = C.c_int64(), C.c_int64()
    p.call("indicator_lags", [int(bool(split)), nprobs, _p(thr, C.c_double), int(lag0), int(nlags)],
           [_p(ones, C.c_int64), _p(counts, C.c_uint64), C.byref(m), C.byref(h)], logp, logp_at=1)
    return {"ones": ones, "lagcount": counts, "lag0": int(lag0), "m": m.value, "h": h.value}


def sampler_indicator_lags(s, thresholds, lag0=1, nlags=0, first_sample=0, walkers=None, split=True, logp=False):
    """:func:`indicator_lags` on the chain a :class:`Sampler` holds (``kmc_sampler_indicator_lags``)."""
    return indicator_lags_from(_SamplerProvider(s, first_sample, walkers), thresholds, lag0, nlags, split, logp)


def indicator_lags(thetas, thresholds, logdensities=None, lag0=1, nlags=0, first_sample=0, walkers=None, split=True, device=0):
    """The device stage of :func:`quantile_mcse` alone (``kmc_chain_indicator_lags``): for ``thresholds[nprobs, ncols]`` the indicators
    ``x <= threshold`` of every column, bit-packed on the device, as a dict ``ones[nprobs, ncols, m]`` (int64: the ones of every chain),
    ``lagcount[nprobs, ncols, nlags]`` (uint64: ``lagcount[..., k] = D_(lag0 + k)``, the pairs ``(i, i - t)`` of a chain whose indicators
    differ, counted by XOR and popcount -- exact integers, the same however the lags are cut into calls) and ``m``, ``h``.  Chains as in
    :func:`lag_sums`."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    return indicator_lags_from(p, thresholds, lag0, nlags, split, p.logp is not None)


def quantile_mcse_raw_from(p, probs, split=True, logp=False, max_lag=None):
    """Everything ``kmc_sampler_quantile_mcse`` / ``kmc_chain_quantile_mcse`` returns: ``[nprobs, ncols]`` arrays ``quantile, ess, mcse,
    lower, upper, T`` (int64), ``flags`` (int32), and ``m``, ``h``, ``info`` (lags computed, bytes the sort moved, bytes the pack kernel
    read, words the lag-count kernel read)."""
    probs = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    ncols = p.ndim + (1 if logp else 0)
    out = {k: np.full((probs.size, ncols), np.nan) for k in QUANTILE_COLUMNS}
    out["T"] = np.zeros((probs.size, ncols), dtype=np.int64)
    out["flags"] = np.zeros((probs.size, ncols), dtype=np.int32)
    out["info"] = np.zeros(4, dtype=np.int64)
    m, h = C.c_int64(), C.c_int64()
    p.call("quantile_mcse", [int(bool(split)), _max_lag_arg(max_lag), probs.size, _p(probs, C.c_double)],
           [_p(out[k], C.c_double) for k in QUANTILE_COLUMNS] + [_p(out["T"], C.c_int64), _p(out["flags"], C.c_int32), C.byref(m), C.byref(h),
                                                                  _p(out["info"], C.c_int64)], logp, logp_at=1)
    out["m"], out["h"] = m.value, h.value
    return out


def quantile_mcse_columns(raw):
    """The public dict from what the library returned: ``quantile, ess, mcse, lower, upper, T, flags`` ``[nprobs, ncols]`` and ``m, h``."""
    out = {k: raw[k] for k in QUANTILE_COLUMNS + ("T", "flags")}
    out.update(m=raw["m"], h=raw["h"])
    return out


def sampler_quantile_mcse(s, probs, first_sample=0, walkers=None, split=True, logp=False, max_lag=None, raw=False):
    """:func:`quantile_mcse` on the chain a :class:`Sampler` holds (``kmc_sampler_quantile_mcse``)."""
    r = quantile_mcse_raw_from(_SamplerProvider(s, first_sample, walkers), probs, split, logp, max_lag)
    return r if raw else quantile_mcse_columns(r)


def quantile_mcse(thetas, probs, logdensities=None, first_sample: int = 0, walkers=None, split: bool = True, max_lag=None, device: int = 0,
                  raw: bool = False):
    """Quantiles of the pooled draws with their effective sample sizes and Monte-Carlo standard errors (Vehtari, Gelman, Simpson,
    Carpenter and Buerkner 2021; ``kmc_chain_quantile_mcse``): for up to 16 probabilities ``probs``, each strictly inside (0, 1), a dict of
    ``[nprobs, ncols]`` arrays ``quantile`` (by the rule of :func:`quantile_ranks` over the ``S = m h`` draws that belong to a chain),
    ``ess`` (of the indicator ``x <= quantile``: the variogram estimator of :func:`convergence` on bit-packed indicator chains, whose lag
    sums are popcounts), ``lower``, ``upper`` (the draws at the ends of the rank interval of :func:`quantile_mcse_ranks`; elements of the
    chain), ``mcse = (upper - lower) / 2``, ``T`` and ``flags`` (as :func:`convergence_stats`; bit 2: the column holds a NaN and
    everything of it is NaN), and ``m``, ``h``.  A constant or two-valued column, whose indicator is 1 everywhere, gives ``ess = mcse =
    NaN`` and no error.  Chains and arguments as in :func:`convergence`; ``raw=True`` adds ``info``."""
    p = _HostProvider(thetas, logdensities, first_sample, walkers, device)
    r = quantile_mcse_raw_from(p, probs, split, p.logp is not None, max_lag)
    return r if raw else quantile_mcse_columns(r)


def add_rank_columns(cols, rank):
    """``cols`` of :func:`columns` with ``rhat_rank, ess_bulk, ess_tail`` of :func:`rank_columns` appended."""
    cols = dict(cols)
    cols.update(rhat_rank=rank["rhat"], ess_bulk=rank["ess_bulk"], ess_tail=rank["ess_tail"])
    return cols


def columns(raw):
    """The public dict of columns from what the library returned: ``mean, std = sqrt(var_plus), rhat, ess, mcse, lag`` (the ``T`` of
    the truncation rule), ``truncated`` (the rule had not fired at ``max_lag``), ``m``, ``h``."""
    with np.errstate(invalid="ignore"):
        std = np.sqrt(raw["var_plus"])
    return {"mean": raw["mean"], "std": std, "rhat": raw["rhat"], "ess": raw["ess"], "mcse": raw["mcse"], "lag": raw["T"],
            "truncated": (raw["flags"] & _lib.CONV_TRUNCATED) != 0, "m": raw["m"], "h": raw["h"]}


def convergence(thetas, logdensities=None, first_sample: int = 0, walkers=None, split: bool = True, max_lag=None, device: int = 0,
                rank: bool = False):
    """Split-R-hat, effective sample size and Monte-Carlo standard error per dimension of ``thetas[walker][sample](dim)`` (and, as a
    last column, of ``logdensities`` when given), over the samples ``>= first_sample`` of the walkers ``walkers``: a dict of columns
    ``mean, std, rhat, ess, mcse, lag, truncated`` and the numbers ``m`` (chains) and ``h`` (samples per chain).

    Every selected walker is a chain, cut into halves with ``split``.  ``rhat = sqrt(var_plus / W)`` compares the variance between
    the chains with the variance within them; ``ess = m h / (1 + 2 sum_{t <= T} rho_t)`` with the autocorrelations ``rho_t`` from the
    variogram and ``T`` the first odd lag at which ``rho_(T+1) + rho_(T+2) < 0``, or ``truncated`` at ``max_lag`` (default
    ``min(h - 1, 1024)``); ``mcse = std / sqrt(ess)``.  A constant column gives NaN; NaN in the chain propagates.

    The walkers of ONE emcee ensemble are not independent (https://dfm.io/posts/autocorr/: "you should not compute the G-R statistic
    using multiple chains in the same emcee ensemble"), so R-hat over them is optimistic: for R-hat use separate runs
    (:func:`evaluate_convergence`) or the independent chains of ``metropolis_chains``.

    ``rank=True`` adds the columns ``rhat_rank``, ``ess_bulk`` and ``ess_tail`` of :func:`rank_convergence`."""
    cols = columns(chain_convergence_raw(thetas, logdensities, first_sample, walkers, split, max_lag, device))
    if rank:
        cols = add_rank_columns(cols, rank_convergence(thetas, logdensities, first_sample, walkers, split, max_lag, device))
    return cols


def _as3(thetas):
    th = np.asarray(thetas, dtype=np.float64)
    if th.ndim == 2:
        th = th[:, :, None]
    if th.ndim != 3:
        raise ValueError("thetas must be [walker][sample] or [walker][sample][dim]")
    return th


def evaluate_convergence(*runs, indices=None, walkernr=None, split: bool = True, device: int = 0, rank: bool = False):
    """Reference ``src/analysis.jl:79-95`` (commented out there): ``(Rs, sample_size, nthin)`` -- R-hat (should be < 1.1) and the
    total effective sample size of all chains combined, per dimension of ``indices`` (all by default), and the average thinning
    factor ``round(n * nwalkers / mean(sample_size))`` (-1 when that is NaN).

    ``runs`` are the ``thetas`` of separate runs of one posterior; their walkers are concatenated, and with ``walkernr`` only walker
    ``walkernr`` of each run is used (the reference's choice).  The reference's warning stands: the walkers of one emcee ensemble are
    not independent, so R-hat over the walkers of a single run is optimistic -- "this needs input from two separate emcee runs", or
    Metropolis chains.  See :func:`convergence` for the definition (the reference's MCMCDiagnostics.jl is not followed).  With
    ``rank=True`` ``Rs`` is the rank-normalised R-hat and ``sample_size`` the bulk ess of :func:`rank_convergence`."""
    if not runs:
        raise ValueError("at least one run")
    ths = [_as3(t) for t in runs]
    if walkernr is not None:
        ths = [t[int(walkernr):int(walkernr) + 1] for t in ths]
    if any(t.shape[1:] != ths[0].shape[1:] for t in ths):
        raise ValueError("the runs must have the same number of samples and dimensions")
    th = np.concatenate(ths, axis=0)
    idx = np.arange(th.shape[2]) if indices is None else np.atleast_1d(np.asarray(indices, dtype=np.int64))
    if rank:
        out = rank_convergence(th, split=split, device=device)
        Rs, sample_size = out["rhat"][idx], out["ess_bulk"][idx]
    else:
        out = convergence(th, split=split, device=device)
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
