"""The yardstick of the effective sample size and Monte-Carlo standard error of quantiles (kmc_*_quantile_mcse, kmc_*_indicator_lags; the
definitions are in include/kissmcmc_hip.h): numpy, scipy.special.betaincinv and the yardsticks of the convergence and rank statistics,
nothing of the product.

The indicator bits by comparison, D_t by counting the differing pairs, the chain moments by the formula of the counts, the statistics
through convergence_yardstick.stats, the Beta quantile through scipy, the index rule as written.

Chains are [sample][walker][dim], the layout of Sampler.chain()."""
import math

import numpy as np
from scipy.special import betaincinv

import convergence_yardstick as cy
import rank_yardstick as ry

HAS_NAN = 4
PHI_MINUS_1, PHI_PLUS_1 = 0.15865525393145707, 0.8413447460685429


def indicators(x, thresholds):
    """I[nprobs][ncols][m][h] (bool) of x[ncols][m][h] and thresholds[nprobs][ncols]; nothing is <= NaN."""
    thr = np.asarray(thresholds, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return x[None] <= thr[:, :, None, None]


def lag_counts(I, lag0, nlags):
    """D[..., k] = #{(i, j): I[..., j, i] != I[..., j, i - t]}, t = lag0 + k: int64 over the leading axes of I[..., m, h]."""
    h = I.shape[-1]
    out = np.zeros(I.shape[:-2] + (nlags,), dtype=np.int64)
    for k in range(nlags):
        t = lag0 + k
        out[..., k] = np.count_nonzero(I[..., t:] != I[..., :h - t], axis=(-2, -1))
    return out


def moments(h, k):
    """mu = k / h, ss = k ((1 - mu)(1 - mu)) + (h - k)(mu mu), s2 = ss / (h - 1), every operation rounded on its own, in this order."""
    k = np.asarray(k, dtype=np.int64)
    kd, hd = k.astype(np.float64), np.float64(h)
    mu = kd / hd
    om = 1.0 - mu
    ss = kd * (om * om) + (h - k).astype(np.float64) * (mu * mu)
    return mu, ss / np.float64(h - 1)


def beta_ab(p, ess):
    """(A, B, a, b): A = ess p + 1, B = ess (1 - p) + 1 and the Beta quantiles at Phi(-1), Phi(1), by scipy."""
    A, B = float(ess) * float(p) + 1.0, float(ess) * (1.0 - float(p)) + 1.0
    return A, B, float(betaincinv(A, B, PHI_MINUS_1)), float(betaincinv(A, B, PHI_PLUS_1))


def ranks(S, a, b):
    """0-based (i1, i2) = (max(floor(a S), 1) - 1, min(ceil(b S), S) - 1), the products rounded once."""
    return max(math.floor(float(a) * float(S)), 1) - 1, min(math.ceil(float(b) * float(S)), S) - 1


def margin(S, a, b):
    """How far a S and b S are from an integer: the index rule agrees between two evaluations of a and b only where this is well
    above their difference times S."""
    return min(abs(v - round(v)) for v in (float(a) * float(S), float(b) * float(S)))


def quantile_mcse(chain, probs, logp=None, first=0, walkers=None, split=True, max_lag=None):
    """dict of [nprobs][ncols] arrays quantile, ess, mcse, lower, upper, T, flags, margin (of the index rule; inf where there is no
    interval), and m, h, sorted[ncols][S]."""
    x, m, h = ry.pooled(chain, logp, first, walkers, split)
    ncols, S = x.shape[0], m * h
    probs = [float(p) for p in probs]
    max_lag = min(h - 1, 1024) if max_lag is None else max_lag
    has_nan = np.isnan(x).reshape(ncols, -1).any(axis=1)
    srt = np.sort(x.reshape(ncols, S) + 0.0, axis=1)
    out = {k: np.full((len(probs), ncols), np.nan) for k in ("quantile", "ess", "mcse", "lower", "upper")}
    out["margin"] = np.full((len(probs), ncols), np.inf)
    for c in range(ncols):
        if not has_nan[c]:
            for ip, p in enumerate(probs):
                out["quantile"][ip, c] = ry.quantile(srt[c], p)
    I = indicators(x, out["quantile"])
    mu, s2 = moments(h, I.sum(axis=-1))
    D = lag_counts(I, 1, max_lag).astype(np.float64)
    st = cy.stats(m, h, mu.reshape(-1, m), s2.reshape(-1, m), D.reshape(-1, max_lag), max_lag)
    out["ess"] = st["ess"].reshape(len(probs), ncols)
    out["T"] = st["T"].reshape(len(probs), ncols)
    out["flags"] = st["flags"].reshape(len(probs), ncols)
    for c in range(ncols):
        for ip, p in enumerate(probs):
            if has_nan[c]:
                out["ess"][ip, c], out["T"][ip, c], out["flags"][ip, c] = np.nan, 0, HAS_NAN
                continue
            ess = out["ess"][ip, c]
            if not ess > 0.0:
                continue
            _, _, a, b = beta_ab(p, ess)
            i1, i2 = ranks(S, a, b)
            out["margin"][ip, c] = margin(S, a, b)
            out["lower"][ip, c], out["upper"][ip, c] = srt[c, i1], srt[c, i2]
            with np.errstate(invalid="ignore"):
                out["mcse"][ip, c] = (srt[c, i2] - srt[c, i1]) / 2.0
    out.update(m=m, h=h, sorted=srt)
    return out


def asymptotic_mcse(p, S):
    """sqrt(p (1 - p) / S) / phi(z_p): the standard error of the quantile p of S independent standard normal draws."""
    z = float(ry.inv_cdf(np.array([p]))[0])
    return math.sqrt(p * (1.0 - p) / S) / (math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))
