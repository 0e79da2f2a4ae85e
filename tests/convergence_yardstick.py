"""The yardstick of the convergence diagnostics (kmc_*_lag_sums, kmc_convergence_stats; the definitions are in
include/kissmcmc_hip.h): numpy and math.fsum only, nothing of the product.

`raw` gives the three arrays of the device stage with EXACT sums: every term is formed in float64 exactly as the definition writes it
(one subtraction and one multiplication, both rounded) and the terms are added with math.fsum, which returns the correctly rounded sum.
`stats` restates the host stage operation for operation, in Python floats (IEEE doubles): it must agree with the library bit for bit.

Chains are [sample][walker][dim], the layout of Sampler.chain()."""
import math

import numpy as np

NEED_LAGS, TRUNCATED = 1, 2


def ar1(rng, phi, nsamples, nwalkers, ndim):
    """Independent AR(1) series of unit stationary variance: chain[sample][walker][dim]."""
    x = np.empty((nsamples, nwalkers, ndim))
    x[0] = rng.standard_normal((nwalkers, ndim))
    s = math.sqrt(1.0 - phi * phi)
    for i in range(1, nsamples):
        x[i] = phi * x[i - 1] + s * rng.standard_normal((nwalkers, ndim))
    return x


def selection(nsamples, nwalkers, first=0, walkers=None, split=True):
    """(walker indices ascending, n, h, m, the first sample of every half)."""
    if walkers is None:
        w = np.arange(nwalkers)
    else:
        w = np.asarray(walkers)
        w = np.flatnonzero(w) if w.dtype == np.bool_ else np.unique(w.astype(np.int64))
    n = nsamples - first
    h = n // 2 if split else n
    starts = [first, first + n - h] if split else [first]
    return w, n, h, len(starts) * len(w), starts


def chains_of(chain, logp=None, first=0, walkers=None, split=True):
    """x[h][m][ncols] in float64: chain j = half * nw + k; the log-densities, when given, are the last column."""
    chain = np.asarray(chain)
    cols = chain.astype(np.float64)                                                # (a float32 chain widens exactly)
    if logp is not None:
        cols = np.concatenate([cols, np.asarray(logp, dtype=np.float64)[:, :, None]], axis=2)
    w, n, h, m, starts = selection(chain.shape[0], chain.shape[1], first, walkers, split)
    return np.concatenate([cols[s:s + h][:, w] for s in starts], axis=1), h, m


def fsum_rows_plain(a):
    """math.fsum along the rows of a 2-D array [K][N], element by element; a row with inf or NaN in it gets numpy's sum (IEEE: inf,
    or NaN), where math.fsum would raise."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([math.fsum(row) if np.isfinite(row).all() else float(np.sum(row)) for row in a.tolist()])


def fsum_rows(a, overwrite=False):
    """math.fsum along the rows of a 2-D array [K][N] -- the correctly rounded exact sum of every row -- without handing K * N
    Python floats to math.fsum (60 ns each: ten seconds for the largest case of the tests).

    The terms are cut into slices that numpy adds without any rounding error, and math.fsum adds the few slice sums.  One round
    (the ExtractVector step of Rump, Ogita and Oishi's AccSum, 2008): with |a| < 2^e, N <= 2^(b - 1) and sigma = 1.5 * 2^(e + b),
    q = (sigma + a) - sigma is a rounded to a multiple of u = 2^(e + b - 52), and both q and the remainder a - q -- the rounding
    error of the addition sigma + a -- are exact.  Every partial sum of the q of a row is a multiple of u below 2^(e + b) = 2^52 u,
    hence a double: np.sum(q) is exact in any order.  The remainders are at most u / 2 and go into the next round; each round takes
    52 - b bits off, until nothing is left.  A row's total is the exact sum of its slice sums, which math.fsum rounds once."""
    a = np.array(a, dtype=np.float64, order="C", copy=not overwrite)
    n = a.shape[1]
    if n < 64:
        return fsum_rows_plain(a)
    b = max(1, (n - 1).bit_length()) + 1
    parts = []
    q = np.empty_like(a)
    while True:
        amax = max(float(a.max()), -float(a.min()))
        if not amax > 0.0:
            if amax != amax:                                                       # a NaN
                return fsum_rows_plain(a if not parts else np.concatenate([np.array(parts).T, a], axis=1))
            break
        e = math.frexp(amax)[1] if amax != math.inf else 2000                      # amax < 2^e
        if e + b - 52 < -1000 or e + b > 1000:                                     # (near the ends of the range, inf: the rest to math.fsum)
            return fsum_rows_plain(a if not parts else np.concatenate([np.array(parts).T, a], axis=1))
        sigma = 1.5 * math.ldexp(1.0, e + b)
        np.add(a, sigma, out=q)
        q -= sigma
        a -= q
        parts.append(q.sum(axis=1))
    if not parts:
        return np.zeros(a.shape[0])
    return np.array([math.fsum(row) for row in np.array(parts).T.tolist()])


def raw(chain, logp=None, first=0, walkers=None, split=True, lag0=1, nlags=0, means=None):
    """dict: chain_mean[ncols, m], chain_var[ncols, m], lagsum[ncols, nlags] (D_lag0 ...), m, h -- and what the error bounds of a
    sum in free order need: abs_sum[ncols, m] = sum |x|, sq_sum[ncols, m] = sum (x - mean)^2 (the variance's numerator).
    `means[ncols, m]` replaces the chain means the squares are centred on (the second pass of an implementation under test centres
    on ITS means, which are not these to the last bit)."""
    with np.errstate(invalid="ignore", over="ignore"):                             # (inf and NaN in the chain propagate, silently)
        return _raw(chain, logp, first, walkers, split, lag0, nlags, means)


def _raw(chain, logp, first, walkers, split, lag0, nlags, means):
    x, h, m = chains_of(chain, logp, first, walkers, split)
    ncols = x.shape[2]
    xs = np.ascontiguousarray(x.transpose(2, 1, 0))                                # [ncols][m][h]
    flat = xs.reshape(ncols * m, h)
    mean = fsum_rows(flat) / h
    d = flat - (mean if means is None else np.asarray(means, dtype=np.float64).reshape(-1))[:, None]
    sq = fsum_rows(d * d, overwrite=True)
    out = {"m": m, "h": h, "chain_mean": mean.reshape(ncols, m), "chain_var": (sq / (h - 1)).reshape(ncols, m),
           "abs_sum": fsum_rows(np.abs(flat), overwrite=True).reshape(ncols, m), "sq_sum": sq.reshape(ncols, m)}
    lag = np.zeros((ncols, nlags))
    for k in range(nlags):
        t = lag0 + k
        dd = xs[:, :, t:] - xs[:, :, :h - t]                                       # [ncols][m][h - t]
        dd *= dd
        lag[:, k] = fsum_rows(dd.reshape(ncols, -1), overwrite=True)
    out["lagsum"] = lag
    return out


def stats(m, h, chain_mean, chain_var, lagsum, max_lag):
    """The host stage: dict of per-column lists mean, W, B, var_plus, rhat, ess, mcse, T, flags.  lagsum[c][t - 1] = D_t."""
    chain_mean, chain_var, lagsum = np.asarray(chain_mean), np.asarray(chain_var), np.asarray(lagsum)
    nlags = lagsum.shape[1]
    keys = ("mean", "W", "B", "var_plus", "rhat", "ess", "mcse", "T", "flags")
    out = {k: [] for k in keys}
    nan = float("nan")
    for c in range(chain_mean.shape[0]):
        mu, s2, D = chain_mean[c].tolist(), chain_var[c].tolist(), lagsum[c].tolist()
        sm = 0.0
        for j in range(m):
            sm += mu[j]
        mean = sm / float(m)
        sw = 0.0
        for j in range(m):
            sw += s2[j]
        W = sw / float(m)
        sb = 0.0
        for j in range(m):
            d = mu[j] - mean
            sb += d * d
        B_over_h = sb / float(m - 1)
        frac = float(h - 1) / float(h)
        vp = frac * W + B_over_h
        if W == 0.0:
            row = (mean, W, float(h) * B_over_h, vp, nan, nan, nan, 0, 0)
        else:
            rhat = math.sqrt(vp / W) if vp / W >= 0.0 else nan                     # (math.sqrt raises where C returns NaN)

            def rho(t):
                return 1.0 - (D[t - 1] / (float(m) * float(h - t))) / (2.0 * vp)
            T, flags = 1, 0
            while True:
                if T + 2 > max_lag:
                    flags |= TRUNCATED
                    break
                if T + 2 > nlags:
                    flags |= NEED_LAGS
                    break
                if rho(T + 1) + rho(T + 2) < 0.0:
                    break
                T += 2
            S = 0.0
            for t in range(1, min(T, nlags) + 1):
                S += rho(t)
            den = 1.0 + 2.0 * S
            ess = (float(m) * float(h)) / den if den > 0.0 else nan
            q = vp / ess
            mcse = math.sqrt(q) if q >= 0.0 else nan
            row = (mean, W, float(h) * B_over_h, vp, rhat, ess, mcse, T, flags)
        for k, v in zip(keys, row):
            out[k].append(v)
    return {k: np.array(v, dtype=np.int64 if k == "T" else np.int32 if k == "flags" else np.float64) for k, v in out.items()}


def convergence(chain, logp=None, first=0, walkers=None, split=True, max_lag=None):
    """raw + stats with every lag up to max_lag: what kmc_*_convergence returns (the lags beyond the rule's stop do not matter)."""
    x, h, m = chains_of(chain, logp, first, walkers, split)
    max_lag = min(h - 1, 1024) if max_lag is None else max_lag
    r = raw(chain, logp, first, walkers, split, 1, max_lag)
    return stats(m, h, r["chain_mean"], r["chain_var"], r["lagsum"], max_lag), r


def pair_margins(m, h, var_plus, lagsum, upto):
    """|rho_(k+1) + rho_(k+2)| for odd k = 1, 3, ... while k + 2 <= upto, per column: how far the truncation rule's tests are from
    zero.  A comparison of T, ess or mcse between two evaluations is meaningful only where these are well above the rounding noise."""
    lagsum = np.asarray(lagsum)
    t = np.arange(1, lagsum.shape[1] + 1)
    rho = 1.0 - (lagsum / (m * (h - t))) / (2.0 * np.asarray(var_plus)[:, None])
    k = np.arange(1, upto - 1, 2)
    return np.abs(rho[:, k] + rho[:, k + 1])                                       # rho[:, k] is rho_(k+1)
