"""The highest-density interval of include/kissmcmc_hip.h restated in numpy: the one reference of tests/test_hdi_cpu.py and
tests/test_gpu_hdi.py.  Every device comparison against it is an equality of lo, hi and start.

Per column: the N draws sorted ascending after x + 0.0 (so -0.0 is +0.0); k = floor(p N) in double; the widths
w_i = x_(i+k) - x_(i), i = 0 .. N - k - 1; i* = the lexicographic minimum of (w_i is NaN, w_i, i); the interval is
[x_(i*), x_(i*+k)].  A column with a NaN among its draws: NaN, NaN and i* = -1."""
import numpy as np


def span(n, p):
    """k = floor(p n), evaluated in double as written."""
    return int(np.floor(np.float64(p) * np.float64(n)))


def column(x, p):
    """``(lo, hi, start, k)`` of the draws ``x`` (1-D, any float dtype; widened exactly) for the probability ``p``."""
    x = np.asarray(x).astype(np.float64).ravel()
    n = x.size
    k = span(n, p)
    assert 1 <= k <= n - 1, (n, p, k)
    if np.isnan(x).any():
        return np.nan, np.nan, -1, k
    xs = np.sort(x + 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        w = xs[k:] - xs[:n - k]
    isnan = np.isnan(w)
    i = np.arange(n - k)
    best = int(np.lexsort((i, np.where(isnan, 0.0, w), isnan))[0])       # the last key is the primary one
    return xs[best], xs[best + k], best, k


def columns(draws, probs):
    """``draws[N, ncols]``, ``probs[nprob]`` -> ``lo[nprob, ncols], hi[nprob, ncols], start[nprob, ncols] (int64), k[nprob]``."""
    draws = np.asarray(draws)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    P, ncols = probs.size, draws.shape[1]
    lo, hi = np.empty((P, ncols)), np.empty((P, ncols))
    start, k = np.empty((P, ncols), dtype=np.int64), np.empty(P, dtype=np.int64)
    for a, p in enumerate(probs.tolist()):
        for c in range(ncols):
            lo[a, c], hi[a, c], start[a, c], k[a] = column(draws[:, c], p)
    return lo, hi, start, k


def of_chain(thetas, probs, logdensities=None, first_sample=0, walkers=None):
    """The same for ``thetas[walker][sample](dim)`` (and ``logdensities[walker][sample]`` as the last column), over the samples
    ``>= first_sample`` of the walkers ``walkers`` (an index array or None)."""
    th = np.asarray(thetas)
    if th.ndim == 2:
        th = th[:, :, None]
    if logdensities is not None:
        th = np.concatenate([th.astype(np.float64), np.asarray(logdensities, dtype=np.float64)[:, :, None]], axis=2)
    if walkers is not None:
        th = th[np.asarray(walkers)]
    th = th[:, first_sample:]
    return columns(th.reshape(-1, th.shape[2]), probs)


def prob_for(n, k):
    """A probability p with floor(p n) == k exactly: the middle of [k / n, (k + 1) / n)."""
    p = (k + 0.5) / n
    assert 0.0 < p < 1.0 and span(n, p) == k
    return p
