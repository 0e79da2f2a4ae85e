"""numpy restatement of the marginal histograms (kmc_sampler_histograms / kmc_chain_histograms; include/kissmcmc_hip.h): the binning
rule written with searchsorted, the 1-D histograms of the selected columns with their below / above / nan counts, and the 2-D histograms
of all pairs in list order.  tests/test_histograms_cpu.py pins it against np.histogram, np.histogram2d and np.histogramdd; the GPU
tests compare the kernels with it."""
import numpy as np

BELOW, ABOVE, NAN = -1, -2, -3


def bin_index(x, edges):
    """Per element of x: the bin i with e[i] <= x < e[i + 1], the last bin closed (x == e[B] -> B - 1); BELOW for x < e[0], ABOVE for
    x > e[B], NAN for a NaN.  Comparisons against the edges only."""
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    B = e.size - 1
    i = np.searchsorted(e, x, side="right") - 1          # the last edge <= x (a NaN sorts past every edge)
    i = np.where(x == e[B], B - 1, i)                    # the closed last bin
    i = np.where(x < e[0], BELOW, i)
    i = np.where(x > e[B], ABOVE, i)
    return np.where(np.isnan(x), NAN, i)


def hist1d(x, edges):
    """(counts[B] int64, outside[3] int64: below, above, nan) of the 1-D array x."""
    i = bin_index(np.ravel(x), edges)
    B = np.size(edges) - 1
    counts = np.bincount(i[i >= 0], minlength=B).astype(np.int64)
    return counts, np.array([np.sum(i == BELOW), np.sum(i == ABOVE), np.sum(i == NAN)], dtype=np.int64)


def hist2d(x, y, ex, ey):
    """counts[Bx][By] int64 of the rows whose two coordinates both lie inside their ranges."""
    ix, iy = bin_index(np.ravel(x), ex), bin_index(np.ravel(y), ey)
    Bx, By = np.size(ex) - 1, np.size(ey) - 1
    ok = (ix >= 0) & (iy >= 0)
    return np.bincount(ix[ok] * By + iy[ok], minlength=Bx * By).astype(np.int64).reshape(Bx, By)


def pair_list(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def select(chain, logp=None, first_sample=0, walkers=None):
    """chain [sample][walker][dim] -> (rows [N][dim], logp [N] | None) over the samples >= first_sample of the walkers `walkers` (a
    boolean mask, indices, or None)."""
    chain = np.asarray(chain, dtype=np.float64)
    w = np.arange(chain.shape[1]) if walkers is None else (np.flatnonzero(walkers) if np.asarray(walkers).dtype == np.bool_ else np.unique(walkers))
    rows = chain[first_sample:, w].reshape(-1, chain.shape[2])
    return rows, None if logp is None else np.asarray(logp, dtype=np.float64)[first_sample:, w].ravel()


def histograms(chain, dims, edges, logp=None, first_sample=0, walkers=None, pairs=False):
    """What the library returns: (counts1[ncols, B], outside[ncols, 3], counts2[npairs, B, B] | None, N) for the chain columns `dims`,
    in that order, and -- when logp is given -- the log-densities as the last column; edges [ncols][B + 1]."""
    rows, lp = select(chain, logp, first_sample, walkers)
    cols = [rows[:, d] for d in dims] + ([] if lp is None else [lp])
    edges = np.asarray(edges, dtype=np.float64)
    assert edges.shape[0] == len(cols)
    got = [hist1d(c, e) for c, e in zip(cols, edges)]
    counts1, outside = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    counts2 = None
    if pairs:
        counts2 = np.stack([hist2d(rows[:, dims[a]], rows[:, dims[b]], edges[a], edges[b]) for a, b in pair_list(len(dims))])
    return counts1, outside, counts2, rows.shape[0]
