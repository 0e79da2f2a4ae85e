"""The eleven read-outs of a stored chain -- order statistics, arg-max, histograms, lag sums, convergence, rank scores, rank-normalised
convergence, highest-density intervals, indicator lag counts, the ESS and MCSE of quantiles, the covariance -- by their two routes: on
the chain a sampler holds (kmc_sampler_*) and on the same chain copied out and uploaded again (kmc_chain_*).  Both routes run one body
per read-out on one view of the chain, so every output agrees bit for bit.
A new read-out joins here."""
import numpy as np
import pytest


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(name, got, want):
    """Dicts and tuples of arrays and numbers, None included, compared by their bits."""
    if isinstance(want, dict):
        assert list(got) == list(want), name
        for k in want:
            assert_same(f"{name}[{k}]", got[k], want[k])
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), name
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(f"{name}[{i}]", g, w)
    elif want is None:
        assert got is None, name
    else:
        assert same_bits(got, want), name


@pytest.mark.gpu
def test_the_two_routes_agree_bit_for_bit_in_all_eleven_readouts(kmc):
    """8 walkers x 3 dimensions in doubles (the stored row is padded: ld = 4 > ndim), 40 stored samples, first_sample = 3, two walkers
    masked out, split, the log-densities included: n = 37 samples give h = 18 per half, below one 32-sample tile of the lag kernel and
    below one sort tile of 4096 keys -- the smallest shape at which the edge paths of both are the only paths."""
    from kissmcmc_jl_amd import chain_convergence as cc
    from kissmcmc_jl_amd import chain_covariance as cv
    from kissmcmc_jl_amd.summary import _HostProvider, _SamplerProvider
    nw, nd, ns, first = 8, 3, 40, 3
    walkers = np.array([1, 1, 0, 1, 1, 1, 0, 1], dtype=bool)
    ranks = np.array([0, 7, 110, 221], dtype=np.int64)                          # N = 37 * 6 = 222
    dims = np.arange(nd)
    edges = np.stack([np.linspace(-2.5, 2.5, 9)] * nd + [np.linspace(-12.0, 0.0, 9)])
    thresholds = np.array([[-0.5, 0.0, 0.5, -3.0], [1.0, 0.25, -1.0, -1.5]])      # [nprobs][ncols]

    def hdi(p):
        lo, hi, start, nan_count, info = p.hdi([0.5, 0.9], logp=True)
        return {"lo": lo, "hi": hi, "start": start, "nan_count": nan_count, "info": info[:3], "n": p.n}    # (info[3..5] are timings)

    def readouts(p):
        out = {"order_stats": p.order_stats(ranks, logp=True), "n": p.n, "argmax": p.argmax(),
               "histograms": p.histograms(dims, edges, logp=True, pairs=True), "n_hist": p.n,
               "lag_sums": cc.lag_sums_from(p, lag0=1, nlags=5, split=True, logp=True),
               "convergence": cc.convergence_raw_from(p, split=True, logp=True),
               "rank_scores": cc.rank_scores_from(p, split=True, folded=True, logp=True),
               "rank_convergence": cc.rank_convergence_raw_from(p, split=True, logp=True),
               "hdi": hdi(p),
               "indicator_lags": cc.indicator_lags_from(p, thresholds, lag0=1, nlags=5, split=True, logp=True),
               "quantile_mcse": cc.quantile_mcse_raw_from(p, [0.1, 0.5], split=True, logp=True),
               "covariance": cv.covariance_raw_from(p, logp=True)}
        return out

    G = 3 + ns
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, 3, 1, 2.0, 5, store_chain=True, store_logp=True) as s:
        s.set_positions(np.random.default_rng(5).standard_normal((nw, nd)))
        s.run(G)
        s.sync()
        chain, logp = s.chain()                                                  # [sample][walker][dim], [sample][walker]
        assert chain.shape == (ns, nw, nd) and chain.dtype == np.float64
        by_sampler = readouts(_SamplerProvider(s, first, walkers))
    by_host = readouts(_HostProvider(chain.transpose(1, 0, 2), logp.T, first, walkers))
    assert by_sampler["n"] == by_sampler["n_hist"] == 37 * 6
    assert by_sampler["hdi"]["n"] == by_sampler["covariance"]["n"] == 37 * 6 and by_sampler["hdi"]["lo"].shape == (2, 4)
    for k in ("lag_sums", "convergence", "rank_scores", "rank_convergence", "indicator_lags", "quantile_mcse"):
        assert (by_sampler[k]["m"], by_sampler[k]["h"]) == (12, 18), k
    assert by_sampler["histograms"][2].shape == (3, 8, 8) and by_sampler["rank_scores"]["rank2"].shape == (4, 12, 18)
    assert_same("readouts", by_host, by_sampler)
