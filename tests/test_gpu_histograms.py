"""GPU: marginal histograms on the device -- the 1-D histogram of every selected column and the 2-D histogram of every pair
(kmc_sampler_histograms, kmc_chain_histograms) against their numpy restatement (tests/histogram_yardstick.py) over the fetched chain.
Counts are integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import histogram_yardstick as hy

pytestmark = pytest.mark.gpu


def run_sampler(kmc, nw, nd, ns, nburn=3, nthin=1, seed=5, **kw):
    """A Gaussian sampler with ns stored samples; returns it after the run (the caller closes it)."""
    G = nburn + ns * nthin
    th = np.random.default_rng(seed).standard_normal((nw, nd))
    s = kmc.Sampler(kmc.GaussianIso(), nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, **kw)
    s.set_positions(th)
    s.run(G)
    s.sync()
    return s


def check_hist(got, chain, dims, logp=None, first=0, walkers=None):
    """(counts, edges, outside) of a 1-D call against the yardstick over the same edges; returns N."""
    counts, edges, outside = got
    want1, wout, _, n = hy.histograms(chain, dims, edges, logp, first, walkers)
    assert counts.dtype == np.int64 and outside.dtype == np.int64
    np.testing.assert_array_equal(counts, want1)
    np.testing.assert_array_equal(outside, wout)
    np.testing.assert_array_equal(counts.sum(1) + outside.sum(1), np.full(counts.shape[0], n))
    return n


def check_corner(out, chain, first=0, walkers=None):
    dims = out["dims"]
    want1, wout, want2, n = hy.histograms(chain, dims, out["edges"], None, first, walkers, pairs=True)
    assert out["n"] == n and out["hist2d"].dtype == np.int64
    assert out["pairs"] == [(dims[a], dims[b]) for a, b in hy.pair_list(len(dims))]
    np.testing.assert_array_equal(out["hist1d"], want1)
    np.testing.assert_array_equal(out["outside"], wout)
    np.testing.assert_array_equal(out["hist2d"], want2)


def pair_plan(ndims, nbins):
    from kissmcmc_jl_amd import _lib
    ppg, ng, lds = C.c_int32(), C.c_int32(), C.c_int32()
    assert _lib.lib().kmc_hist_pair_plan(ndims, nbins, C.byref(ppg), C.byref(ng), C.byref(lds)) == _lib.OK
    return ppg.value, ng.value, lds.value


DIMS7 = [30, 2, 17, 5, 31, 0, 11]                                                  # unordered, not contiguous


@pytest.mark.parametrize("nw,nd,ns,dims,B2,kw", [
    (6, 2, 5, None, 32, {}),                                                       # one pair, fewer rows than a workgroup
    (100, 3, 40, None, 32, {}),                                                    # odd ndim: padded rows
    (64, 32, 33, DIMS7, 64, {}),                                                   # 21 pairs of 16 KiB: several pair groups, the last not full
    (202, 200, 7, [199, 0, 100], 32, {}),                                          # column grouping on the 1-D side over all 200 columns
    (128, 4, 50, None, 32, dict(dtype="f32")),                                     # float chain, widened exactly
], ids=["6x2x5", "100x3x40", "64x32x33-7dims", "202x200x7", "128x4x50-f32"])
def test_sampler_chain_histograms_equal_numpy(kmc, nw, nd, ns, dims, B2, kw):
    with run_sampler(kmc, nw, nd, ns, **kw) as s:
        assert s.samples_done == ns
        chain, logp = s.chain()
        all_dims = list(range(nd))
        # every column and the log-densities, full range: np.histogram(column, bins=40), counts and edges
        got = s.histogram(logp=True)
        assert check_hist(got, chain, all_dims, logp) == ns * nw
        for c, col in enumerate([chain[:, :, d] for d in range(nd)] + [logp]):
            want, we = np.histogram(col, bins=40)
            np.testing.assert_array_equal(got[1][c], we)
            np.testing.assert_array_equal(got[0][c], want)
        # a range narrower than the data: below and above fill
        got = s.histogram(bins=17, range=(-0.7, 0.9), dims=dims, logp=True)
        check_hist(got, chain, all_dims if dims is None else dims, logp)
        if ns * nw >= 1000:
            assert got[2][:-1, :2].all()
        # the full corner, full range and a narrower one
        full = s.corner(bins=B2, dims=dims)
        check_corner(full, chain)
        for k, (a, b) in enumerate(full["pairs"]):
            ea, eb = full["edges"][full["dims"].index(a)], full["edges"][full["dims"].index(b)]
            np.testing.assert_array_equal(full["hist2d"][k], np.histogram2d(chain[:, :, a].ravel(), chain[:, :, b].ravel(), bins=[ea, eb])[0])
        assert full["hist2d"].sum() == len(full["pairs"]) * ns * nw
        check_corner(s.corner(bins=B2, dims=dims, quantile_range=(0.1, 0.8)), chain)
        if dims is DIMS7:
            ppg, ng, lds = pair_plan(len(dims), B2)                                 # the budget really cuts the 21 pairs into groups
            assert ng >= 2 and ng == -(-21 // ppg) and ppg * B2 * B2 * 4 <= lds <= 160 * 1024
            assert 10 % ppg != 0                                                   # five of them: 10 pairs, a last group that is not full
            check_corner(s.corner(bins=B2, dims=dims[:5], range=(-1.0, 1.2)), chain)


@pytest.mark.parametrize("nw,nd,ns,dims", [(8, 200, 7, None), (6, 4100, 3, [0, 4099])], ids=["8x200x7", "6x4100x3"])
def test_long_rows_with_few_walkers(kmc, nw, nd, ns, dims):
    """Rows that need column grouping, and ndim > 4096, at walker counts no sampler accepts: the same kernels over a chain of that
    shape in host memory (kmc_chain_histograms), an odd ndim's neighbour included."""
    rng = np.random.default_rng(nd)
    chain = rng.standard_normal((ns, nw, nd)) * np.exp(rng.uniform(-3, 3, nd))
    logp = rng.standard_normal((ns, nw))
    th, lg = chain.transpose(1, 0, 2), logp.T
    sel = list(range(nd)) if dims is None else dims
    check_hist(kmc.histogram(th, bins=11, dims=dims, logdensities=lg), chain, sel, logp)
    check_hist(kmc.histogram(th, bins=256, range=(-1.0, 1.0)), chain, list(range(nd)))
    got = kmc.histogram(th[:, :, :nd - 1], bins=11)                                # 199 / 4099 columns: a last group that is not full
    check_hist(got, chain[:, :, :nd - 1], list(range(nd - 1)))
    cdims = [0, nd - 1] if dims is None else dims
    check_corner(kmc.corner(th, bins=9, dims=cdims), chain)
    check_corner(kmc.corner(th, bins=64, dims=[nd - 1, 3, 0, nd // 2], range=(-2.0, 1.0)), chain)


@pytest.fixture(scope="module")
def grid_chain():
    """A host chain on a 0.25 grid, [sample][walker][dim] with its log-densities: 3 000 rows, several workgroups."""
    rng = np.random.default_rng(12)
    chain = np.round(rng.standard_normal((50, 60, 5)) * [1.0, 2.0, 0.5, 4.0, 1.0] * 4.0) / 4.0
    return chain, np.round(rng.standard_normal((50, 60)) * 4.0) / 4.0


def test_elements_exactly_on_the_edges(kmc, grid_chain):
    chain, logp = grid_chain
    th, lg = chain.transpose(1, 0, 2), logp.T
    e = np.arange(-1.0, 1.0 + 0.125, 0.25)                                         # 8 bins whose edges are on the grid; narrower than the data
    assert np.sum(np.isin(chain, e)) > 3000 and np.sum(chain == e[-1]) > 100       # many elements on interior edges and on e[B]
    got = kmc.histogram(th, bins=e, logdensities=lg)
    check_hist(got, chain, range(5), logp)
    flat = chain.reshape(-1, 5)
    for d in range(5):
        np.testing.assert_array_equal(got[0][d], np.histogram(flat[:, d], bins=e)[0])
        assert got[2][d].tolist() == [np.sum(flat[:, d] < e[0]), np.sum(flat[:, d] > e[-1]), 0] and got[2][d, :2].all()
    out = kmc.corner(th, bins=e)
    check_corner(out, chain)
    for k, (a, b) in enumerate(out["pairs"]):
        np.testing.assert_array_equal(out["hist2d"][k], np.histogram2d(flat[:, a], flat[:, b], bins=[e, e])[0])


def test_infinities_and_nans_are_counted_apart(kmc, grid_chain):
    chain, logp = (a.copy() for a in grid_chain)
    chain[[0, 3, 49, 7], [0, 59, 30, 7], [0, 1, 4, 2]] = [np.inf, -np.inf, np.nan, np.nan]
    chain[10, 10] = [np.nan, np.inf, 0.0, -np.inf, 0.0]                            # one row, several columns
    logp[[1, 2, 3], [1, 2, 3]] = [np.nan, -np.inf, np.inf]
    th, lg = chain.transpose(1, 0, 2), logp.T
    got = kmc.histogram(th, bins=13, range=(-3.0, 3.5), logdensities=lg)
    check_hist(got, chain, range(5), logp)
    assert got[2][:, 2].tolist() == [1, 0, 1, 0, 1, 1]                             # the NaNs, column by column
    assert got[2][0, 1] >= 1 and got[2][1, 0] >= 1 and got[2][3, 0] >= 1
    check_corner(kmc.corner(th, bins=13, range=(-3.0, 3.5)), chain)


@pytest.mark.parametrize("B", [1, 64, 256])
def test_bin_count_limits_and_log_spaced_edges(kmc, grid_chain, B):
    chain, logp = grid_chain
    rng = np.random.default_rng(B)
    pos = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), chain.shape))              # six decades per column
    th = pos.transpose(1, 0, 2)
    e = np.logspace(-3, 3, B + 1)                                                  # non-uniform edges, narrower than the data
    k = min(4, B + 1)
    pos[:k, :4, 0] = e[:k, None]                                                   # and elements on them
    pos[5, :, 1] = e[-1]
    got = kmc.histogram(th, bins=e)
    check_hist(got, pos, range(5))
    np.testing.assert_array_equal(got[0][1], np.histogram(pos[:, :, 1], bins=e)[0])
    check_hist(kmc.histogram(grid_chain[0].transpose(1, 0, 2), bins=B), chain, range(5))       # uniform, full range
    if B <= 64:
        check_corner(kmc.corner(th, bins=e), pos)
        check_corner(kmc.corner(grid_chain[0].transpose(1, 0, 2), bins=B, dims=[4, 1, 2]), chain)


def test_one_repeated_value_fills_one_bin(kmc):
    """The contention case: every lane adds to the same counter."""
    nw, nd, ns = 64, 4, 20
    chain = np.full((ns, nw, nd), 1.2345678901234567)
    th = chain.transpose(1, 0, 2)
    N = ns * nw
    counts, edges, outside = kmc.histogram(th, bins=40)                            # numpy's widening: [x - 0.5, x + 0.5]
    np.testing.assert_array_equal(edges[0], np.histogram(chain[:, :, 0], bins=40)[1])
    np.testing.assert_array_equal(counts, np.stack([np.histogram(chain[:, :, 0], bins=40)[0]] * nd))
    assert np.sort(counts, axis=1)[:, -1].tolist() == [N] * nd and counts.sum() == N * nd and not outside.any()
    out = kmc.corner(th, bins=32)
    check_corner(out, chain)
    assert np.all(out["hist2d"].reshape(6, -1).max(axis=1) == N) and out["hist2d"].sum() == 6 * N


def test_many_rows_per_workgroup(kmc):
    """150 000 rows of 16 columns: more steps (1-D) and more tiles (2-D) than workgroups, so that every workgroup loops, the last
    round only partly filled."""
    rng = np.random.default_rng(21)
    nw, ns, nd = 300, 500, 16
    chain = rng.standard_normal((ns, nw, nd)) * np.linspace(0.2, 3.0, nd)
    logp = rng.standard_normal((ns, nw))
    th = chain.transpose(1, 0, 2)
    mask = rng.random(nw) < 0.7
    assert check_hist(kmc.histogram(th, bins=24, range=(-2.0, 2.5), logdensities=logp.T), chain, range(nd), logp) == ns * nw
    check_hist(kmc.histogram(th, bins=24, first_sample=3, walkers=mask), chain, range(nd), None, 3, mask)
    check_corner(kmc.corner(th, bins=20, dims=[15, 0, 7, 8], range=(-2.0, 2.5), first_sample=3, walkers=mask), chain, 3, mask)


def test_first_sample_and_walker_selections(kmc):
    nw, nd, ns = 20, 3, 9
    with run_sampler(kmc, nw, nd, ns) as s:
        chain, logp = s.chain()
        mask = np.zeros(nw, dtype=bool)
        mask[[1, 2, 7, 19]] = True
        for first, walkers in [(0, None), (4, None), (0, mask), (3, mask), (3, [19, 7, 2, 1]), (8, [5]), (ns - 1, np.arange(nw) == 0)]:
            got = s.histogram(bins=6, range=(-1.0, 1.5), first_sample=first, walkers=walkers, logp=True)
            n = check_hist(got, chain, range(nd), logp, first, walkers)
            got = s.histogram(bins=6, first_sample=first, walkers=walkers, dims=[2, 0])          # the selection's own minimum and maximum
            assert check_hist(got, chain, [2, 0], None, first, walkers) == n and not got[2].any()
            out = s.corner(bins=5, range=(-1.0, 1.5), first_sample=first, walkers=walkers)
            assert out["n"] == n
            check_corner(out, chain, first, walkers)
            np.testing.assert_array_equal(kmc.corner(chain.transpose(1, 0, 2), bins=5, range=(-1.0, 1.5), first_sample=first, walkers=walkers)["hist2d"],
                                          out["hist2d"])                           # the host-chain route, same kernels
        assert n == 1


def test_thinning_and_burn_in_count_the_stored_samples(kmc):
    nw, nd = 32, 3
    s = kmc.Sampler(kmc.GaussianIso(), nw, nd, 40, 7, 3, 2.0, 11, store_chain=True, store_logp=True)
    with s:
        s.set_positions(np.random.default_rng(1).standard_normal((nw, nd)))
        s.run(25)                                                                  # part of the run: (25 - 7) // 3 = 6 samples so far
        s.sync()
        assert s.samples_done == 6 and s.nsamples == 11
        chain, logp = s.chain()
        assert check_hist(s.histogram(bins=10, logp=True), chain, range(nd), logp) == 6 * nw
        check_corner(s.corner(bins=10), chain)
        s.run(15)
        s.sync()
        chain, logp = s.chain()
        assert check_hist(s.histogram(bins=10, logp=True), chain, range(nd), logp) == 11 * nw
        check_corner(s.corner(bins=10), chain)


def test_tempered_sampler_histograms_rung_zero(kmc):
    with run_sampler(kmc, 64, 4, 12, betas=[1.0, 0.5]) as s:
        assert s.ntemps == 2
        chain, logp = s.chain()
        assert check_hist(s.histogram(bins=20, logp=True), chain, range(4), logp) == 12 * 64
        check_corner(s.corner(bins=16), chain)


def test_defaults_equal_numpy(kmc):
    with run_sampler(kmc, 100, 3, 41) as s:
        chain, _ = s.chain()
        flat = chain.reshape(-1, 3)
        counts, edges, outside = s.histogram(bins=25)
        out = s.corner(bins=25)
        for d in range(3):
            want, we = np.histogram(flat[:, d], bins=25)
            np.testing.assert_array_equal(edges[d], we)                            # bit for bit
            np.testing.assert_array_equal(out["edges"][d], we)
            np.testing.assert_array_equal(counts[d], want)
            np.testing.assert_array_equal(out["hist1d"][d], want)
        for k, (a, b) in enumerate([(0, 1), (0, 2), (1, 2)]):
            want, wx, wy = np.histogram2d(flat[:, a], flat[:, b], bins=25)
            np.testing.assert_array_equal(out["edges"][a], wx)
            np.testing.assert_array_equal(out["edges"][b], wy)
            np.testing.assert_array_equal(out["hist2d"][k], want)
        assert not outside.any() and out["n"] == flat.shape[0]
        assert kmc.hist_mode(counts, edges).shape == (3,) and kmc.credible_levels(out["hist2d"][0]).shape == (2,)


def test_refusals(kmc):
    from kissmcmc_jl_amd import _lib

    def status(fn):
        with pytest.raises(kmc.KmcError) as e:
            fn()
        return e.value.status

    G = kmc.GaussianIso()
    e = np.linspace(-1.0, 1.0, 5)
    with kmc.Sampler(G, 8, 2, 10, store_logp=True) as s:                            # no KMC_STORE_CHAIN
        assert status(lambda: s.histogram(bins=e)) == _lib.ERR_BAD_ARG
        assert status(lambda: s.corner(bins=e)) == _lib.ERR_BAD_ARG
    with run_sampler(kmc, 8, 2, 5) as s0, kmc.Sampler(G, 8, 2, 10, store_chain=True) as s:    # no KMC_STORE_LOGP
        assert status(lambda: s.histogram(bins=e, logp=True)) == _lib.ERR_BAD_ARG
        assert status(lambda: s.histogram(bins=e)) == _lib.ERR_BAD_ARG             # nothing stored yet: N = 0
        assert status(lambda: s0.histogram(bins=e, first_sample=5)) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.histogram(bins=e, walkers=np.zeros(8, dtype=bool))) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.histogram(bins=np.linspace(0, 1, 258))) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.corner(bins=np.linspace(0, 1, 66))) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.corner(bins=e, dims=[1])) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.histogram(bins=e, dims=[1, 1])) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.histogram(bins=e[::-1])) == _lib.ERR_BAD_ARG
        assert s0.histogram(bins=e)[0].shape == (2, 4)
    with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, stream_chain=True) as s:
        with pytest.raises(kmc.KmcError, match="kmc_chain_histograms") as err:
            s.histogram(bins=e)
        assert err.value.status == _lib.ERR_UNSUPPORTED
        assert status(lambda: s.corner(bins=e)) == _lib.ERR_UNSUPPORTED
    for kw in (dict(shard_rank=0, shard_count=2), dict(p2p=True)):
        with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, **kw) as s:
            assert status(lambda: s.histogram(bins=e)) == _lib.ERR_UNSUPPORTED
