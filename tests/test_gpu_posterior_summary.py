"""GPU: posterior summaries on the device -- exact order statistics by radix select (kmc_sampler_order_stats, kmc_chain_order_stats) and
the MAP sample (kmc_sampler_chain_argmax, kmc_chain_argmax) against their numpy restatement (tests/summary_yardstick.py).  The results
are elements of the chain and integers, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import summary_yardstick as sy

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_sampler(kmc, nw, nd, ns, nburn=3, nthin=1, seed=5, **kw):
    """A Gaussian sampler with ns stored samples; returns it after the run (the caller closes it)."""
    G = nburn + ns * nthin
    th = np.random.default_rng(seed).standard_normal((nw, nd))
    s = kmc.Sampler(kmc.GaussianIso(), nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, **kw)
    s.set_positions(th)
    s.run(G)
    s.sync()
    return s


def check_against_sort(s, ranks):
    chain, logp = s.chain()
    n = chain.shape[0] * chain.shape[1]
    ranks = np.asarray(ranks(n) if callable(ranks) else ranks, dtype=np.int64)
    want_th = np.sort(chain.reshape(n, -1), axis=0)
    want_lp = np.sort(logp.ravel())
    for i in range(0, ranks.size, 16):
        r = ranks[i:i + 16]
        th, lp, N = s.order_stats(r, logp=True)
        assert N == n
        np.testing.assert_array_equal(th, want_th[r])
        np.testing.assert_array_equal(lp, want_lp[r])
        th2, lp2, _ = s.order_stats(r)                                             # without the log-densities' column
        assert lp2 is None
        np.testing.assert_array_equal(th2, th)
    return chain, logp


EDGE = lambda n: [0, n // 2, n - 1, n // 2]                                        # {0, N/2, N-1} and one repeated rank


@pytest.mark.parametrize("nw,nd,ns,ranks,kw", [
    (6, 2, 5, lambda n: np.arange(n), {}),                                         # every rank: the full sort
    (100, 3, 40, EDGE, {}),                                                        # odd ndim: padded rows
    (64, 32, 33, EDGE, {}),
    (202, 200, 7, EDGE, {}),                                                       # rows that need dimension grouping (a sampler wants ndim + 2 walkers)
    (128, 4, 50, EDGE, dict(dtype="f32")),                                         # float chain, widened exactly
    (64, 5, 20, lambda n: [0, 1, n // 3, n // 2, n - 2, n - 1, 7, 7, 8, 9, 10, 11, 12, 13, 14, 15], {}),    # 16 ranks: the smallest column group
], ids=["6x2x5-all", "100x3x40", "64x32x33", "202x200x7", "128x4x50-f32", "64x5x20-16ranks"])
def test_sampler_chain_order_statistics_equal_sort(kmc, nw, nd, ns, ranks, kw):
    with run_sampler(kmc, nw, nd, ns, **kw) as s:
        assert s.samples_done == ns
        chain, logp = check_against_sort(s, ranks)
        th, lp, k, w = s.map_sample()
        kk, ww = np.unravel_index(np.argmax(logp), logp.shape)                     # (np.argmax: the first of equal maxima, row-major)
        assert (k, w) == (kk, ww) and lp == logp[kk, ww]
        np.testing.assert_array_equal(th, chain[kk, ww])


@pytest.mark.parametrize("nw,nd,ns", [(8, 200, 7), (6, 4100, 3)], ids=["8x200x7", "6x4100x3"])
def test_long_rows_with_few_walkers(kmc, nw, nd, ns):
    """Rows that need dimension grouping, and ndim > 4096, at walker counts no sampler accepts (it wants at least ndim + 2): the same
    kernels over a chain of that shape in host memory (kmc_chain_order_stats / kmc_chain_argmax), an odd ndim's neighbour included."""
    from kissmcmc_jl_amd.summary import _HostProvider
    rng = np.random.default_rng(nd)
    chain = rng.standard_normal((ns, nw, nd)) * np.exp(rng.uniform(-20, 20, nd))
    logp = rng.standard_normal((ns, nw))
    n = ns * nw
    ranks = EDGE(n)
    p = _HostProvider(chain.transpose(1, 0, 2), logp.T)
    th, lp = p.order_stats(ranks, logp=True)
    assert p.n == n
    np.testing.assert_array_equal(th, np.sort(chain.reshape(n, nd), axis=0)[ranks])
    np.testing.assert_array_equal(lp, np.sort(logp.ravel())[ranks])
    th1, _ = _HostProvider(chain[:, :, :nd - 1].transpose(1, 0, 2)).order_stats(ranks[:3])     # 199 / 4099 columns: a last group that is not full
    np.testing.assert_array_equal(th1, th[:3, :nd - 1])
    t, l, k, w = p.argmax()
    assert (k, w) == np.unravel_index(np.argmax(logp), logp.shape) and l == logp[k, w]
    np.testing.assert_array_equal(t, chain[k, w])


def test_tempered_sampler_summarises_rung_zero(kmc):
    with run_sampler(kmc, 64, 4, 12, betas=[1.0, 0.5]) as s:
        assert s.ntemps == 2
        check_against_sort(s, EDGE)


def test_thinning_and_burn_in_count_the_stored_samples(kmc):
    nw, nd = 32, 3
    s = kmc.Sampler(kmc.GaussianIso(), nw, nd, 40, 7, 3, 2.0, 11, store_chain=True, store_logp=True)
    with s:
        s.set_positions(np.random.default_rng(1).standard_normal((nw, nd)))
        s.run(25)                                                                  # part of the run: (25 - 7) // 3 = 6 samples so far
        s.sync()
        assert s.samples_done == 6 and s.nsamples == 11
        check_against_sort(s, EDGE)
        s.run(15)
        s.sync()
        assert s.samples_done == 11
        check_against_sort(s, EDGE)


def test_first_sample_and_walker_selections(kmc):
    nw, nd, ns = 20, 3, 9
    with run_sampler(kmc, nw, nd, ns) as s:
        chain, logp = s.chain()
        mask = np.zeros(nw, dtype=bool)
        mask[[1, 2, 7, 19]] = True
        for first, walkers in [(0, None), (4, None), (0, mask), (3, mask), (3, [19, 7, 2, 1]), (8, [5]), (ns - 1, np.arange(nw) == 0)]:
            _, _, n = sy.order_stats(chain, [0], logp, first, walkers)
            ranks = sorted({0, n // 2, n - 1})
            want_th, want_lp, _ = sy.order_stats(chain, ranks, logp, first, walkers)
            th, lp, N = s.order_stats(ranks, first_sample=first, walkers=walkers, logp=True)
            assert N == n
            np.testing.assert_array_equal(th, want_th)
            np.testing.assert_array_equal(lp, want_lp)
            wth, wlp, wk, ww = sy.argmax(chain, logp, first, walkers)
            gth, glp, gk, gw = s.map_sample(first_sample=first, walkers=walkers)
            assert (gk, gw, glp) == (wk, ww, wlp)
            np.testing.assert_array_equal(gth, wth)
        assert n == 1                                                              # the last selection: one sample of one walker
        q = s.quantiles([0.0, 0.3, 1.0], first_sample=ns - 1, walkers=[0])
        np.testing.assert_array_equal(q, np.repeat(chain[ns - 1, 0][None], 3, axis=0))


def test_adversarial_values_through_the_host_chain_route(kmc):
    """3 000 elements per dimension (several workgroups flush), one hard case per dimension, all in one select."""
    adv = sy.adversarial(3000)
    names = sorted(adv)
    nw, ns = 60, 50
    thetas = np.stack([adv[k].reshape(nw, ns) for k in names], axis=2)             # [walker][sample][dim]
    n = nw * ns
    dup = adv["heavy_duplicate"]
    below, upto = int(np.sum(dup < 0.75)), int(np.sum(dup <= 0.75))                # the duplicate fills the ranks [below, upto)
    ranks = sorted({0, 1, n // 2 - 1, n // 2, n - 2, n - 1, below - 1, below, upto - 1, upto} & set(range(n)))
    from kissmcmc_jl_amd.summary import _HostProvider
    th, lp = _HostProvider(thetas, thetas[:, :, names.index("specials")]).order_stats(ranks, logp=True)
    for d, k in enumerate(names):
        want = sy.sort_by_key(adv[k])[ranks]
        np.testing.assert_array_equal(bits(th[:, d]), bits(want), err_msg=k)       # bit for bit: -0.0 is not +0.0, a denormal stays one
        for i, r in enumerate(ranks):
            assert bits(sy.radix_select(adv[k], r)) == bits(th[i, d]), (k, r)
    np.testing.assert_array_equal(bits(lp), bits(sy.sort_by_key(adv["specials"])[ranks]))
    q = kmc.quantiles(thetas[:, :, [names.index("all_equal"), names.index("one_ulp_apart")]], [0.0, 0.25, 0.5, 0.75, 1.0])
    one = adv["all_equal"][0]
    np.testing.assert_array_equal(q[:, 0], np.full(5, one))
    np.testing.assert_array_equal(q[:, 1], [one, one, one + 0.5 * (np.nextafter(one, 2.0) - one), np.nextafter(one, 2.0), np.nextafter(one, 2.0)])
    q1 = kmc.quantiles(adv["ascending"].reshape(nw, ns), [0.5])                    # scalar walkers
    assert q1.shape == (1, 1) and q1[0, 0] == sy.quantile(adv["ascending"], 0.5)


def test_map_sample_rules(kmc):
    ns, nw, nd = 7, 9, 3
    rng = np.random.default_rng(3)
    chain = rng.standard_normal((ns, nw, nd))
    logp = -np.abs(rng.standard_normal((ns, nw))) - 1.0
    logp[[5, 2, 2], [1, 6, 4]] = 0.5                                               # three equal maxima: (2, 4) is the smallest (sample, walker)
    logp[:, 8] = -np.inf                                                           # a column of -inf
    logp[0, 0] = np.nan                                                            # ignored
    th, lg = chain.transpose(1, 0, 2), logp.T                                      # [walker][sample](dim)
    t, l, k, w = kmc.map_sample(th, lg)
    assert (k, w, l) == (2, 4, 0.5)
    np.testing.assert_array_equal(t, chain[2, 4])
    keep = np.ones(nw, dtype=bool)
    keep[[4, 6]] = False                                                           # a mask that removes the global maximum's first two
    assert kmc.map_sample(th, lg, walkers=keep)[2:] == (5, 1)
    assert kmc.map_sample(th, lg, first_sample=3)[2:] == (5, 1)
    t, l, k, w = kmc.map_sample(th, lg, walkers=[8])                               # only -inf left: still the smallest (sample, walker)
    assert (k, w, l) == (0, 8, -np.inf)
    np.testing.assert_array_equal(t, chain[0, 8])
    for sel in (dict(), dict(walkers=keep), dict(first_sample=3), dict(walkers=[8]), dict(walkers=[0])):
        assert kmc.map_sample(th, lg, **sel)[2:] == sy.argmax(chain, logp, sel.get("first_sample", 0), sel.get("walkers"))[2:]
    big = np.random.default_rng(4).standard_normal((700, 900))                     # several workgroups in stage 1
    big[[100, 650], [899, 3]] = 9.0
    assert kmc.map_sample(np.zeros((900, 700, 1)), big.T)[2:] == (100, 899)


def test_refusals(kmc):
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()

    def status(fn):
        with pytest.raises(kmc.KmcError) as e:
            fn()
        return e.value.status

    G = kmc.GaussianIso()
    with kmc.Sampler(G, 8, 2, 10, store_logp=True) as s:                            # no KMC_STORE_CHAIN
        assert status(lambda: s.order_stats([0])) == _lib.ERR_BAD_ARG
        assert status(lambda: s.map_sample()) == _lib.ERR_BAD_ARG
    with run_sampler(kmc, 8, 2, 5) as s0, kmc.Sampler(G, 8, 2, 10, store_chain=True) as s:    # no KMC_STORE_LOGP
        assert status(lambda: s.order_stats([0], logp=True)) == _lib.ERR_BAD_ARG
        assert status(lambda: s.map_sample()) == _lib.ERR_BAD_ARG
        assert status(lambda: s.order_stats([0])) == _lib.ERR_BAD_ARG              # nothing stored yet: N = 0
        # ranks out of range, too many ranks, empty selections
        n = 5 * 8
        assert status(lambda: s0.order_stats([n])) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.order_stats([-1])) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.order_stats(np.zeros(17, dtype=np.int64))) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.order_stats([0], first_sample=5)) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.order_stats([0], walkers=np.zeros(8, dtype=bool))) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.map_sample(first_sample=5)) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.quantiles([0.5], first_sample=5)) == _lib.ERR_BAD_ARG
        assert s0.order_stats([n - 1])[2] == n
    with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, stream_chain=True) as s:
        with pytest.raises(kmc.KmcError, match="kmc_chain_order_stats") as e:
            s.order_stats([0])
        assert e.value.status == _lib.ERR_UNSUPPORTED
        assert status(lambda: s.map_sample()) == _lib.ERR_UNSUPPORTED
    for kw in (dict(shard_rank=0, shard_count=2), dict(p2p=True)):
        with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, **kw) as s:
            assert status(lambda: s.order_stats([0])) == _lib.ERR_UNSUPPORTED
            assert status(lambda: s.map_sample()) == _lib.ERR_UNSUPPORTED
    # a host chain that cannot fit the device: refused from its sizes, before anything is read
    x = np.zeros(8)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    r, n = np.zeros(1, dtype=np.int64), C.c_int64()
    out = np.zeros(2)
    huge = 1 << 40
    assert L.kmc_chain_order_stats(x.ctypes.data_as(dp), None, huge, 1024, 2, 0, None, r.ctypes.data_as(ip), 1, 0, out.ctypes.data_as(dp), None,
                                   C.byref(n)) == _lib.ERR_UNSUPPORTED
    k, w, lp = C.c_int64(), C.c_int64(), C.c_double()
    assert L.kmc_chain_argmax(x.ctypes.data_as(dp), x.ctypes.data_as(dp), huge, 1024, 2, 0, None, 0, C.byref(k), C.byref(w), out.ctypes.data_as(dp),
                              C.byref(lp)) == _lib.ERR_UNSUPPORTED
    assert L.kmc_chain_order_stats(x.ctypes.data_as(dp), None, 2, 2, 2, 0, None, r.ctypes.data_as(ip), 1, 0, out.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                   C.byref(n)) == _lib.ERR_BAD_ARG                 # logp_out without logp_host
    all_nan = np.full((4, 3), np.nan)
    assert status(lambda: kmc.map_sample(np.zeros((4, 3, 1)), all_nan)) == _lib.ERR_BAD_ARG


def test_quantiles_and_summary_of_a_run(kmc):
    with run_sampler(kmc, 100, 3, 41, moments=True) as s:
        chain, logp = s.chain()
        flat = chain.reshape(-1, 3)
        srt = np.sort(flat, axis=0)
        q = [0.16, 0.5, 0.84]
        got, got_lp = s.quantiles(q, logp=True)
        want = np.array([[sy.quantile(srt[:, d], v) for d in range(3)] for v in q])
        np.testing.assert_array_equal(got, want)                                   # the stated formula on np.sort, exactly
        np.testing.assert_array_equal(got_lp, [sy.quantile(np.sort(logp.ravel()), v) for v in q])
        ref = np.quantile(flat, q, axis=0)                                         # numpy's own arithmetic: the same value to 1 ulp
        assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))
        np.testing.assert_array_equal(kmc.quantiles(chain.transpose(1, 0, 2), q), got)        # the host-chain route, same kernels
        out = s.summary(theta_true=np.zeros(3), names="xyz")
        assert list(out) == ["var", "err", "median", "mean", "mode", "std"] and out["var"] == ["x", "y", "z"]
        np.testing.assert_array_equal(out["median"], got[1])
        np.testing.assert_array_equal(out["err"], np.abs(got[1]))
        np.testing.assert_array_equal(out["mode"], s.map_sample()[0])
        np.testing.assert_allclose(out["mean"], flat.mean(axis=0), rtol=1e-12, atol=1e-12)     # (streaming moments: another summation order)
        np.testing.assert_allclose(out["std"], flat.std(axis=0, ddof=1), rtol=1e-10)
        host = kmc.summarize_run(chain.transpose(1, 0, 2), logp.T, theta_true=np.zeros(3), names="xyz")
        for col in ("err", "median", "mode"):
            np.testing.assert_array_equal(host[col], out[col])
    with run_sampler(kmc, 100, 3, 41) as s2:                                       # no moments: mean / std from the chain
        out2 = s2.summary()
        np.testing.assert_array_equal(out2["mean"], flat.mean(axis=0))
        np.testing.assert_array_equal(out2["std"], flat.std(axis=0, ddof=1))
        np.testing.assert_array_equal(out2["median"], got[1])
