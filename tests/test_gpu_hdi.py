"""GPU: highest-density intervals of a stored chain, scanned on the device (kmc_sampler_hdi, kmc_chain_hdi, Sampler.hdi, kmc.hdi and the
hdi= keyword of summary / summarize_run) against tests/hdi_yardstick.py.

The result is exact: lo, hi and start are compared for equality everywhere, and there is no tolerance in this file.

Sizes.  One workgroup of the scan takes T = 4096 consecutive window starts of a sorted column.  N = 2 (one window), 5, T and T + 1
(17 walkers x 241 samples) are the one-tile cases and the tile's edge, each with k = 1, p = 0.5, p = 0.94 and k = N - 1; N = 12301 is
three tiles and a ragged fourth, where a window ends in another tile than it starts in and, for the large k, whole tiles hold no
window.  Every shape runs in a single-probability call and in a call of several, which are different instances of the kernel."""
import numpy as np
import pytest

import hdi_yardstick as hy

pytestmark = pytest.mark.gpu

INF = np.inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(kmc, th, probs, lp=None, first_sample=0, walkers=None):
    """kmc.hdi on thetas[walker][sample](dim) equals the yardstick; returns the device's dict."""
    got = kmc.hdi(th, probs, logdensities=lp, first_sample=first_sample, walkers=walkers)
    lo, hi, start, k = hy.of_chain(th, probs, lp, first_sample, walkers)
    scalar = np.ndim(probs) == 0
    if scalar:
        lo, hi, start, k = lo[0], hi[0], start[0], int(k[0])
    assert got["lo"].shape == lo.shape and got["start"].dtype == np.int64
    np.testing.assert_array_equal(got["lo"], lo)
    np.testing.assert_array_equal(got["hi"], hi)
    np.testing.assert_array_equal(got["start"], start)
    np.testing.assert_array_equal(got["k"], k)
    assert not np.signbit(got["lo"][got["lo"] == 0.0]).any() and not np.signbit(got["hi"][got["hi"] == 0.0]).any()
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(got["width"], hi - lo)
    sel = np.asarray(th)[slice(None) if walkers is None else np.asarray(walkers)][:, first_sample:]
    assert got["n"] == sel.shape[0] * sel.shape[1]
    nan_cols = (start < 0).reshape(-1, start.shape[-1]).any(axis=0)
    np.testing.assert_array_equal(got["has_nan"], nan_cols)
    return got


def three_columns(rng, nw, ns):
    """[walker][sample][3]: a normal column, integers with many equal widths, a skewed column."""
    return np.stack([rng.standard_normal((nw, ns)), rng.integers(0, 7, size=(nw, ns)).astype(np.float64), rng.exponential(size=(nw, ns))], axis=2)


@pytest.mark.parametrize("nw, ns", [(2, 1), (1, 2), (5, 1), (1, 5), (16, 256), (17, 241)])
def test_one_tile_and_its_edge(kmc, nw, ns):
    N = nw * ns
    th = three_columns(np.random.default_rng(N + nw), nw, ns)
    ks = sorted({1, hy.span(N, 0.5), hy.span(N, 0.94), N - 1})
    probs = [0.5 if k == hy.span(N, 0.5) else 0.94 if k == hy.span(N, 0.94) else hy.prob_for(N, k) for k in ks]
    got = check(kmc, th, probs)
    assert got["k"].tolist() == ks
    for a, p in enumerate(probs):                                     # ... and one probability at a time
        one = check(kmc, th, p)
        np.testing.assert_array_equal(one["lo"], got["lo"][a])
        np.testing.assert_array_equal(one["start"], got["start"][a])


def test_several_tiles_sixteen_probabilities(kmc):
    N = 12301
    rng = np.random.default_rng(12301)
    th = np.stack([rng.standard_normal((1, N)), np.round(rng.standard_normal((1, N)), 2)], axis=2)
    ks = [1, 2, 100, 4095, 4096, 4097, 6000, 8191, 8192, 8193, 8205, 10000, 12000, 12288, 12299, 12300]
    probs = [hy.prob_for(N, k) for k in ks]
    got = check(kmc, th, probs)
    assert got["k"].tolist() == ks and got["lo"].shape == (16, 2)
    for a, p in enumerate(probs):
        one = kmc.hdi(th, p)
        assert one["k"] == ks[a]
        for key in ("lo", "hi", "start"):
            np.testing.assert_array_equal(one[key], got[key][a])
    # the same draws dealt to many walkers: the sorted column, and with it the answer, is the same
    many = kmc.hdi(th.reshape(N, 1, 2), probs[3:7])
    for key in ("lo", "hi", "start"):
        np.testing.assert_array_equal(many[key], got[key][3:7])


def test_ties(kmc):
    rng = np.random.default_rng(3)
    nw, ns = 10, 500
    th = np.stack([np.full((nw, ns), 2.5), rng.integers(-3, 4, size=(nw, ns)).astype(np.float64), rng.choice([-0.0, 0.0], size=(nw, ns)),
                   np.tile(np.arange(ns, dtype=np.float64), (nw, 1))], axis=2)
    N = nw * ns
    got = check(kmc, th, [hy.prob_for(N, 1), 0.5, 0.94])
    assert (got["start"][:, 0] == 0).all() and (got["width"][:, 0] == 0.0).all()          # the constant column
    assert (got["start"][:, 2] == 0).all() and not np.signbit(got["lo"][:, 2]).any()      # the zeros
    assert (got["start"][1:, 3] == 0).all()                                               # every window as wide as the first


def test_special_values(kmc):
    rng = np.random.default_rng(4)
    nw, ns = 6, 700                                                   # N = 4200: the infinities sort into both tiles
    a = rng.standard_normal((nw, ns))
    a[rng.random((nw, ns)) < 0.2] = INF
    a[rng.random((nw, ns)) < 0.2] = -INF
    b = np.full((nw, ns), INF)
    c = rng.standard_normal((nw, ns))
    c[rng.random((nw, ns)) < 0.7] = -INF
    th = np.stack([a, b, c], axis=2)
    N = nw * ns
    got = check(kmc, th, [hy.prob_for(N, 1), 0.5, 0.94, hy.prob_for(N, N - 1)])
    assert (got["start"][:, 1] == 0).all() and (got["lo"][:, 1] == INF).all() and np.isnan(got["width"][:, 1]).all()
    check(kmc, th, 0.94)
    check(kmc, np.array([[[-INF], [0.0], [1.0], [INF]]]), 0.5)
    check(kmc, np.full((1, 4, 1), INF), 0.5)


def test_one_nan_in_one_column_of_three(kmc):
    th = three_columns(np.random.default_rng(5), 9, 500)
    th[4, 321, 1] = np.nan
    got = check(kmc, th, [0.5, 0.94])
    assert got["has_nan"].tolist() == [False, True, False]
    assert np.isnan(got["lo"][:, 1]).all() and np.isnan(got["hi"][:, 1]).all() and (got["start"][:, 1] == -1).all()
    assert (got["start"][:, [0, 2]] >= 0).all()
    assert check(kmc, th, 0.94)["has_nan"].tolist() == [False, True, False]


def test_layouts(kmc):
    rng = np.random.default_rng(6)
    check(kmc, rng.standard_normal((12, 40)), [0.5, 0.94])                                # ndim = 1, scalar walkers
    check(kmc, rng.standard_normal((12, 40)), 0.94)
    th33 = rng.standard_normal((7, 30, 33))                                               # 231 positions a row: four gather tiles
    check(kmc, th33, [0.3, 0.94])
    check(kmc, rng.standard_normal((20, 300, 3)).astype(np.float32), [0.5, 0.94])         # floats, widened exactly
    th = three_columns(rng, 11, 130)
    lp = -0.5 * (th ** 2).sum(axis=2)
    got = check(kmc, th, [0.5, 0.94], lp=lp)                                              # the log-densities as the last column
    assert got["lo"].shape == (2, 4)
    np.testing.assert_array_equal(got["lo"][:, :3], kmc.hdi(th, [0.5, 0.94])["lo"])
    walkers, first = [0, 3, 4, 9], 17
    masked = check(kmc, th, [0.5, 0.94], lp=lp, first_sample=first, walkers=walkers)
    copied = kmc.hdi(th[walkers][:, first:], [0.5, 0.94], logdensities=lp[walkers][:, first:])
    for key in ("lo", "hi", "start", "k", "width"):
        np.testing.assert_array_equal(masked[key], copied[key])
    assert masked["n"] == copied["n"] == 4 * (130 - first)
    mask = np.zeros(11, dtype=bool)
    mask[walkers] = True
    np.testing.assert_array_equal(kmc.hdi(th, 0.94, first_sample=first, walkers=mask)["lo"], masked["lo"][1, :3])


def run_sampler(kmc, pdf, dtype="f64", **kw):
    nw, nd, G, nburn = 64, 3, 220, 20
    s = kmc.Sampler(pdf, nw, nd, G, nburn, 1, 2.0, 11, store_chain=True, store_logp=True, dtype=dtype, **kw)
    s.set_positions(0.5 + 0.1 * np.abs(np.random.default_rng(7).standard_normal((nw, nd))))
    s.run(G)
    s.sync()
    return s


@pytest.mark.parametrize("density, dtype", [("GaussianIso", "f64"), ("Exponential", "f64"), ("GaussianIso", "f32"), ("Exponential", "f32")])
def test_sampler_route(kmc, density, dtype):
    probs = [0.5, 0.94]
    with run_sampler(kmc, getattr(kmc, density)(), dtype) as s:
        assert s.samples_done == 200
        chain, clogp = s.chain()
        th, lp = chain.transpose(1, 0, 2), clogp.T
        got = s.hdi(probs, logp=True)
        host = check(kmc, th, probs, lp=lp)                           # the host route on the downloaded chain equals the yardstick ...
        for key in ("lo", "hi", "start", "k", "width", "has_nan"):    # ... and the sampler's route equals the host route
            np.testing.assert_array_equal(got[key], host[key])
        assert got["n"] == host["n"] == 200 * 64 and got["lo"].shape == (2, 4)
        np.testing.assert_array_equal(s.hdi(0.94)["lo"], got["lo"][1, :3])
        sel = s.hdi(0.5, first_sample=50, walkers=[1, 5, 8, 13, 21], logp=True)
        want = hy.of_chain(th, 0.5, lp, 50, [1, 5, 8, 13, 21])
        np.testing.assert_array_equal(sel["lo"], want[0][0])
        np.testing.assert_array_equal(sel["hi"], want[1][0])
        np.testing.assert_array_equal(sel["start"], want[2][0])
        if density == "Exponential":                                  # skewed: the interval starts below the equal-tailed one's lower end
            q = s.quantiles([0.03, 0.97])
            want_lo, want_hi = hy.of_chain(th, 0.94)[:2]
            assert (want_lo[0] < q[0]).all() and (want_hi[0] - want_lo[0] < q[1] - q[0]).all()
            assert (got["lo"][1, :3] < q[0]).all()


def test_summary_keyword(kmc):
    with run_sampler(kmc, kmc.Exponential()) as s:
        plain, with_hdi = s.summary(), s.summary(hdi=0.94)
        assert list(plain) == ["var", "median", "mean", "mode", "std"]
        assert list(with_hdi) == list(plain) + ["hdi_lo", "hdi_hi"]
        for key in plain:
            np.testing.assert_array_equal(np.asarray(with_hdi[key]), np.asarray(plain[key]))
        h = s.hdi(0.94)
        np.testing.assert_array_equal(with_hdi["hdi_lo"], h["lo"])
        np.testing.assert_array_equal(with_hdi["hdi_hi"], h["hi"])
        chain, clogp = s.chain()
        th, lp = chain.transpose(1, 0, 2), clogp.T
        run_plain, run_hdi = kmc.summarize_run(th, lp), kmc.summarize_run(th, lp, hdi=0.94)
        assert list(run_hdi) == list(run_plain) + ["hdi_lo", "hdi_hi"]
        for key in run_plain:
            np.testing.assert_array_equal(np.asarray(run_hdi[key]), np.asarray(run_plain[key]))
        np.testing.assert_array_equal(run_hdi["hdi_lo"], h["lo"])
        np.testing.assert_array_equal(run_hdi["hdi_hi"], h["hi"])


def test_repeatability(kmc):
    th = three_columns(np.random.default_rng(8), 13, 700)
    probs = [0.2, 0.5, 0.8, 0.94, 0.99]
    a, b = kmc.hdi(th, probs), kmc.hdi(th, probs)
    for key in ("lo", "hi", "width"):
        np.testing.assert_array_equal(bits(a[key]), bits(b[key]))
    np.testing.assert_array_equal(a["start"], b["start"])
    with run_sampler(kmc, kmc.GaussianIso()) as s:
        c, d = s.hdi(probs, logp=True), s.hdi(probs, logp=True)
        for key in ("lo", "hi", "width"):
            np.testing.assert_array_equal(bits(c[key]), bits(d[key]))
        np.testing.assert_array_equal(c["start"], d["start"])


def test_stage_times_and_counts(kmc):
    """The info numbers of the C call: N, the scan's tiles, the bytes it loads and a time for each stage."""
    from kissmcmc_jl_amd.summary import _HostProvider, hdi_from
    th = three_columns(np.random.default_rng(9), 17, 241)
    N, probs = 17 * 241, [0.5, 0.94]
    out = hdi_from(_HostProvider(th), probs, with_info=True)
    k = [hy.span(N, p) for p in probs]
    assert out["info"][0] == N and out["info"][1] == -(-(N - min(k)) // 4096)
    assert out["info"][2] == 8 * 3 * ((N - min(k)) + sum(N - x for x in k))
    assert (out["info"][3:] > 0).all() and out["nan_count"].tolist() == [0, 0, 0]


def status(f):
    from kissmcmc_jl_amd import KmcError
    with pytest.raises(KmcError) as e:
        f()
    return e.value.status


def test_refusals_on_the_device_routes(kmc):
    from kissmcmc_jl_amd import _lib
    G = kmc.GaussianIso()
    with kmc.Sampler(G, 8, 2, 10, store_chain=False) as s:
        with pytest.raises(kmc.KmcError, match="KMC_STORE_CHAIN") as err:
            s.hdi(0.94)
        assert err.value.status == _lib.ERR_BAD_ARG
    with kmc.Sampler(G, 8, 2, 10, store_chain=True) as s:
        s.set_positions(np.random.default_rng(1).standard_normal((8, 2)))
        s.run(10)
        with pytest.raises(kmc.KmcError, match="KMC_STORE_LOGP") as err:
            s.hdi(0.94, logp=True)
        assert err.value.status == _lib.ERR_BAD_ARG
        assert s.hdi(0.94)["n"] == 80
        assert status(lambda: s.hdi(1.0)) == _lib.ERR_BAD_ARG
        assert status(lambda: s.hdi(0.01)) == _lib.ERR_BAD_ARG                            # p N < 1
        assert status(lambda: s.hdi(0.5, first_sample=10)) == _lib.ERR_BAD_ARG            # an empty selection
        assert status(lambda: s.hdi(0.5, first_sample=9, walkers=[3])) == _lib.ERR_BAD_ARG        # N = 1
        assert status(lambda: s.hdi(list(np.linspace(0.1, 0.9, 17)))) == _lib.ERR_BAD_ARG
        assert status(lambda: s.summary(hdi=1.5)) == _lib.ERR_BAD_ARG
    with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, stream_chain=True) as s:
        with pytest.raises(kmc.KmcError, match="kmc_chain_hdi") as err:
            s.hdi(0.94)
        assert err.value.status == _lib.ERR_UNSUPPORTED
