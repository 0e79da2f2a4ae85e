"""Marginal histograms without a device: the numpy yardstick (tests/histogram_yardstick.py -- what the GPU tests compare the kernels
with) against np.histogram, np.histogram2d and np.histogramdd; the Python front end (ranges, edges, dims and pair order) on a fake
provider; hist_mode and credible_levels known answers; and every argument refusal of kmc_chain_histograms, none of which touches a device.
(Header, SYMBOLS and the Julia ccalls are compared by tests/test_c_abi.py.)"""
import ctypes as C

import numpy as np
import pytest

import histogram_yardstick as hy
import summary_yardstick as sy


# ---- the yardstick is numpy's rule -------------------------------------------------------------------------------------------------

def edge_cases():
    """name -> (x, edges)"""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(5000) * 3.0
    grid = np.round(x * 4.0) / 4.0                                               # a 0.25 grid: many elements exactly on edges
    lin = np.linspace(-2.0, 2.0, 17)                                             # edges on that grid, narrower than the data
    logx = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), 4000))
    loge = np.logspace(-3, 3, 41)
    on_edges = np.concatenate([lin, lin, np.nextafter(lin, -np.inf), np.nextafter(lin, np.inf)])
    return {
        "random": (x, np.linspace(x.min(), x.max(), 51)),
        "rounded": (grid, lin),
        "log_spaced": (np.concatenate([logx, loge]), loge),
        "one_bin": (x, np.array([-1.0, 1.5])),
        "256_bins": (x, np.linspace(-9.0, 9.0, 257)),
        "on_every_edge": (on_edges, lin),
        "irregular": (x, np.sort(rng.standard_normal(30)) * 2.0),
    }


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_yardstick_equals_np_histogram(name):
    x, e = edge_cases()[name]
    counts, outside = hy.hist1d(x, e)
    np.testing.assert_array_equal(counts, np.histogram(x, bins=e)[0])
    assert counts.dtype == np.int64 and outside.tolist() == [np.sum(x < e[0]), np.sum(x > e[-1]), 0]
    assert counts.sum() + outside.sum() == x.size
    if name == "on_every_edge":                                                  # the rule, spelt out: e[i] itself opens bin i, e[B] closes B - 1
        i = hy.bin_index(e, e)
        assert i.tolist() == list(range(e.size - 1)) + [e.size - 2]


def test_yardstick_infinities_and_nan():
    e = np.array([-1.0, 0.0, 2.0, 5.0])
    x = np.array([np.nan, -np.inf, np.inf, -1.0, 5.0, 0.0, np.nextafter(5.0, 6.0), np.nextafter(-1.0, -2.0), 4.999, np.nan])
    assert hy.bin_index(x, e).tolist() == [hy.NAN, hy.BELOW, hy.ABOVE, 0, 2, 1, hy.ABOVE, hy.BELOW, 2, hy.NAN]
    counts, outside = hy.hist1d(x, e)
    assert counts.tolist() == [1, 1, 2] and outside.tolist() == [2, 2, 2]
    finite = x[np.isfinite(x)]
    np.testing.assert_array_equal(hy.hist1d(finite, e)[0], np.histogram(finite, bins=e)[0])
    np.testing.assert_array_equal(counts, np.histogram(x[~np.isnan(x)], bins=e)[0])     # +-inf are ordinary values: outside


def test_yardstick_equals_np_histogram_with_a_bin_count():
    """np.histogram(x, bins=B) takes its own fast path (a float guess, then a fix-up against the edges): same counts as the rule on
    e = np.linspace(min, max, B + 1), rounded data and single elements included."""
    rng = np.random.default_rng(1)
    for case in range(120):
        B = int(rng.integers(1, 257))
        n = int(rng.choice([1, 2, 7, 1000]))
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
        if case % 3 == 0:
            x = np.round(x, 1)
        want, we = np.histogram(x, bins=B)
        lo, hi = (x.min() - 0.5, x.max() + 0.5) if x.min() == x.max() else (x.min(), x.max())
        e = np.linspace(lo, hi, B + 1)
        np.testing.assert_array_equal(e, we)
        np.testing.assert_array_equal(hy.hist1d(x, e)[0], want)


def test_yardstick_equals_np_histogram2d_and_histogramdd():
    rng = np.random.default_rng(2)
    for case in range(40):
        n = int(rng.choice([1, 50, 3000]))
        x, y = rng.standard_normal(n), rng.standard_normal(n) * 2.0 + 1.0
        if case % 2:
            x, y = np.round(x * 4.0) / 4.0, np.round(y * 4.0) / 4.0
        ex = np.linspace(-1.5, 1.5, int(rng.integers(1, 65)) + 1)                # narrower than the data: rows drop out
        ey = np.sort(rng.uniform(-4.0, 6.0, int(rng.integers(1, 65)) + 1))
        got = hy.hist2d(x, y, ex, ey)
        np.testing.assert_array_equal(got, np.histogram2d(x, y, bins=[ex, ey])[0].astype(np.int64))
        np.testing.assert_array_equal(got, np.histogramdd(np.stack([x, y], axis=1), bins=[ex, ey])[0].astype(np.int64))
    x = np.array([0.0, 1.0, 2.0, np.nan, 1.0, np.inf])                           # a row counts iff BOTH coordinates are inside
    y = np.array([0.0, 5.0, 2.0, 1.0, np.nan, 1.0])
    assert hy.hist2d(x, y, [0.0, 1.0, 2.0], [0.0, 1.0, 2.0]).tolist() == [[1, 0], [0, 1]]


def test_yardstick_histograms_shapes_and_pair_order():
    rng = np.random.default_rng(3)
    chain, logp = rng.standard_normal((5, 4, 6)), rng.standard_normal((5, 4))
    dims = [4, 0, 3]
    edges = np.stack([np.linspace(-1, 1, 9)] * 4)
    c1, out, c2, n = hy.histograms(chain, dims, edges, logp, first_sample=1, walkers=[3, 1], pairs=True)
    assert c1.shape == (4, 8) and out.shape == (4, 3) and c2.shape == (3, 8, 8) and n == 8
    assert hy.pair_list(3) == [(0, 1), (0, 2), (1, 2)]
    sel = chain[1:, [1, 3]].reshape(-1, 6)
    np.testing.assert_array_equal(c2[1], np.histogram2d(sel[:, 4], sel[:, 3], bins=[edges[0], edges[2]])[0])
    np.testing.assert_array_equal(c1[3], np.histogram(logp[1:, [1, 3]], bins=edges[3])[0])
    np.testing.assert_array_equal(c1.sum(1) + out.sum(1), [8] * 4)


# ---- the Python front end on a fake provider -----------------------------------------------------------------------------------------

class FakeProvider:
    """Order statistics and histograms from numpy, recording what the front end asks for."""

    def __init__(self, thetas, logp=None):
        self.chain = np.asarray(thetas).transpose(1, 0, 2)
        self.logp = None if logp is None else np.asarray(logp).T
        self.n, self.ndim = self.chain.shape[0] * self.chain.shape[1], self.chain.shape[2]
        self.rank_calls, self.hist_calls = [], []

    def order_stats(self, ranks, logp=False):
        self.rank_calls.append(list(ranks))
        th, lp, _ = sy.order_stats(self.chain, ranks, self.logp if logp else None)
        return th, lp

    def histograms(self, dims, edges, logp=False, pairs=False):
        self.hist_calls.append((list(dims), np.array(edges), logp, pairs))
        c1, out, c2, _ = hy.histograms(self.chain, list(dims), edges, self.logp if logp else None, pairs=pairs)
        return c1, out, c2


@pytest.fixture(scope="module")
def run():
    rng = np.random.default_rng(0)
    th = rng.standard_normal((6, 50, 4)) * [1.0, 2.0, 0.5, 30.0] + [0.0, 5.0, -1.0, 100.0]      # [walker][sample][dim]
    th[:, :, 2] = np.round(th[:, :, 2], 1)
    return th, rng.standard_normal((6, 50))


def test_default_range_reproduces_np_histogram_edges_included(kmc, run):
    from kissmcmc_jl_amd.summary import histogram_from
    th, lp = run
    flat = th.reshape(-1, 4)
    for B in (1, 7, 40, 256):
        p = FakeProvider(th, lp)
        counts, edges, outside = histogram_from(p, bins=B, logp=True)
        assert p.rank_calls == [[0, flat.shape[0] - 1]]                          # minimum and maximum: one call for all columns
        assert counts.shape == (5, B) and edges.shape == (5, B + 1) and counts.dtype == np.int64
        for c, col in enumerate(list(flat.T) + [lp.ravel()]):
            want, we = np.histogram(col, bins=B)
            np.testing.assert_array_equal(edges[c], we)                          # bit for bit
            np.testing.assert_array_equal(counts[c], want)
        assert not outside.any()


def test_equal_limits_are_widened_as_numpy_does(kmc):
    from kissmcmc_jl_amd.summary import histogram_from
    th = np.full((4, 5, 2), 3.25)
    th[:, :, 1] = np.arange(20).reshape(4, 5)
    counts, edges, outside = histogram_from(FakeProvider(th), bins=10)
    want, we = np.histogram(th[:, :, 0], bins=10)
    np.testing.assert_array_equal(edges[0], we)
    assert edges[0, 0] == 2.75 and edges[0, -1] == 3.75
    np.testing.assert_array_equal(counts[0], want)
    np.testing.assert_array_equal(counts[1], np.histogram(th[:, :, 1], bins=10)[0])
    one = np.full((1, 1, 1), -7.0)                                               # a single element
    counts, edges, _ = histogram_from(FakeProvider(one), bins=3)
    np.testing.assert_array_equal(edges[0], np.histogram(one, bins=3)[1])
    assert counts.tolist() == [np.histogram(one, bins=3)[0].tolist()]


def test_ranges_and_edge_arrays(kmc, run):
    from kissmcmc_jl_amd.summary import histogram_from, quantiles_from
    th, lp = run
    flat = th.reshape(-1, 4)
    # one (lo, hi) for every column: np.histogram(range=...)
    counts, edges, outside = histogram_from(FakeProvider(th), bins=12, range=(-2.0, 3.0))
    for c in range(4):
        want, we = np.histogram(flat[:, c], bins=12, range=(-2.0, 3.0))
        np.testing.assert_array_equal(edges[c], we)
        np.testing.assert_array_equal(counts[c], want)
        assert outside[c].tolist() == [np.sum(flat[:, c] < -2.0), np.sum(flat[:, c] > 3.0), 0]
    # a range per column, with the log-densities as the last
    rng5 = np.array([[-1, 1], [0, 9], [-2, 0], [50, 150], [-1, 0.5]], dtype=float)
    counts, edges, outside = histogram_from(FakeProvider(th, lp), bins=9, range=rng5, logp=True)
    for c, col in enumerate(list(flat.T) + [lp.ravel()]):
        want, we = np.histogram(col, bins=9, range=tuple(rng5[c]))
        np.testing.assert_array_equal(edges[c], we)
        np.testing.assert_array_equal(counts[c], want)
    np.testing.assert_array_equal(counts.sum(1) + outside.sum(1), [flat.shape[0]] * 5)
    # quantile limits
    p = FakeProvider(th)
    counts, edges, outside = histogram_from(p, bins=20, quantile_range=(0.001, 0.999))
    q = quantiles_from(FakeProvider(th), [0.001, 0.999])
    for c in range(4):
        np.testing.assert_array_equal(edges[c], np.linspace(q[0, c], q[1, c], 21))
        np.testing.assert_array_equal(counts[c], np.histogram(flat[:, c], bins=edges[c])[0])
    assert outside[:, :2].sum() > 0 and not outside[:, 2].any()
    # edges given: shared, and per column
    e = np.array([-3.0, -1.0, 0.0, 0.5, 4.0])
    counts, edges, _ = histogram_from(FakeProvider(th), bins=e, dims=[1, 0])
    assert edges.shape == (2, 5) and np.all(edges == e)
    np.testing.assert_array_equal(counts, [np.histogram(flat[:, 1], bins=e)[0], np.histogram(flat[:, 0], bins=e)[0]])
    e2 = np.stack([e, e * 2.0 + 5.0])
    counts, edges, _ = histogram_from(FakeProvider(th), bins=e2, dims=[0, 1])
    np.testing.assert_array_equal(counts[1], np.histogram(flat[:, 1], bins=e2[1])[0])
    for bad in (dict(bins=0), dict(bins=np.zeros((3, 5))), dict(bins=5, range=(1.0, 2.0, 3.0)), dict(bins=5, range=(2.0, 1.0)),
                dict(bins=5, range=(0.0, np.inf)), dict(bins=5, dims=[]), dict(bins=5, quantile_range=(0.1,))):
        with pytest.raises(ValueError):
            histogram_from(FakeProvider(th), **bad)
    with pytest.raises(IndexError):
        histogram_from(FakeProvider(th), bins=5, dims=[4])


def test_corner_dims_and_pair_order(kmc, run):
    from kissmcmc_jl_amd.summary import corner_from
    th, _ = run
    flat = th.reshape(-1, 4)
    p = FakeProvider(th)
    out = corner_from(p, bins=8, dims=[3, 0, 2])
    assert list(out) == ["dims", "pairs", "edges", "hist1d", "outside", "hist2d", "n"]
    assert out["dims"] == [3, 0, 2] and out["pairs"] == [(3, 0), (3, 2), (0, 2)] and out["n"] == flat.shape[0]
    assert len(p.hist_calls) == 1 and p.hist_calls[0][0] == [3, 0, 2] and p.hist_calls[0][2:] == (False, True)
    assert out["hist2d"].shape == (3, 8, 8) and out["hist1d"].shape == (3, 8) and out["edges"].shape == (3, 9)
    for i, d in enumerate([3, 0, 2]):
        want, we = np.histogram(flat[:, d], bins=8)
        np.testing.assert_array_equal(out["edges"][i], we)
        np.testing.assert_array_equal(out["hist1d"][i], want)
    for k, (a, b) in enumerate(out["pairs"]):
        ea, eb = out["edges"][out["dims"].index(a)], out["edges"][out["dims"].index(b)]
        np.testing.assert_array_equal(out["hist2d"][k], np.histogram2d(flat[:, a], flat[:, b], bins=[ea, eb])[0])
        np.testing.assert_array_equal(out["hist2d"][k].sum(axis=1), out["hist1d"][out["dims"].index(a)])     # full ranges: the marginals
    full = corner_from(FakeProvider(th), bins=4)
    assert full["dims"] == [0, 1, 2, 3] and full["pairs"] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def test_hist_mode_and_credible_levels_known_answers(kmc):
    e = np.array([0.0, 1.0, 3.0, 4.0, 8.0])
    assert kmc.hist_mode([1, 5, 2, 5], e) == 2.0                                 # the first of the two fullest bins: [1, 3)
    assert kmc.hist_mode([0, 0, 0, 9], e) == 6.0
    np.testing.assert_array_equal(kmc.hist_mode([[1, 5, 2, 5], [7, 0, 0, 7]], np.stack([e, e + 10.0])), [2.0, 10.5])
    h = np.array([[4, 3], [2, 1]])                                               # cumulative shares, fullest first: 0.4, 0.7, 0.9, 1.0
    np.testing.assert_array_equal(kmc.credible_levels(h, [0.4, 0.5, 0.7, 0.75, 1.0]), [4, 3, 3, 2, 1])
    assert kmc.credible_levels(h, 0.05).tolist() == [4]
    g = np.zeros((5, 5), dtype=np.int64)
    g[2, 2], g[2, 3], g[0, 0] = 60, 30, 10
    assert kmc.credible_levels(g).tolist() == [60, 30]                           # 0.393 -> the peak alone; 0.865 -> peak and neighbour
    for t, p in zip(kmc.credible_levels(g, [0.393, 0.865, 0.95]), [0.393, 0.865, 0.95]):
        assert g[g >= t].sum() >= p * g.sum() and g[g > t].sum() < p * g.sum()   # the smallest super-level set that holds the share
    with pytest.raises(ValueError):
        kmc.credible_levels(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        kmc.credible_levels(h, [0.0])


# ---- the library's refusals, none of which touches a device --------------------------------------------------------------------------

def test_every_bad_argument_is_refused_before_the_device(kmc):
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    dp, ip, i32p, bp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    ns, nw, nd = 4, 3, 5
    chain, logp = np.zeros((ns, nw, nd)), np.zeros((ns, nw))
    keep = []

    def call(dims=None, nbins=4, edges=None, first=0, mask=None, pairs=False, with_logp=False, chain_=chain, shape=(ns, nw, nd), device=10 ** 6):
        nsel = nd if dims is None else len(dims)
        ncols = nsel + (1 if with_logp else 0)
        e = np.ascontiguousarray(np.tile(np.linspace(0.0, 1.0, max(nbins, 0) + 1), (ncols, 1)) if edges is None else edges, dtype=np.float64)
        d = None if dims is None else np.ascontiguousarray(dims, dtype=np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        B = max(nbins, 1)
        c1, out = np.zeros((ncols, B), dtype=np.int64), np.zeros((ncols, 3), dtype=np.int64)
        c2 = np.zeros((max(nsel * (nsel - 1) // 2, 1), B, B), dtype=np.int64) if pairs else None
        n = C.c_int64(-1)
        keep.extend([e, d, m, c1, out, c2])
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return L.kmc_chain_histograms(p(chain_, dp), p(logp, dp) if with_logp else None, *shape, first, p(m, bp), p(d, i32p), 0 if d is None else d.size,
                                      p(e, dp), nbins, device, p(c1, ip), p(out, ip), p(c2, ip), C.byref(n))

    # a request with nothing wrong gets as far as the device ordinal (10^6: out of range, or no device at all) -- so everything below
    # is refused for its own reason, before that point
    assert call() in (_lib.ERR_BAD_ARG, _lib.ERR_NO_DEVICE) and b"device" in L.kmc_last_error()
    assert call(dims=[4, 0], pairs=True, with_logp=True) in (_lib.ERR_BAD_ARG, _lib.ERR_NO_DEVICE) and b"device" in L.kmc_last_error()

    def refused(needle, **kw):
        assert call(**kw) == _lib.ERR_BAD_ARG, kw
        assert needle in L.kmc_last_error().decode(), (kw, L.kmc_last_error())

    refused("1..256", nbins=0)
    refused("1..256", nbins=257)
    assert call(nbins=256) != _lib.ERR_BAD_ARG or b"device" in L.kmc_last_error()
    refused("1..64", nbins=65, pairs=True, dims=[0, 1])
    assert b"device" in (call(nbins=64, pairs=True, dims=[0, 1]), L.kmc_last_error())[1]
    refused("between 2 and 16", pairs=True, dims=[2])
    refused("between 2 and 16", pairs=True, dims=list(range(17)), shape=(ns, nw, 40), chain_=np.zeros((ns, nw, 40)))
    assert b"device" in (call(pairs=True, dims=list(range(16)), shape=(ns, nw, 40), chain_=np.zeros((ns, nw, 40))), L.kmc_last_error())[1]
    refused("outside [0, 5)", dims=[0, 5])
    refused("outside [0, 5)", dims=[-1])
    refused("selected twice", dims=[1, 3, 1])
    for bad in ([0.0, 1.0, 1.0, 2.0, 3.0], [0.0, 2.0, 1.0, 3.0, 4.0], [0.0, 1.0, np.nan, 3.0, 4.0], [-np.inf, 1.0, 2.0, 3.0, 4.0], [0.0, 1.0, 2.0, 3.0, np.inf]):
        e = np.tile(np.linspace(0.0, 1.0, 5), (nd, 1))
        e[nd - 1] = bad                                                          # the last column's edges: every column is checked
        refused("finite and strictly increasing", edges=e)
    e = np.tile(np.linspace(0.0, 1.0, 5), (3, 1))
    e[2] = [3.0, 2.0, 1.0, 0.0, -1.0]
    refused("finite and strictly increasing", edges=e, dims=[0, 1], with_logp=True)     # the log-densities' column too
    refused("empty", first=ns)
    refused("empty", mask=[0, 0, 0])
    refused("first_sample", first=ns + 1)
    refused("first_sample", first=-1)
    refused("nsamples, nwalkers, ndim", shape=(0, nw, nd))
    refused("null", chain_=None)
    # the sampler call with no sampler
    assert L.kmc_sampler_histograms(None, 0, None, None, 0, None, 4, 0, None, None, None, None) == _lib.ERR_BAD_ARG
    # the pair plan: pure arithmetic
    ppg, ng, lds = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.kmc_hist_pair_plan(7, 64, C.byref(ppg), C.byref(ng), C.byref(lds)) == _lib.OK
    assert 64 * 1024 <= lds.value <= 160 * 1024 and ppg.value * 64 * 64 * 4 <= lds.value
    assert ng.value == -(-21 // ppg.value) and ng.value >= 2
    assert L.kmc_hist_pair_plan(2, 1, C.byref(ppg), C.byref(ng), C.byref(lds)) == _lib.OK and (ppg.value, ng.value) == (1, 1)
    assert L.kmc_hist_pair_plan(16, 8, C.byref(ppg), C.byref(ng), C.byref(lds)) == _lib.OK and ppg.value * ng.value >= 120
    for bad in ((1, 8), (17, 8), (4, 0), (4, 65)):
        assert L.kmc_hist_pair_plan(*bad, None, None, None) == _lib.ERR_BAD_ARG
