"""GPU: the posterior covariance matrix summed on the device (kmc_sampler_covariance, kmc_chain_covariance; Sampler.covariance,
kmc.covariance) against its exact restatement (tests/covariance_yardstick.py).

Lane maps.  The operand and accumulator maps of the double-precision matrix instruction are checked first and exactly: on integer data
whose column sums are multiples of n every mean, centred value, product and sum is an integer far below 2^53, so the device must
return the integer sums divided once by n - 1, bit for bit, whatever order it adds in.

Tolerance (derived, not measured).  Every sum the device returns is a sum S of N terms t_k added in an order of the library's and of
the instruction's, each product either rounded or fused into an addition: at most one rounding per term.  Adding N numbers in ANY order
commits at most N - 1 roundings, each relative to a partial sum of at most sum |t_k| (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 4.2), and the rounded products add one more unit: |computed - exact| <= N u sum |t_k| to first order,
u = 2^-53.  The yardstick adds the exact products exactly (an error-free product split, math.fsum) and rounds once; the division that
follows (by n, by n - 1) rounds once on each side: at most three further units.  Hence the bound asserted everywhere:

    |got - exact| <= (N + 4) 2^-53 sum |t_k|

For cov, N = n and the terms are (x_a - mean_a)(x_b - mean_b) with the centred values formed in double as the definition writes them
and mean the DEVICE's (its second pass centres on what its first pass found), so the yardstick is given that mean.  For mean, N = n,
against sum |x|."""
import numpy as np
import pytest

import covariance_yardstick as cy

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(chain, logp=None):
    """[sample][walker][dim] -> the thetas[walker][sample][dim], logdensities[walker][sample] of the module-level functions."""
    return chain.transpose(1, 0, 2), None if logp is None else logp.T


def check(got, chain, logp=None, first=0, walkers=None, label=""):
    """A covariance dict against the yardstick on the selection; returns the yardstick's sums."""
    x = cy.rows_of(chain, logp, first, walkers)
    n, C = x.shape
    assert got["n"] == n and got["mean"].shape == (C,) and got["cov"].shape == got["corr"].shape == (C, C) and got["std"].shape == (C,)
    want = cy.sums(x, mean=got["mean"])
    em, bm = np.abs(got["mean"] - want["col_sum"] / n) * n, (n + 4) * U * want["col_abs"]
    ec, bc = np.abs(got["cov"] - want["cross"] / (n - 1)) * (n - 1), (n + 4) * U * want["cross_abs"]
    print(f"{label} n={n} C={C}: mean err/bound {np.max(em / np.maximum(bm, 1e-300)):.3f}, cov err/bound {np.max(ec / np.maximum(bc, 1e-300)):.3f}")
    assert np.all(em <= bm) and np.all(ec <= bc)
    assert (bits(got["cov"]) == bits(got["cov"].T)).all()
    wc, ws = cy.correlation(got["cov"])
    assert (bits(got["corr"]) == bits(wc)).all() and (bits(got["std"]) == bits(ws)).all()
    return want


def same(a, b):
    return all((bits(a[k]) == bits(b[k])).all() for k in ("mean", "cov", "corr", "std")) and a["n"] == b["n"]


def gauss_chain(seed, ns, nw, nd):
    """A correlated, shifted, unevenly scaled sample: chain[sample][walker][dim]."""
    rng = np.random.default_rng(seed)
    mix = np.eye(nd) + 0.3 * rng.standard_normal((nd, nd)) / np.sqrt(nd)
    scale, shift = np.exp(rng.uniform(-3, 3, nd)), 10.0 * rng.standard_normal(nd)
    return (rng.standard_normal((ns, nw, nd)) @ mix) * scale + shift


def test_lane_maps_exactly(kmc):
    """Integers in [-8, 8], n = 64 rows, every column sum a multiple of n, C = 33 (three tiles, the last with one column), no two columns
    alike and nothing symmetric about the pattern: a swapped row / column map, or the accumulator map of the f32 forms, puts sums into
    the wrong entries and fails; the right maps give the integer sums divided once by n - 1, exactly."""
    n, C = 64, 33
    rng = np.random.default_rng(2)
    x = rng.integers(-8, 9, size=(n, C)).astype(np.int64)
    for c in range(C):
        r = 0
        while x[:, c].sum() % n:                                                    # walk the sum down to a multiple of n
            if x[r % n, c] > -8:
                x[r % n, c] -= 1
            r += 1
    assert (x.sum(axis=0) % n == 0).all() and np.abs(x).max() <= 8
    assert len({tuple(col) for col in x.T.tolist()}) == C and len({tuple(np.abs(col)) for col in x.T.tolist()}) == C
    mean = x.sum(axis=0) // n
    d = x - mean[None, :]
    S = d.T @ d                                                                     # int64: exact
    assert not (S[:16, 16:32] == S[:16, 16:32].T).all()
    chain = x.reshape(16, 4, C).astype(np.float64)                                  # 16 samples of 4 walkers
    got = kmc.covariance(*host(chain))
    assert got["n"] == n and (got["mean"] == mean).all()
    want = S.astype(np.float64) / float(n - 1)
    wrong = np.argwhere(got["cov"] != want)
    assert wrong.size == 0, f"{len(wrong)} entries differ, the first at {wrong[0]}: {got['cov'][tuple(wrong[0])]} != {want[tuple(wrong[0])]}"
    lp = chain[:, :, 7] * 2.0 - chain[:, :, 20]                                      # ... and with the log-densities as column 33
    gl = kmc.covariance(chain.transpose(1, 0, 2), lp.T)
    dl = 2 * d[:, 7] - d[:, 20]
    assert (gl["cov"][:C, :C] == want).all() and (gl["cov"][C, :C] == (dl @ d) / float(n - 1)).all() and gl["cov"][C, C] == (dl @ dl) / float(n - 1)


@pytest.mark.parametrize("nd,with_logp", [(1, False), (3, True), (15, False), (16, False), (17, False), (32, False), (33, False)])
def test_tile_edges(kmc, nd, with_logp):
    """C = 1, 3 + logp, 15, 16, 17, 32, 33 at 5 walkers x 41 samples: 205 rows, not a multiple of 4."""
    chain = gauss_chain(nd, 41, 5, nd)
    logp = -0.5 * np.sum(np.random.default_rng(1).standard_normal((41, 5, 2)) ** 2, axis=2) if with_logp else None
    got = kmc.covariance(*host(chain, logp))
    check(got, chain, logp, label=f"tile edge ndim={nd}")
    assert same(got, kmc.covariance(*host(chain, logp)))
    if nd > 1:                                                                       # (a sanity check of the yardstick itself, loose)
        ref = np.cov(cy.rows_of(chain, logp), rowvar=False)
        assert np.all(np.abs(got["cov"] - ref) <= 1e-9 * np.abs(ref) + 1e-12 * np.outer(got["std"], got["std"]))


def test_strip_edge(kmc):
    """ndim = 16 strip_tiles + 1: the first row of tile pairs is cut into two strips, the second of a single pair."""
    nd = 16 * kmc.cov_plan(1)["strip_tiles"] + 1
    assert kmc.cov_plan(nd)["nstrips"] == kmc.cov_plan(nd - 1)["nstrips"] + 2
    chain = gauss_chain(4, 9, 2, nd)
    check(kmc.covariance(*host(chain)), chain, label="strip edge")


def test_row_partition(kmc):
    """Row counts about the block of rows a wave takes at a time: the fold sees 1 partial sum (less than a block, a block less one row, a
    full block), 2 (a block and one row) and 3."""
    B = kmc.cov_plan(5)["rows_per_wave_block"]
    assert B % 4 == 0
    for rows in (2, B - 1, B, B + 1, 2 * B + 3):
        chain = gauss_chain(rows, rows, 1, 5)
        raw = kmc.chain_covariance.covariance_raw_from(kmc.summary._HostProvider(*host(chain)))
        assert raw["info"][0] == rows and raw["info"][1] == (rows + B - 1) // B
        check(kmc.covariance(*host(chain)), chain, label=f"{rows} rows")
    chain = gauss_chain(7, B // 2 + 1, 2, 5)                                         # B + 2 rows in two walkers
    check(kmc.covariance(*host(chain)), chain, label="two walkers")


def test_selection(kmc):
    ns, nw, nd = 23, 6, 4
    chain = gauss_chain(9, ns, nw, nd)
    logp = -np.abs(gauss_chain(10, ns, nw, 1))[:, :, 0]
    every_other = np.arange(nw) % 2 == 0
    for first, walkers in ((5, None), (0, [4]), (3, every_other), (ns - 1, None)):
        got = kmc.covariance(*host(chain, logp), first_sample=first, walkers=walkers)
        check(got, chain, logp, first, walkers, label=f"first={first} walkers={walkers}")
        poisoned, plogp = chain.copy(), logp.copy()                                  # NaN in every row that is not selected
        keep = np.zeros((ns, nw), dtype=bool)
        keep[first:, cy.walkers_of(nw, walkers)] = True
        poisoned[~keep] = np.nan
        plogp[~keep] = np.nan
        gp = kmc.covariance(*host(poisoned, plogp), first_sample=first, walkers=walkers)
        assert np.isfinite(gp["cov"]).all() and np.isfinite(gp["mean"]).all()
        check(gp, poisoned, plogp, first, walkers, label="  unselected rows NaN")
        assert same(got, gp)


def test_nan_and_inf_stay_in_their_columns(kmc):
    chain = gauss_chain(12, 19, 3, 18)
    for bad in (np.nan, np.inf):
        c = chain.copy()
        c[7, 1, 16] = bad                                                            # one selected element, in the second tile
        got = kmc.covariance(*host(c))
        hit = np.zeros((18, 18), dtype=bool)
        hit[16, :] = hit[:, 16] = True
        assert np.isnan(got["cov"][hit]).all() and np.isfinite(got["cov"][~hit]).all()
        assert (np.isnan(got["mean"]) if bad != bad else np.isinf(got["mean"]))[16] and np.isfinite(np.delete(got["mean"], 16)).all()
        sub = np.delete(np.delete(got["cov"], 16, axis=0), 16, axis=1)               # the other columns: as if column 16 were not there
        corr, std = cy.correlation(sub)
        check({"n": got["n"], "mean": np.delete(got["mean"], 16), "cov": sub, "corr": corr, "std": std}, np.delete(c, 16, axis=2), label=f"beside {bad}")
    c = chain.copy()
    c[:, :, 3] = 2.5                                                                 # a constant column: variance 0, NaN correlations, no error
    got = kmc.covariance(*host(c))
    assert got["mean"][3] == 2.5 and (got["cov"][3] == 0.0).all() and np.isnan(got["corr"][3]).all() and got["corr"][0, 0] == 1.0


def run_sampler(kmc, nw, nd, ns, nburn=3, seed=5, **kw):
    G = nburn + ns
    s = kmc.Sampler(kmc.GaussianIso(), nw, nd, G, nburn, 1, 2.0, seed, store_chain=True, store_logp=True, **kw)
    s.set_positions(np.random.default_rng(seed).standard_normal((nw, nd)))
    s.run(G)
    s.sync()
    return s


@pytest.mark.parametrize("nd,kw", [(3, {}), (5, {}), (4, {"dtype": "f32"}), (5, {"dtype": "f32"})])
def test_sampler_route(kmc, nd, kw):
    """The chain a sampler holds -- rows padded (ld != ndim) at ndim = 3 and 5, floats with dtype="f32" -- with the log-densities as the
    last column: within the bound of the yardstick on s.chain(), bit-equal to kmc.covariance on s.chain() with the same selection,
    and bit-equal from call to call."""
    with run_sampler(kmc, 12, nd, 30, **kw) as s:
        chain, logp = s.chain()
        for first, walkers, lp in ((0, None, True), (4, [1, 2, 5, 11], True), (0, None, False)):
            got = s.covariance(first_sample=first, walkers=walkers, logp=lp)
            check(got, chain, logp if lp else None, first, walkers, label=f"sampler ndim={nd} {kw}")
            assert same(got, s.covariance(first_sample=first, walkers=walkers, logp=lp))
            th, ld = host(chain, logp)
            assert same(got, kmc.covariance(th, ld if lp else None, first_sample=first, walkers=walkers))


def test_sampler_refusals(kmc):
    from kissmcmc_jl_amd import _lib

    def status(fn):
        with pytest.raises(kmc.KmcError) as e:
            fn()
        return e.value.status

    G = kmc.GaussianIso()
    with kmc.Sampler(G, 8, 2, 10, store_logp=True) as s:                            # no KMC_STORE_CHAIN
        assert status(lambda: s.covariance()) == _lib.ERR_BAD_ARG
    with kmc.Sampler(G, 8, 2, 30, 3, 1, 2.0, 1, store_chain=True) as s:
        assert status(lambda: s.covariance()) == _lib.ERR_BAD_ARG                   # nothing stored yet: an empty selection
        s.set_positions(np.random.default_rng(0).standard_normal((8, 2)))
        s.run(30)
        s.sync()
        assert status(lambda: s.covariance(logp=True)) == _lib.ERR_BAD_ARG          # no KMC_STORE_LOGP
        assert s.covariance()["n"] == 27 * 8
        assert status(lambda: s.covariance(walkers=np.zeros(8, dtype=bool))) == _lib.ERR_BAD_ARG
        assert status(lambda: s.covariance(first_sample=26, walkers=[3])) == _lib.ERR_BAD_ARG       # n = 1
        assert s.covariance(first_sample=25, walkers=[3])["n"] == 2
    with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, stream_chain=True) as s:
        with pytest.raises(kmc.KmcError, match="kmc_chain_covariance") as err:
            s.covariance()
        assert err.value.status == _lib.ERR_UNSUPPORTED
    for kw in (dict(shard_rank=0, shard_count=2), dict(p2p=True)):
        with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, **kw) as s:
            assert status(lambda: s.covariance()) == _lib.ERR_UNSUPPORTED


def test_summary_with_covariance(kmc):
    with run_sampler(kmc, 10, 3, 25) as s:
        plain, full, c = s.summary(), s.summary(covariance=True), s.covariance()
        assert list(plain) == ["var", "median", "mean", "mode", "std"]              # the default output: key for key what it was
        assert list(full) == list(plain) + ["cov", "corr"]
        assert (bits(full["cov"]) == bits(c["cov"])).all() and (bits(full["corr"]) == bits(c["corr"])).all()
        chain, logp = s.chain()
        th, ld = host(chain, logp)
        hp, hf = kmc.summarize_run(th, ld), kmc.summarize_run(th, ld, covariance=True)
        assert list(hf) == list(hp) + ["cov", "corr"] and list(hp) == list(plain)
        assert (bits(hf["cov"]) == bits(c["cov"])).all() and (bits(hf["corr"]) == bits(c["corr"])).all()
