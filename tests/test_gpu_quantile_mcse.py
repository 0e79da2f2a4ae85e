"""GPU: the effective sample size and Monte-Carlo standard error of quantiles from bit-packed indicator chains (kmc_*_indicator_lags,
kmc_*_quantile_mcse, Sampler.indicator_lags / quantile_mcse, kmc.indicator_lags / quantile_mcse, summary(quantile_mcse=True)) against
tests/quantile_mcse_yardstick.py.

The device stage is integers: the counts of the ones and the lag counts D_t are compared for equality with counted pairs, at chain
lengths on both sides of a word edge, with every lag from 1 to h - 1, and however the lags are cut into calls.

The whole call.  quantile, lower and upper are elements of the chain (or the interpolation of two) and mcse is half their difference:
compared bit for bit, as are T and flags.  The lag counts are the same integers and the chain moments the same operations on the same
counts as the yardstick's, and kmc_convergence_stats is the yardstick's stats operation for operation, so ess is expected to be EQUAL; it
is asserted within rtol 1e-12 and the test prints which it was (on the MI355X it was equality in every case).  lower and upper depend on
a and b through floor(a S) and ceil(b S); the library's Beta quantile and scipy's differ by up to 1.5e-12 relatively
(tests/test_quantile_mcse_cpu.py), i.e. by less than 1e-6 in a S at S <= 1e5, so the yardstick's a S and b S are asserted to lie more
than 1e-4 from an integer -- else another seed is to be taken.

End to end.  mcse / (sqrt(p (1 - p) / S) / phi(z_p)) on convergence_yardstick.ar1, 64 walkers x 500 samples: independent draws inside
[0.6, 1.6] (the yardstick alone gave 0.80 ... 1.33 over ten seeds), phi = 0.7 at least 1.2 (the yardstick: 1.39 ... 2.87)."""
import numpy as np
import pytest

import convergence_yardstick as cy
import quantile_mcse_yardstick as qy
import rank_yardstick as ry

pytestmark = pytest.mark.gpu

KEYS = ["quantile", "ess", "mcse", "lower", "upper", "T", "flags", "m", "h"]


def host(chain, logp=None):
    """[sample][walker][dim] -> the thetas[walker][sample][dim], logdensities[walker][sample] of the module-level functions."""
    return chain.transpose(1, 0, 2), None if logp is None else logp.T


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and bool(np.all(a == b))
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def thresholds_of(rng, x, nprobs):
    """[nprobs][ncols]: order statistics of the columns of x[ncols][m][h] at random places, so that ties with a threshold occur."""
    flat = np.sort(x.reshape(x.shape[0], -1), axis=1)
    at = rng.integers(0, flat.shape[1], size=(nprobs, x.shape[0]))
    return np.ascontiguousarray(flat[np.arange(x.shape[0])[None, :], at])


def check_stage(kmc, chain, logp, thr, first=0, walkers=None, split=False, cuts=("one", "32", "each")):
    th, lp = host(chain, logp)
    x, m, h = ry.pooled(chain, logp, first, walkers, split)
    I = qy.indicators(x, thr)
    want_ones, want = I.sum(axis=-1), qy.lag_counts(I, 1, h - 1)
    kw = dict(first_sample=first, walkers=walkers, split=split)
    got = kmc.indicator_lags(th, thr, lp, 1, h - 1, **kw)
    assert (got["m"], got["h"]) == (m, h) and got["lagcount"].dtype == np.uint64 and got["ones"].dtype == np.int64
    np.testing.assert_array_equal(got["ones"], want_ones)
    np.testing.assert_array_equal(got["lagcount"].astype(np.int64), want)
    if "32" in cuts and h - 1 > 32:
        a, b = kmc.indicator_lags(th, thr, lp, 1, 32, **kw), kmc.indicator_lags(th, thr, lp, 33, h - 1 - 32, **kw)
        assert np.concatenate([a["lagcount"], b["lagcount"]], axis=2).tobytes() == got["lagcount"].tobytes()
    if "each" in cuts:
        for t in range(1, h):
            one = kmc.indicator_lags(th, thr, lp, t, 1, **kw)
            assert one["lagcount"][:, :, 0].tobytes() == np.ascontiguousarray(got["lagcount"][:, :, t - 1]).tobytes(), t
    return got


@pytest.mark.parametrize("h,m,nd,with_logp,nprobs", [(4, 2, 1, False, 1), (63, 3, 3, True, 5), (64, 70, 33, False, 16), (65, 2, 33, False, 5),
                                                     (127, 3, 1, False, 16), (128, 70, 3, True, 1), (129, 3, 33, False, 16),
                                                     (200, 70, 3, True, 5)])
def test_device_stage_is_counted_pairs(kmc, h, m, nd, with_logp, nprobs):
    """Unsplit chains of h samples, a word edge on either side of h; every lag 1 .. h - 1 (t = 63, 64, 65, 127, 128 cross a word), cut as
    one call, as 32 + the rest, and one lag per call: the same integers each way."""
    rng = np.random.default_rng(1000 + h)
    chain = np.round(rng.standard_normal((h, m, nd)), 1)                            # (rounded: ties with the thresholds)
    logp = rng.standard_normal((h, m)) if with_logp else None
    x, _, _ = ry.pooled(chain, logp, 0, None, False)
    check_stage(kmc, chain, logp, thresholds_of(rng, x, nprobs))


def test_device_stage_over_two_staged_runs_of_words(kmc):
    """412 chains of 300 samples, 5 words each: 2060 words per (probability, column), more than one workgroup stages, with a chain
    lying across the edge; 299 lags, more than the 256 lanes of a workgroup."""
    plan = kmc.indicator_plan()
    assert 412 * 5 > plan["chunk_words"] and plan["chunk_words"] % 5 != 0 and 299 > plan["threads"]
    rng = np.random.default_rng(7)
    chain = cy.ar1(rng, 0.8, 300, 412, 1)
    x, _, _ = ry.pooled(chain, None, 0, None, False)
    check_stage(kmc, chain, None, thresholds_of(rng, x, 2), cuts=("one", "32"))


def test_device_stage_split_odd_n_mask_and_first_sample(kmc):
    """A split with an odd n (the middle sample belongs to no chain), five scattered walkers of 70, first_sample = 7, the log-densities
    as the last column: no pair straddles the halves or reaches before first_sample."""
    rng = np.random.default_rng(3)
    ns, nw, nd, first = 7 + 2 * 65 + 1, 70, 3, 7
    chain, logp = np.round(rng.standard_normal((ns, nw, nd)), 1), rng.standard_normal((ns, nw))
    mask = np.zeros(nw, dtype=bool)
    mask[[3, 17, 40, 60, 69]] = True
    x, m, h = ry.pooled(chain, logp, first, mask, True)
    assert (m, h) == (10, 65)
    check_stage(kmc, chain, logp, thresholds_of(rng, x, 5), first, mask, True, cuts=("one", "32"))
    x, m, h = ry.pooled(chain, None, 1, None, True)
    assert (m, h) == (140, 68)
    check_stage(kmc, chain, None, thresholds_of(rng, x, 3), 1, None, True, cuts=("one",))


def pattern_chain(rng, ns, nw):
    """[ns][nw][5]: normal draws, one value, two values, +-inf among normal draws, and a column with one NaN."""
    cols = [rng.standard_normal((ns, nw)), np.full((ns, nw), 2.5), rng.choice([-1.0, 3.0], size=(ns, nw)),
            np.where(rng.random((ns, nw)) < 0.2, rng.choice([-np.inf, np.inf], size=(ns, nw)), rng.standard_normal((ns, nw))),
            rng.standard_normal((ns, nw))]
    cols[4][ns // 3, nw // 2] = np.nan
    return np.stack(cols, axis=2)


def check_whole(got, want, label):
    assert list(got) == KEYS and (got["m"], got["h"]) == (want["m"], want["h"])
    finite = np.isfinite(want["margin"])
    assert np.all(want["margin"][finite] > 1e-4), f"{label}: an a S or b S within 1e-4 of an integer; take another seed"
    for k in ("quantile", "lower", "upper", "mcse"):
        assert same(got[k], want[k]), (label, k, got[k], want[k])
    np.testing.assert_array_equal(got["T"], want["T"])
    np.testing.assert_array_equal(got["flags"], want["flags"])
    print(f"{label}: ess {'equal to' if same(got['ess'], want['ess']) else 'within rtol 1e-12 of, not equal to,'} the yardstick's")
    np.testing.assert_allclose(got["ess"], want["ess"], rtol=1e-12, atol=0.0, equal_nan=True)


@pytest.mark.parametrize("split", [True, False])
def test_whole_call_on_value_patterns(kmc, split):
    """Normal draws, a constant column (ess NaN, no error), a two-valued column, a column with +-inf and a column with a NaN
    (KMC_CONV_HAS_NAN, the others unaffected), 12 walkers x 401 samples: everything against the yardstick."""
    rng = np.random.default_rng(21)
    chain = pattern_chain(rng, 401, 12)
    probs = [0.05, 0.16, 0.5, 0.84, 0.95]
    got = kmc.quantile_mcse(host(chain)[0], probs, split=split)
    want = qy.quantile_mcse(chain, probs, split=split)
    check_whole(got, want, f"patterns split={split}")
    assert np.isnan(got["ess"][:, 1]).all() and np.isnan(got["mcse"][:, 1]).all() and (got["flags"][:, 1] == 0).all() and (got["quantile"][:, 1] == 2.5).all()
    assert (got["flags"][:, 4] == qy.HAS_NAN).all() and all(np.isnan(got[k][:, 4]).all() for k in KEYS[:5]) and (got["T"][:, 4] == 0).all()
    assert np.isfinite(got["mcse"][:, 0]).all() and (got["mcse"][:, 0] > 0).all() and np.isfinite(got["ess"][:, 0]).all()
    assert np.isfinite(got["ess"][1:4, 3]).all() and np.isfinite(got["mcse"][2, 3])    # (a tenth of the column is -inf, a tenth +inf: q05 and q95 are infinite)
    assert np.isnan(got["ess"][[0, 4], 3]).all() and (got["flags"][:, 3] == 0).all()  # ... their indicators constant: ess NaN, no error
    assert np.isin(got["lower"][:, 0], chain[:, :, 0]).all() and np.isin(got["upper"][:, 0], chain[:, :, 0]).all()


def test_whole_call_sizes_probabilities_and_max_lag(kmc):
    """33 columns + the log-densities, 16 probabilities with a repeat, 70 walkers of which 23 are selected, first_sample > 0, an odd n,
    and a max_lag that truncates; then two identical calls: identical bits."""
    rng = np.random.default_rng(5)
    chain, logp = cy.ar1(rng, 0.5, 131, 70, 33), rng.standard_normal((131, 70))
    probs = list(np.linspace(0.03, 0.97, 15)) + [0.5]
    sel = np.arange(70) % 3 == 0
    th, lp = host(chain, logp)
    for max_lag in (None, 5):
        got = kmc.quantile_mcse(th, probs, lp, first_sample=6, walkers=sel, max_lag=max_lag)
        check_whole(got, qy.quantile_mcse(chain, probs, logp, 6, sel, True, max_lag), f"34 columns max_lag={max_lag}")
        assert got["quantile"].shape == (16, 34) and (got["m"], got["h"]) == (48, 62)
    assert ((got["flags"] & cy.TRUNCATED) != 0).any()
    again = kmc.quantile_mcse(th, probs, lp, first_sample=6, walkers=sel, max_lag=5)
    for k in KEYS:
        assert np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes(), k


def test_consistent_with_rank_convergence(kmc):
    """probs = [0.05, 0.5, 0.95]: quantile is rank_convergence's q05, median, q95 bit for bit; ess at 0.05 and 0.95 equals ess_q05 and
    ess_q95 within rtol 1e-10 (the same integers D_t; the older route's chain variances are two-pass sums of doubles)."""
    chain = cy.ar1(np.random.default_rng(9), 0.6, 301, 16, 3)
    th, _ = host(chain)
    got, rank = kmc.quantile_mcse(th, [0.05, 0.5, 0.95]), kmc.rank_convergence(th)
    for i, k in enumerate(("q05", "median", "q95")):
        assert same(got["quantile"][i], rank[k]), k
    np.testing.assert_allclose(got["ess"][0], rank["ess_q05"], rtol=1e-10, atol=0.0)
    np.testing.assert_allclose(got["ess"][2], rank["ess_q95"], rtol=1e-10, atol=0.0)
    np.testing.assert_array_equal(got["T"][[0, 2]], rank["lag"][[2, 3]])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sampler_route(kmc, dtype):
    """GaussianIso, 100 walkers x 3 dimensions (rows padded to 4 columns), 120 stored generations, in doubles and in floats: the chain
    where it lies gives the bits of the host-chain route on s.chain(), and the yardstick's; summary(quantile_mcse=True) adds one column
    and changes no other."""
    nw, nd, ns, nburn, seed = 100, 3, 120, 3, 5
    G = nburn + ns
    kw = {} if dtype == "f64" else dict(dtype="f32")
    probs = [0.05, 0.5, 0.95]
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, nburn, 1, 2.0, seed, store_chain=True, store_logp=True, **kw) as s:
        s.set_positions(np.random.default_rng(seed).standard_normal((nw, nd)))
        s.run(G)
        s.sync()
        chain, logp = s.chain()
        th, lp = host(chain, logp)
        sel = np.arange(nw) % 3 == 0
        for args in (dict(logp=True), dict(first_sample=11, walkers=sel, split=False)):
            got = s.quantile_mcse(probs, **args)
            hargs = {k: v for k, v in args.items() if k != "logp"}
            other = kmc.quantile_mcse(th, probs, lp if args.get("logp") else None, **hargs)
            for k in KEYS:
                assert np.asarray(other[k]).tobytes() == np.asarray(got[k]).tobytes(), k
            check_whole(got, qy.quantile_mcse(chain, probs, logp if args.get("logp") else None, args.get("first_sample", 0), args.get("walkers"),
                                              args.get("split", True)), f"sampler {dtype} {sorted(args)}")
        x, m, h = ry.pooled(chain, logp)
        thr = thresholds_of(np.random.default_rng(1), x, 2)
        a, b = s.indicator_lags(thr, 1, h - 1, logp=True), kmc.indicator_lags(th, thr, lp, 1, h - 1)
        assert a["ones"].tobytes() == b["ones"].tobytes() and a["lagcount"].tobytes() == b["lagcount"].tobytes()
        np.testing.assert_array_equal(a["lagcount"].astype(np.int64), qy.lag_counts(qy.indicators(x, thr), 1, h - 1))
        base, more = s.summary(), s.summary(quantile_mcse=True)
        assert list(base) == ["var", "median", "mean", "mode", "std"] and list(more) == list(base) + ["median_mcse"]
        for k in base:
            assert np.array_equal(np.asarray(base[k]), np.asarray(more[k])), k
        assert more["median_mcse"].tobytes() == np.ascontiguousarray(s.quantile_mcse([0.5])["mcse"][0]).tobytes()
        run = kmc.summarize_run(th, lp, quantile_mcse=True)
        assert list(run) == list(more) and run["median_mcse"].tobytes() == more["median_mcse"].tobytes()
        assert list(kmc.summarize_run(th, lp)) == list(base)


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_end_to_end(kmc, phi):
    """64 walkers x 500 samples of AR(1), one column: the mcse over the asymptotic standard error of the quantile of independent draws."""
    chain = cy.ar1(np.random.default_rng(2), phi, 500, 64, 1)
    probs = [0.05, 0.5, 0.95]
    got = kmc.quantile_mcse(host(chain)[0], probs)
    S = got["m"] * got["h"]
    ratio = np.array([got["mcse"][i, 0] / qy.asymptotic_mcse(p, S) for i, p in enumerate(probs)])
    print(f"phi = {phi}: mcse / asymptotic = {ratio}")
    if phi == 0.0:
        assert np.all((ratio >= 0.6) & (ratio <= 1.6))
    else:
        assert np.all(ratio >= 1.2)


def test_refusals(kmc):
    from kissmcmc_jl_amd import _lib
    G = kmc.GaussianIso()

    def status(f):
        with pytest.raises(kmc.KmcError) as err:
            f()
        return err.value.status

    with kmc.Sampler(G, 8, 2, 10, store_logp=True) as s:                            # no KMC_STORE_CHAIN
        assert status(lambda: s.quantile_mcse([0.5])) == _lib.ERR_BAD_ARG
        assert status(lambda: s.indicator_lags(np.zeros((1, 2)))) == _lib.ERR_BAD_ARG
    with kmc.Sampler(G, 8, 2, 30, 3, 1, 2.0, 1, store_chain=True) as s:
        s.set_positions(np.random.default_rng(0).standard_normal((8, 2)))
        s.run(30)
        s.sync()
        assert status(lambda: s.quantile_mcse([0.5], logp=True)) == _lib.ERR_BAD_ARG       # no KMC_STORE_LOGP
        assert status(lambda: s.quantile_mcse([0.5], first_sample=27)) == _lib.ERR_BAD_ARG  # the selection is empty
        assert status(lambda: s.quantile_mcse([0.5, 1.0])) == _lib.ERR_BAD_ARG
        assert status(lambda: s.quantile_mcse([])) == _lib.ERR_BAD_ARG
        assert status(lambda: s.quantile_mcse([0.5] * 17)) == _lib.ERR_BAD_ARG
        assert status(lambda: s.indicator_lags(np.zeros((1, 2)), 1, 13)) == _lib.ERR_BAD_ARG  # h = 13: lags up to 12
        assert s.quantile_mcse([0.5])["quantile"].shape == (1, 2)
    with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, stream_chain=True) as s:
        with pytest.raises(kmc.KmcError, match="kmc_chain_quantile_mcse") as err:
            s.quantile_mcse([0.5])
        assert err.value.status == _lib.ERR_UNSUPPORTED
        with pytest.raises(kmc.KmcError, match="kmc_chain_indicator_lags"):
            s.indicator_lags(np.zeros((1, 2)))
    for kw in (dict(shard_rank=0, shard_count=2), dict(p2p=True)):
        with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, **kw) as s:
            assert status(lambda: s.quantile_mcse([0.5])) == _lib.ERR_UNSUPPORTED
            assert status(lambda: s.indicator_lags(np.zeros((1, 2)))) == _lib.ERR_UNSUPPORTED
