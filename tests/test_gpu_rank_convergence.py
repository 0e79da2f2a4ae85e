"""GPU: rank-normalised R-hat with bulk and tail effective sample sizes, ranked on the device (kmc_*_rank_scores,
kmc_*_rank_convergence, Sampler.rank_scores / rank_convergence, kmc.rank_scores / rank_convergence and the rank=True forms of
convergence, summary and evaluate_convergence) against tests/rank_yardstick.py.

Ranks and quantiles are exact: rank2, median, q05 and q95 are compared for equality.

Scores.  Where |p - 0.5| <= 0.425 the score is +, -, *, / on the same inputs in the same order as the yardstick's: the same bits.
Elsewhere |z_dev - z_yard| <= 96 * 2^-53 |z_yard|: both sides form t = sqrt(-log(r)) from the same r; the two logarithms are within
1 ulp each of the true one, the two sqrt and the two subtractions move t - 1.6 (or t - 5) by at most 6 * 2^-53 t; |dz/dt| < 1.5 and
t <= 1.12 |z| on the tails; each side then commits 29 roundings in Horner sums whose coefficients and argument are all positive, so
nothing cancels: (10 + 58) 2^-53 |z|, asserted with 96 for slack.  A failure is a finding about the device's log or a contraction.

Statistics (the bounds of tests/test_gpu_convergence.py, restated).  The device's statistics are compared with the yardstick's computed
FROM THE DEVICE'S OWN z (as the tests of the plain diagnostics give the yardstick the device's chain means), so that only the sums
differ: each is a sum of N terms formed alike on both sides and added in an order the library chooses, |got - fsum| <= (N + 4) 2^-53
sum |t_k|.  With rel = 4 (h + m + 8) 2^-53: rhat within rel; T and the truncation flag equal, after asserting on the yardstick that
every pair sum rho_(k+1) + rho_(k+2) the rule tests lies more than 1e-9 from zero (rounding moves one by less than 1e-10); ess within
4 T (m h + 4) 2^-53 / (1 + 2 sum rho_t) + rel.  The lag sums of the indicator columns are sums of 0 / 1 terms and so exact in any
order; their ess differs from the yardstick's through the chain moments alone and keeps the same bound.

Sizes.  K = rank_plan()["tile_keys"] keys are one workgroup's tile of a sort pass; the pooled draws S = m h take the values 8, K - 1,
K, K + 1 and 3 K + 5 unsplit, with 2 walkers where S is even and else with the fewest walkers that divide S (no S = K - 1 or K + 1
draws are 2 chains of equal length)."""
import numpy as np
import pytest

import convergence_yardstick as cy
import rank_yardstick as ry

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TAIL = 96 * U
RANK_KEYS = ["rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "median", "q05", "q95", "lag", "truncated",
             "has_nan", "m", "h"]


def K(kmc):
    return kmc.rank_plan()["tile_keys"]


def host(chain, logp=None):
    """[sample][walker][dim] -> the thetas[walker][sample][dim], logdensities[walker][sample] of the module-level functions."""
    return chain.transpose(1, 0, 2), None if logp is None else logp.T


def walkers_for(S):
    return next(nw for nw in range(2, S) if S % nw == 0 and S // nw >= 4)


def patterns(rng, S):
    """[S][8]: the value patterns of the issue, one per column."""
    bits = rng.integers(0, 2 ** 64, size=S, dtype=np.uint64)
    raw = bits.view(np.float64).copy()
    raw[np.isnan(raw)] = 1.5                                                       # every digit of the key carries information; no NaN
    cols = [cy.ar1(rng, 0.9, S, 1, 1)[:, 0, 0],
            raw,
            1.0 + rng.integers(0, 256, size=S) * 2.0 ** -52,                       # keys that differ in the last byte only, with ties
            rng.choice([2.0 ** 1000, -2.0 ** 1000, 2.0 ** -1000, -2.0 ** -1000], size=S),       # ... in the top bytes only
            np.full(S, 2.5),                                                       # one value
            rng.choice([-1.0, 3.0], size=S),                                       # two values
            np.round(rng.standard_normal(S), 1),
            rng.choice([-0.0, 0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.0 ** -1040, 1.0], size=S)]
    return np.stack(cols, axis=1)


def check_scores(got_z, want_rank2, S):
    """Device z against the yardstick's z of the (exact) ranks: the same bits in the central branch, the derived bound on the tails."""
    want = ry.scores(want_rank2, S)
    mid = ry.central(ry.p_of(want_rank2, S))
    assert got_z.shape == want.shape and np.all(got_z[mid] == want[mid])
    if (~mid).any():
        err = np.abs(got_z[~mid] - want[~mid]) / np.abs(want[~mid])
        print(f"scores S={S}: {int((~mid).sum())} on the tails, largest error / bound {err.max() / TAIL:.3f}")
        assert np.all(err <= TAIL)


def check_ranks(got, t, folded=False):
    """One rank_scores dict against the yardstick's transforms."""
    assert (got["m"], got["h"], got["S"]) == (t["m"], t["h"], t["S"])
    np.testing.assert_array_equal(got["nan_count"], t["nan_count_folded" if folded else "nan_count"])
    want = t["rank2_folded" if folded else "rank2"]
    np.testing.assert_array_equal(got["rank2"], want)
    bad = got["nan_count"] > 0
    assert np.isnan(got["z"][bad]).all()
    if (~bad).any():
        check_scores(got["z"][~bad], want[~bad], t["S"])
    if folded:
        np.testing.assert_array_equal(got["centre"], t["median"])
    else:
        assert got["centre"] is None


def check_statistics(cols, z, z_folded, t, max_lag=None):
    """A rank_convergence dict against the yardstick's statistics of the device's own scores z, z_folded and the indicators."""
    m, h, ncols = t["m"], t["h"], t["z"].shape[0]
    st, r = ry.statistics_of(z, z_folded, t["i05"], t["i95"], max_lag)
    nlag = r["lagsum"].shape[1]
    for c in range(4 * ncols):                                                     # the truncation condition, on the yardstick
        upto = min(int(st["T"][c]) + 2, nlag)
        if upto >= 3 and st["W"][c] != 0.0:
            margins = cy.pair_margins(m, h, st["var_plus"][c:c + 1], r["lagsum"][c:c + 1], upto)
            assert margins.min() > 1e-9, f"transformed column {c}: a pair sum within 1e-9 of zero; take another seed"
    want = ry.combine(st, ncols, t["nan_count"], t["nan_count_folded"])
    assert (cols["m"], cols["h"]) == (m, h)
    np.testing.assert_array_equal(cols["lag"], want["T"])
    np.testing.assert_array_equal(cols["truncated"], (want["flags"] & cy.TRUNCATED) != 0)
    np.testing.assert_array_equal(cols["has_nan"], (want["flags"] & ry.HAS_NAN) != 0)
    for k in ("median", "q05", "q95"):
        np.testing.assert_array_equal(cols[k], t[k])
    rel = 4 * (h + m + 8) * U
    for k in ("rhat", "rhat_bulk", "rhat_folded"):
        np.testing.assert_allclose(cols[k], want[k], rtol=rel, atol=0, equal_nan=True)
    worst = 0.0
    for k, row in (("ess_bulk", 0), ("ess_q05", 2), ("ess_q95", 3)):
        w = want[k]
        ok = ~np.isnan(w)
        assert np.array_equal(np.isnan(cols[k]), ~ok)
        tol = 4 * want["T"][row][ok] * (m * h + 4) * U / (m * h / w[ok]) + rel
        err = np.abs(cols[k][ok] - w[ok]) / w[ok]
        worst = max(worst, float(np.max(err / tol))) if ok.any() else worst
        assert np.all(err <= tol), k
    print(f"statistics m={m} h={h}: T {want['T'].min()}..{want['T'].max()}, ess err/tol {worst:.3f}")
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(cols["ess_tail"], np.where(np.isnan(cols["ess_q05"]) | np.isnan(cols["ess_q95"]), np.nan,
                                                                 np.minimum(cols["ess_q05"], cols["ess_q95"])))
        np.testing.assert_array_equal(cols["rhat"], np.where(np.isnan(cols["rhat_bulk"]) | np.isnan(cols["rhat_folded"]), np.nan,
                                                             np.maximum(cols["rhat_bulk"], cols["rhat_folded"])))
    return want


# ---- ranks, exact ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["8", "K-1", "K", "K+1", "3K+5"])
def test_ranks_of_every_value_pattern(kmc, which):
    """Unsplit, S pooled draws, eight columns of value patterns: keys that differ in every digit, in the last byte only, in the top
    bytes only, one value, two values, heavy ties, and the two zeros with the infinities and subnormals."""
    k = K(kmc)
    S = {"8": 8, "K-1": k - 1, "K": k, "K+1": k + 1, "3K+5": 3 * k + 5}[which]
    nw = 2 if S % 2 == 0 else walkers_for(S)
    chain = patterns(np.random.default_rng(S), S).reshape(S // nw, nw, 8)
    th, _ = host(chain)
    t = ry.transforms(chain, split=False)
    assert t["S"] == S and t["m"] == nw
    got = kmc.rank_scores(th, split=False)
    check_ranks(got, t)
    again = kmc.rank_scores(th, split=False)
    assert again["rank2"].tobytes() == got["rank2"].tobytes() and again["z"].tobytes() == got["z"].tobytes()
    check_ranks(kmc.rank_scores(th, split=False, folded=True), t, folded=True)    # (inf - inf: the folded mixed column is all NaN or not, as the yardstick says)


@pytest.mark.parametrize("ncols,with_logp", [(1, False), (3, True), (33, False)], ids=["1", "3+logp", "33"])
def test_column_counts_split_with_an_odd_n(kmc, ncols, with_logp):
    """1, 3 and 33 columns and the log-densities as the last; split with an odd n, so that the middle sample is out of the pool;
    more than one tile of the transposing gather along both axes."""
    rng = np.random.default_rng(ncols)
    chain = cy.ar1(rng, 0.9, 151, 5, ncols)
    chain[75] = 1e6                                                                # the middle sample: ranked by nobody
    logp = -0.5 * np.sum(chain * chain, axis=2) if with_logp else None
    th, lp = host(chain, logp)
    t = ry.transforms(chain, logp, split=True)
    assert (t["m"], t["h"], t["S"]) == (10, 75, 750) and t["rank2"].shape[0] == ncols + (1 if with_logp else 0)
    check_ranks(kmc.rank_scores(th, lp), t)
    check_ranks(kmc.rank_scores(th, lp, folded=True), t, folded=True)


def test_walker_mask_first_sample_and_a_nan_column(kmc):
    """70 walkers, a mask of five scattered ones, first_sample = 7: what lies outside the selection is never ranked.  Then one NaN
    inside the selection: its column reports NaN and has_nan, its neighbours are unaffected."""
    rng = np.random.default_rng(4)
    chain = cy.ar1(rng, 0.9, 90, 70, 3)
    logp = -0.5 * np.sum(chain * chain, axis=2)
    chain[30, 5, 1] = np.nan                                                       # outside the mask
    chain[3, 17, 0] = np.nan                                                       # a selected walker, before first_sample
    mask = np.zeros(70, dtype=bool)
    mask[[3, 17, 40, 60, 69]] = True
    th, lp = host(chain, logp)
    t = ry.transforms(chain, logp, 7, mask)
    assert (t["m"], t["h"]) == (10, 41) and not t["nan_count"].any()
    for walkers in (mask, [69, 60, 3, 17, 40]):
        check_ranks(kmc.rank_scores(th, lp, first_sample=7, walkers=walkers), t)
    clean = kmc.rank_convergence(th, lp, first_sample=7, walkers=mask)
    assert list(clean) == RANK_KEYS and not clean["has_nan"].any() and np.isfinite(clean["rhat"]).all()
    chain[50, 40, 1] = np.nan
    th, lp = host(chain, logp)
    t = ry.transforms(chain, logp, 7, mask)
    assert t["nan_count"].tolist() == [0, 1, 0, 0]
    check_ranks(kmc.rank_scores(th, lp, first_sample=7, walkers=mask), t)
    check_ranks(kmc.rank_scores(th, lp, first_sample=7, walkers=mask, folded=True), t, folded=True)
    cols = kmc.rank_convergence(th, lp, first_sample=7, walkers=mask)
    assert cols["has_nan"].tolist() == [False, True, False, False] and (cols["lag"][:, 1] == 0).all()
    for k in RANK_KEYS[:10]:
        assert np.isnan(cols[k][1]), k
        assert cols[k][[0, 2, 3]].tobytes() == clean[k][[0, 2, 3]].tobytes(), k
    # inf - inf in the fold: more than half of the draws are +inf, so the median is (unsplit: S = 415 is odd and the median is a draw);
    # a NaN of the folded column only
    chain[50, 40, 1] = 0.25
    chain[rng.random((90, 70)) < 0.6, 2] = np.inf
    th, lp = host(chain, logp)
    t = ry.transforms(chain, logp, 7, mask, split=False)
    assert t["S"] == 415 and t["median"][2] == np.inf and not t["nan_count"].any() and 0 < t["nan_count_folded"][2] < t["S"]
    assert t["nan_count_folded"][[0, 1, 3]].tolist() == [0, 0, 0]
    check_ranks(kmc.rank_scores(th, lp, first_sample=7, walkers=mask, split=False, folded=True), t, folded=True)
    cols = kmc.rank_convergence(th, lp, first_sample=7, walkers=mask, split=False)
    assert cols["has_nan"].tolist() == [False, False, True, False] and np.isnan(cols["rhat_folded"][2]) and np.isnan(cols["rhat"][2])
    assert cols["median"][2] == np.inf and np.isfinite(cols["rhat_bulk"][2]) and cols["lag"][1, 2] == 0
    assert np.isfinite(cols["rhat"][[0, 1, 3]]).all() and np.isfinite(cols["ess_tail"][[0, 1, 3]]).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sampler_route(kmc, dtype):
    """GaussianIso, 100 walkers x 3 dimensions (rows padded to 4 columns), 120 stored generations, in doubles and in floats, whose
    widened values tie: the ranks of the chain where it lies against the yardstick on the fetched chain."""
    nw, nd, ns, nburn, seed = 100, 3, 120, 3, 5
    G = nburn + ns
    kw = {} if dtype == "f64" else dict(dtype="f32")
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, nburn, 1, 2.0, seed, store_chain=True, store_logp=True, **kw) as s:
        s.set_positions(np.random.default_rng(seed).standard_normal((nw, nd)))
        s.run(G)
        s.sync()
        chain, logp = s.chain()
        t = ry.transforms(chain, logp)
        assert (t["m"], t["h"]) == (200, 60)
        got, gotf = s.rank_scores(logp=True), s.rank_scores(logp=True, folded=True)
        check_ranks(got, t)
        check_ranks(gotf, t, folded=True)
        sel = np.arange(nw) % 3 == 0
        check_ranks(s.rank_scores(first_sample=11, walkers=sel, split=False), ry.transforms(chain, None, 11, sel, False))
        cols = s.rank_convergence(logp=True)
        assert list(cols) == RANK_KEYS
        check_statistics(cols, got["z"], gotf["z"], t)
        # the host-chain route over the fetched chain: the same kernels on an unpadded double copy, the same bits
        th, lp = host(chain, logp)
        other = kmc.rank_convergence(th, lp)
        for k in RANK_KEYS[:12]:
            assert np.asarray(other[k]).tobytes() == np.asarray(cols[k]).tobytes(), k
        # opt-in on the existing calls; their defaults and outputs do not change
        plain, ranked = s.convergence(), s.convergence(rank=True)
        assert list(plain) == ["mean", "std", "rhat", "ess", "mcse", "lag", "truncated", "m", "h"]
        assert list(ranked) == list(plain) + ["rhat_rank", "ess_bulk", "ess_tail"]
        for k in plain:
            assert np.asarray(plain[k]).tobytes() == np.asarray(ranked[k]).tobytes(), k
        own = s.rank_convergence()                                                 # (without the log-densities the scratch rows are shorter and the sums
        for k, src in (("rhat_rank", "rhat"), ("ess_bulk", "ess_bulk"), ("ess_tail", "ess_tail")):      # are added in another order: equal to rounding)
            assert ranked[k].tobytes() == own[src].tobytes(), k
            np.testing.assert_allclose(own[src], cols[src][:nd], rtol=1e-9)
        base, conv, more = s.summary(), s.summary(convergence=True), s.summary(convergence="rank")
        assert list(base) == ["var", "median", "mean", "mode", "std"] and list(conv) == list(base) + ["rhat", "ess", "mcse"]
        assert list(more) == list(conv) + ["rhat_rank", "ess_bulk", "ess_tail"]
        for k in conv:
            assert np.array_equal(np.asarray(conv[k]), np.asarray(more[k])), k
        for k in ("rhat_rank", "ess_bulk", "ess_tail"):
            assert more[k].tobytes() == ranked[k].tobytes(), k
        assert list(kmc.convergence(th)) == list(plain) and list(kmc.summarize_run(th, lp, convergence=True)) == list(conv)
        assert list(kmc.summarize_run(th, lp, convergence="rank")) == list(more)


# ---- end to end --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ar1_chain():
    """AR(1), phi = 0.9, 16 walkers x 2 columns x 801 samples; and the same with one chain's scale tripled."""
    chain = cy.ar1(np.random.default_rng(11), 0.9, 801, 16, 2)
    wide = chain.copy()
    wide[:, 5, :] *= 3.0
    return chain, wide


@pytest.mark.parametrize("tripled", [False, True], ids=["ar1", "one-chain-tripled"])
def test_end_to_end(kmc, ar1_chain, tripled):
    chain = ar1_chain[1 if tripled else 0]
    th, _ = host(chain)
    t = ry.transforms(chain)
    assert (t["m"], t["h"], t["S"]) == (32, 400, 12800)
    got, gotf = kmc.rank_scores(th), kmc.rank_scores(th, folded=True)
    check_ranks(got, t)
    check_ranks(gotf, t, folded=True)
    cols = kmc.rank_convergence(th)
    assert list(cols) == RANK_KEYS
    want = check_statistics(cols, got["z"], gotf["z"], t)
    assert not cols["has_nan"].any() and np.all(cols["ess_tail"] > 0) and np.all(cols["ess_bulk"] > 0)
    # two identical calls: the same bits in every output
    again = kmc.rank_convergence(th)
    for k in RANK_KEYS:
        assert np.asarray(again[k]).tobytes() == np.asarray(cols[k]).tobytes(), k
    for a, b in ((kmc.rank_scores(th), got), (kmc.rank_scores(th, folded=True), gotf)):
        for k in ("rank2", "z", "nan_count"):
            assert a[k].tobytes() == b[k].tobytes(), k
    plain = kmc.convergence(th)
    ranked = kmc.convergence(th, rank=True)
    assert list(ranked) == list(plain) + ["rhat_rank", "ess_bulk", "ess_tail"] and ranked["rhat_rank"].tobytes() == cols["rhat"].tobytes()
    for k in plain:
        assert np.asarray(plain[k]).tobytes() == np.asarray(ranked[k]).tobytes(), k
    Rs, size, nthin = kmc.evaluate_convergence(th[:8], th[8:], rank=True)
    assert Rs.tobytes() == cols["rhat"].tobytes() and size.tobytes() == cols["ess_bulk"].tobytes()
    assert nthin == int(round(801 * 16 / np.mean(cols["ess_bulk"])))
    Rs0, size0, _ = kmc.evaluate_convergence(th[:8], th[8:])
    assert Rs0.tobytes() == plain["rhat"].tobytes() and size0.tobytes() == plain["ess"].tobytes()
    if tripled:                                                                    # the case the feature exists for
        assert np.all(cols["rhat_folded"] > cols["rhat_bulk"]) and np.all(cols["rhat"] > plain["rhat"])
        assert np.all(want["rhat_folded"] > 1.05) and np.all(want["rhat_bulk"] < 1.05)
    else:
        assert np.all(cols["rhat"] < 1.05)


def test_refusals(kmc):
    from kissmcmc_jl_amd import _lib

    def status(fn):
        with pytest.raises(kmc.KmcError) as e:
            fn()
        return e.value.status

    G = kmc.GaussianIso()
    with kmc.Sampler(G, 8, 2, 10, store_logp=True) as s:                            # no KMC_STORE_CHAIN
        assert status(lambda: s.rank_convergence()) == _lib.ERR_BAD_ARG
        assert status(lambda: s.rank_scores()) == _lib.ERR_BAD_ARG
    with kmc.Sampler(G, 8, 2, 30, 3, 1, 2.0, 1, store_chain=True) as s:
        s.set_positions(np.random.default_rng(0).standard_normal((8, 2)))
        s.run(30)
        s.sync()
        assert status(lambda: s.rank_convergence(logp=True)) == _lib.ERR_BAD_ARG    # no KMC_STORE_LOGP
        assert status(lambda: s.rank_scores(logp=True)) == _lib.ERR_BAD_ARG
        assert status(lambda: s.summary(convergence="rank") and s.convergence(logp=True, rank=True)) == _lib.ERR_BAD_ARG
        assert s.rank_convergence()["h"] == 13 and s.rank_scores()["rank2"].shape == (2, 16, 13)
        assert status(lambda: s.rank_convergence(max_lag=13)) == _lib.ERR_BAD_ARG   # max_lag >= h
        assert status(lambda: s.rank_convergence(first_sample=21)) == _lib.ERR_BAD_ARG      # h = 3
        assert status(lambda: s.rank_scores(walkers=[2], split=False)) == _lib.ERR_BAD_ARG  # one chain
    with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, stream_chain=True) as s:
        with pytest.raises(kmc.KmcError, match="kmc_chain_rank_convergence") as err:
            s.rank_convergence()
        assert err.value.status == _lib.ERR_UNSUPPORTED
        assert status(lambda: s.rank_scores()) == _lib.ERR_UNSUPPORTED
    for kw in (dict(shard_rank=0, shard_count=2), dict(p2p=True)):
        with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, **kw) as s:
            assert status(lambda: s.rank_convergence()) == _lib.ERR_UNSUPPORTED
