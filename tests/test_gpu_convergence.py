"""GPU: convergence across chains on the device -- chain means, chain variances and the lag sums of the variogram
(kmc_sampler_lag_sums, kmc_chain_lag_sums) against their exact restatement (tests/convergence_yardstick.py: raw), and split-R-hat,
effective sample size and Monte-Carlo standard error end to end (kmc_*_convergence, Sampler.convergence, kmc.convergence) against
raw + stats.

Tolerances (derived, not measured).  Every number the device stage returns is a sum S of N terms t_k, each formed in double exactly as
the yardstick forms it (one subtraction, one multiplication), added in an order the library is free to choose.  Adding N doubles in ANY
order commits at most N - 1 roundings, each relative to a partial sum that is at most sum |t_k| in magnitude, so
|computed - exact| <= gamma_(N-1) sum |t_k| with gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 4.2); for the N < 2^22 of these tests gamma_(N-1) < N u.  The yardstick's math.fsum is the exact sum
rounded once (u |S| <= u sum |t_k|), and where a division follows the sum (the mean by h, the variance by h - 1) each side rounds
once more: three further units at most.  Hence the bound asserted everywhere:

    |got - fsum| <= (N + 4) 2^-53 sum |t_k|

For D_t and the centred squares the terms are not negative, sum |t_k| is the sum itself and the bound is relative, with N = m (h - t)
and N = h.  The centred squares are taken about the DEVICE's chain means (its second pass centres on what its first pass found), so the
yardstick is given those.  For the means the bound is against sum |x|, N = h.

Truncation.  T, ess and mcse are compared end to end only after asserting, on the yardstick, that every pair sum rho_(k+1) + rho_(k+2)
the rule tests on its way lies more than 1e-9 from zero -- rounding in D_t moves a pair sum by at most 2 (N + 4) 2^-53 < 1e-10 -- so that
both sides stop at the same T; ess then differs by at most the 2 T rounded rho_t in its denominator:
|d ess| / ess <= 4 T (N + 4) 2^-53 / (1 + 2 sum rho_t), with the factor 2 of slack for var+ (ESS_TOL below)."""
import numpy as np
import pytest

import convergence_yardstick as cy

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def run_sampler(kmc, nw, nd, ns, nburn=3, nthin=1, seed=5, **kw):
    """A Gaussian sampler with ns stored samples; returns it after the run (the caller closes it)."""
    G = nburn + ns * nthin
    th = np.random.default_rng(seed).standard_normal((nw, nd))
    s = kmc.Sampler(kmc.GaussianIso(), nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, **kw)
    s.set_positions(th)
    s.run(G)
    s.sync()
    return s


def host(chain, logp=None):
    """[sample][walker][dim] -> the thetas[walker][sample][dim], logdensities[walker][sample] of the module-level functions."""
    return chain.transpose(1, 0, 2), None if logp is None else logp.T


def check_moments(got, chain, logp=None, first=0, walkers=None, split=True):
    want = cy.raw(chain, logp, first, walkers, split, means=got["chain_mean"])
    m, h = want["m"], want["h"]
    assert (got["m"], got["h"]) == (m, h) and got["chain_mean"].shape == want["chain_mean"].shape == got["chain_var"].shape
    em = np.abs(got["chain_mean"] - want["chain_mean"]) * h
    ev = np.abs(got["chain_var"] - want["chain_var"]) * (h - 1)
    bm, bv = (h + 4) * U * want["abs_sum"], (h + 4) * U * want["sq_sum"]
    print(f"moments m={m} h={h}: mean err/bound {np.max(em / bm):.3f}, var err/bound {np.max(ev / np.maximum(bv, 1e-300)):.3f}")
    assert np.all(em <= bm) and np.all(ev <= bv)
    return want


def check_lags(got_lagsum, want_lagsum, m, h, lag0):
    got_lagsum, want_lagsum = np.asarray(got_lagsum), np.asarray(want_lagsum)
    assert got_lagsum.shape == want_lagsum.shape
    t = lag0 + np.arange(want_lagsum.shape[1])
    bound = (m * (h - t) + 4) * U * want_lagsum
    err = np.abs(got_lagsum - want_lagsum)
    print(f"lags {lag0}..{t[-1]} m={m} h={h}: err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


def check_device_stage(got, chain, logp=None, first=0, walkers=None, split=True):
    """The three arrays of one lag_sums call against the yardstick; returns the yardstick's raw dict."""
    check_moments(got, chain, logp, first, walkers, split)
    want = cy.raw(chain, logp, first, walkers, split, got["lag0"], got["lagsum"].shape[1])
    check_lags(got["lagsum"], want["lagsum"], want["m"], want["h"], got["lag0"])
    return want


def check_end_to_end(cols, chain, logp=None, first=0, walkers=None, split=True, max_lag=None, r=None):
    """A convergence dict (mean, std, rhat, ess, mcse, lag, truncated, m, h) against raw + stats of the yardstick (r: its raw arrays
    with the lags 1 .. max_lag, where a test has them already)."""
    if r is None:
        want, r = cy.convergence(chain, logp, first, walkers, split, max_lag)
    else:
        want = cy.stats(r["m"], r["h"], r["chain_mean"], r["chain_var"], r["lagsum"], max_lag)
    m, h = r["m"], r["h"]
    max_lag = r["lagsum"].shape[1]
    assert (cols["m"], cols["h"]) == (m, h)
    T = want["T"]
    for c in range(T.size):                                                        # the truncation condition, on the yardstick
        upto = min(int(T[c]) + 2, max_lag)
        if upto >= 3:
            margins = cy.pair_margins(m, h, want["var_plus"][c:c + 1], r["lagsum"][c:c + 1], upto)
            assert margins.min() > 1e-9, f"column {c}: a pair sum within 1e-9 of zero; take another seed"
    np.testing.assert_array_equal(cols["lag"], T)
    np.testing.assert_array_equal(cols["truncated"], (want["flags"] & cy.TRUNCATED) != 0)
    rel = 4 * (h + m + 8) * U
    mean_abs = r["abs_sum"].sum(axis=1) / (m * h)
    assert np.all(np.abs(cols["mean"] - want["mean"]) <= (h + m + 8) * U * mean_abs)
    np.testing.assert_allclose(cols["std"], np.sqrt(want["var_plus"]), rtol=rel, atol=0)
    np.testing.assert_allclose(cols["rhat"], want["rhat"], rtol=rel, atol=0)
    den = m * h / want["ess"]
    ESS_TOL = 4 * T * (m * h + 4) * U / den + rel
    err = np.abs(cols["ess"] - want["ess"]) / want["ess"]
    print(f"end to end m={m} h={h}: T {T.min()}..{T.max()}, ess err/tol {np.max(err / ESS_TOL):.3f}")
    assert np.all(err <= ESS_TOL)
    assert np.all(np.abs(cols["mcse"] - want["mcse"]) <= (ESS_TOL + rel) * want["mcse"])
    return want


def plan():
    from kissmcmc_jl_amd import chain_convergence
    return chain_convergence.lag_plan()


# ---- the host-chain route ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    """100 walkers x 3 dimensions x 2 001 samples of AR(1), phi = 0.9, with 'log-densities': (chain, logp, the yardstick's raw arrays for
    the lags 1 .. 200).  Computed once (2 to 3 s) and shared."""
    rng = np.random.default_rng(7)
    chain = cy.ar1(rng, 0.9, 2001, 100, 3)
    logp = -0.5 * np.sum(chain * chain, axis=2)
    return chain, logp, cy.raw(chain, logp, lag0=1, nlags=200)


def test_every_lag_of_a_short_odd_chain(kmc):
    """5 walkers x 3 dimensions x 41 samples: n odd (the middle sample belongs to neither half), h = 20, every lag 1 .. 19 -- one
    sample tile, all of it on the masked path."""
    chain = cy.ar1(np.random.default_rng(1), 0.9, 41, 5, 3)
    th, _ = host(chain)
    got = kmc.lag_sums(th, nlags=19)
    assert (got["m"], got["h"]) == (10, 20)
    check_device_stage(got, chain)
    check_device_stage(kmc.lag_sums(th, nlags=40, split=False), chain, split=False)
    check_end_to_end(kmc.convergence(th), chain)


def test_lag_blocks_and_sample_tiles(kmc, big):
    """100 x 3 x 2 001 with log-densities, lags 1 .. 200: several lag blocks, the last not full, and 32 sample tiles a half, cut into
    chunks -- whatever block and tile sizes the kernel has."""
    chain, logp, want = big
    p = plan()
    assert 200 > p["lag_block"] and 200 % p["lag_block"] != 0 and want["h"] > 2 * p["tile_samples"]
    th, lp = host(chain, logp)
    got = kmc.lag_sums(th, lp, nlags=200)
    assert got["lagsum"].shape == (4, 200) and (got["m"], got["h"]) == (200, 1000)
    check_moments(got, chain, logp)
    check_lags(got["lagsum"], want["lagsum"], 200, 1000, 1)
    # the same lags from a call that starts elsewhere: against the yardstick, and the same bits as before
    part = kmc.lag_sums(th, lp, lag0=65, nlags=70, moments=False)
    assert part["chain_mean"] is None and part["lagsum"].shape == (4, 70)
    check_lags(part["lagsum"], want["lagsum"][:, 64:134], 200, 1000, 65)
    assert part["lagsum"].tobytes() == got["lagsum"][:, 64:134].tobytes()
    # two identical calls: identical bits
    again = kmc.lag_sums(th, lp, nlags=200)
    for k in ("chain_mean", "chain_var", "lagsum"):
        assert again[k].tobytes() == got[k].tobytes(), k
    # end to end, log-densities included; the rule stops well inside max_lag = 256 for phi = 0.9
    cols = kmc.convergence(th, lp, max_lag=200)
    w = check_end_to_end(cols, chain, logp, max_lag=200, r=want)
    assert not cols["truncated"].any() and cols["lag"].max() > p["lag_block"] and np.all(w["rhat"] < 1.05)
    assert kmc.convergence(th, lp, max_lag=200)["ess"].tobytes() == cols["ess"].tobytes()
    mean, mcse, std = kmc.error_of_estimated_mean(th)
    full = kmc.convergence(th)
    assert mean.tobytes() == full["mean"].tobytes() and mcse.tobytes() == full["mcse"].tobytes() and std.tobytes() == full["std"].tobytes()


@pytest.mark.parametrize("nw,nd,ns", [(6, 200, 64), (1030, 1, 64), (3, 70, 64), (40, 5, 64)],
                         ids=["6x200x64", "1030x1x64", "3x70x64", "40x5x64"])
def test_row_shapes(kmc, nw, nd, ns):
    """A row longer than a workgroup's 64 lanes (every lane a column of its own; 200 and 70 are no multiples of 64, so the columns
    shift from tile to tile); ndim = 1 with a walker count that is no multiple of 64; a row length that does not divide 64."""
    chain = cy.ar1(np.random.default_rng(nw), 0.9, ns, nw, nd)
    th, _ = host(chain)
    check_device_stage(kmc.lag_sums(th, nlags=31), chain)
    check_device_stage(kmc.lag_sums(th, nlags=63, split=False), chain, split=False)
    check_end_to_end(kmc.convergence(th), chain)


def test_a_step_between_the_halves(kmc):
    """Every walker jumps by 1 000 between its halves.  Split, no pair straddles the step and D_t stays of order m h; a kernel that
    paired across the halves would be wrong by six orders of magnitude.  Unsplit, the step is inside every chain and belongs in D_t."""
    chain = cy.ar1(np.random.default_rng(2), 0.9, 200, 8, 2)
    chain[100:] += 1000.0
    th, _ = host(chain)
    got = kmc.lag_sums(th, nlags=99)
    want = check_device_stage(got, chain)
    assert want["lagsum"].max() < 16 * 100 * 8.0
    got1 = kmc.lag_sums(th, nlags=199, split=False)
    want1 = check_device_stage(got1, chain, split=False)
    assert want1["lagsum"].min() > 1e6
    cols, cols1 = kmc.convergence(th), kmc.convergence(th, split=False)
    assert np.all(cols["rhat"] > 100) and np.all(cols1["rhat"] < 1.01)
    # an odd number of samples and a first_sample: the halves are [5, 102) and [103, 200), and the step is at 103
    chain = cy.ar1(np.random.default_rng(3), 0.9, 200, 8, 2)
    chain[103:] += 1000.0
    th, _ = host(chain)
    want = check_device_stage(kmc.lag_sums(th, nlags=96, first_sample=5), chain, first=5)
    assert want["h"] == 97 and want["lagsum"].max() < 16 * 100 * 8.0


def test_walker_mask_and_first_sample(kmc):
    """64 walkers, a mask of three scattered ones, first_sample = 7; a NaN and a huge value in walkers outside the mask and in samples
    before first_sample must not be read into any sum."""
    chain = cy.ar1(np.random.default_rng(4), 0.9, 71, 64, 2)
    logp = -0.5 * np.sum(chain * chain, axis=2)
    chain[30, 5, 1] = np.nan
    chain[40, 62, 0] = 1e200
    chain[3, 17, 0] = np.nan                                                       # a selected walker, before first_sample
    logp[3, 17] = np.inf
    mask = np.zeros(64, dtype=bool)
    mask[[3, 17, 60]] = True
    th, lp = host(chain, logp)
    for walkers in (mask, [60, 3, 17]):
        got = kmc.lag_sums(th, lp, nlags=31, first_sample=7, walkers=walkers)
        assert (got["m"], got["h"]) == (6, 32) and np.isfinite(got["lagsum"]).all() and np.isfinite(got["chain_var"]).all()
        check_device_stage(got, chain, logp, first=7, walkers=mask)
    check_end_to_end(kmc.convergence(th, lp, first_sample=7, walkers=mask), chain, logp, first=7, walkers=mask)
    # inside the selection a NaN propagates: its column, every lag (sample 7 is the first of a half), and nothing else
    chain[7, 17, 1] = np.nan
    got = kmc.lag_sums(host(chain)[0], nlags=31, first_sample=7, walkers=mask)
    assert np.isnan(got["lagsum"][1]).all() and np.isfinite(got["lagsum"][0]).all()
    assert np.isnan(got["chain_mean"][1]).sum() == 1 and np.isfinite(got["chain_mean"][0]).all()
    cols = kmc.convergence(host(chain)[0], first_sample=7, walkers=mask)
    assert np.isnan(cols["rhat"][1]) and np.isnan(cols["ess"][1]) and np.isfinite(cols["rhat"][0]) and np.isfinite(cols["ess"][0])
    # a constant column: NaN without an error
    chain[:, :, 1] = 2.5
    cols = kmc.convergence(host(chain)[0], first_sample=7, walkers=mask)
    assert cols["mean"][1] == 2.5 and cols["std"][1] == 0.0 and np.isnan(cols["rhat"][1]) and np.isnan(cols["ess"][1]) and cols["lag"][1] == 0


# ---- the sampler route -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{}, dict(dtype="f32"), dict(nburn=7, nthin=3), dict(betas=[1.0, 0.5, 0.25])],
                         ids=["f64", "f32", "thinned", "ladder-rung0"])
def test_sampler_chain(kmc, kw):
    """GaussianIso, 100 walkers x 3 dimensions, 400 stored generations: the device stage and the whole thing on the chain where it lies
    (rows padded to 4 columns; floats with dtype="f32"), against the yardstick on the fetched chain."""
    with run_sampler(kmc, 100, 3, 400, **kw) as s:
        assert s.samples_done == 400
        chain, logp = s.chain()
        got = s.lag_sums(nlags=199, logp=True)
        assert (got["m"], got["h"]) == (200, 200) and got["lagsum"].shape == (4, 199)
        check_device_stage(got, chain, logp)
        check_device_stage(s.lag_sums(nlags=40, split=False, first_sample=11, walkers=np.arange(100) % 3 == 0), chain, None, 11,
                           np.arange(100) % 3 == 0, False)
        # the whole thing is the host stage applied to the device's own arrays, bit for bit
        cols = s.convergence(logp=True)
        st = kmc.convergence_stats(got["m"], got["h"], got["chain_mean"], got["chain_var"], got["lagsum"], 199)
        assert list(cols) == ["mean", "std", "rhat", "ess", "mcse", "lag", "truncated", "m", "h"]
        for k, w in (("mean", st["mean"]), ("std", np.sqrt(st["var_plus"])), ("rhat", st["rhat"]), ("ess", st["ess"]), ("mcse", st["mcse"])):
            assert cols[k].tobytes() == w.tobytes(), k
        np.testing.assert_array_equal(cols["lag"], st["T"])
        np.testing.assert_array_equal(cols["truncated"], (st["flags"] & cy.TRUNCATED) != 0)
        assert not (st["flags"] & cy.NEED_LAGS).any()
        check_end_to_end(cols, chain, logp)
        # the host-chain route over the fetched chain: the same kernels on an unpadded double copy
        th, lp = host(chain, logp)
        check_end_to_end(kmc.convergence(th, lp), chain, logp)
        # the summary table: three more columns with convergence=True, and nothing else changes
        base, more = s.summary(), s.summary(convergence=True)
        assert list(base) == ["var", "median", "mean", "mode", "std"] and list(more) == list(base) + ["rhat", "ess", "mcse"]
        for k in base:
            assert np.array_equal(np.asarray(base[k]), np.asarray(more[k])), k
        plain = s.convergence()
        for k in ("rhat", "ess", "mcse"):
            assert more[k].tobytes() == plain[k].tobytes() == cols[k][:3].tobytes(), k
        run = kmc.summarize_run(th, lp, convergence=True)
        assert list(run) == list(more) and list(kmc.summarize_run(th, lp)) == list(base)
        for k in ("rhat", "ess", "mcse"):
            np.testing.assert_allclose(run[k], more[k], rtol=1e-7)


def test_evaluate_convergence_and_samples_vs_tau(kmc):
    chains = []
    for seed in (5, 6):
        with run_sampler(kmc, 100, 4, 400, seed=seed) as s:
            chains.append(s.chain(logp=False)[0])
            if seed == 5:
                N, taus = kmc.samples_vs_tau(host(chains[0])[0])
                assert N.tolist() == np.round(np.logspace(2, np.log10(400), 10)).astype(int).tolist() and taus.shape == (10, 4)
                for n, tau in zip(N, taus):
                    np.testing.assert_allclose(tau, kmc.int_acorr(host(chains[0])[0][:, :n], warn=False)[0], rtol=1e-12)
    th1, th2 = host(chains[0])[0], host(chains[1])[0]
    both = np.concatenate([th1, th2], axis=0)
    Rs, size, nthin = kmc.evaluate_convergence(th1, th2)
    want = kmc.convergence(both)
    assert Rs.tobytes() == want["rhat"].tobytes() and size.tobytes() == want["ess"].tobytes() and want["m"] == 400
    assert nthin == int(round(400 * 200 / np.mean(want["ess"]))) and nthin >= 1
    check_end_to_end(want, np.concatenate(chains, axis=1))
    # the reference's choice: one walker of each run; two chains, split in four
    Rs, size, nthin = kmc.evaluate_convergence(th1, th2, indices=[2, 0], walkernr=7)
    want = kmc.convergence(np.stack([th1[7], th2[7]]))
    assert want["m"] == 4 and Rs.tobytes() == want["rhat"][[2, 0]].tobytes() and size.tobytes() == want["ess"][[2, 0]].tobytes()
    assert nthin == int(round(400 * 2 / np.mean(want["ess"][[2, 0]])))


def test_refusals(kmc):
    from kissmcmc_jl_amd import _lib

    def status(fn):
        with pytest.raises(kmc.KmcError) as e:
            fn()
        return e.value.status

    G = kmc.GaussianIso()
    with kmc.Sampler(G, 8, 2, 10, store_logp=True) as s:                            # no KMC_STORE_CHAIN
        assert status(lambda: s.convergence()) == _lib.ERR_BAD_ARG
        assert status(lambda: s.lag_sums(nlags=1)) == _lib.ERR_BAD_ARG
    with run_sampler(kmc, 8, 2, 20, seed=1) as s0, kmc.Sampler(G, 8, 2, 30, 3, 1, 2.0, 1, store_chain=True) as s:
        s.set_positions(np.random.default_rng(0).standard_normal((8, 2)))
        s.run(30)
        s.sync()
        assert status(lambda: s.convergence(logp=True)) == _lib.ERR_BAD_ARG         # no KMC_STORE_LOGP
        assert status(lambda: s.summary(convergence=True) and s.lag_sums(nlags=1, logp=True)) == _lib.ERR_BAD_ARG
        assert s.convergence()["h"] == 13
        assert s0.convergence()["h"] == 10 and s0.convergence(max_lag=9)["m"] == 16
        assert status(lambda: s0.convergence(max_lag=10)) == _lib.ERR_BAD_ARG       # max_lag >= h
        assert status(lambda: s0.convergence(max_lag=2)) == _lib.ERR_BAD_ARG
        assert status(lambda: s0.convergence(walkers=np.zeros(8, dtype=bool))) == _lib.ERR_BAD_ARG     # an empty mask
        assert status(lambda: s0.convergence(first_sample=13)) == _lib.ERR_BAD_ARG  # h = 3
        assert status(lambda: s0.convergence(walkers=[2], split=False)) == _lib.ERR_BAD_ARG            # one chain
        assert status(lambda: s0.lag_sums(lag0=10, nlags=1)) == _lib.ERR_BAD_ARG
        assert s0.lag_sums(lag0=9, nlags=1)["lagsum"].shape == (2, 1) and s0.convergence(walkers=[2])["m"] == 2
    with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, stream_chain=True) as s:
        with pytest.raises(kmc.KmcError, match="kmc_chain_convergence") as err:
            s.convergence()
        assert err.value.status == _lib.ERR_UNSUPPORTED
        assert status(lambda: s.lag_sums(nlags=1)) == _lib.ERR_UNSUPPORTED
    for kw in (dict(shard_rank=0, shard_count=2), dict(p2p=True)):
        with kmc.Sampler(G, 8, 2, 10, store_chain=True, store_logp=True, **kw) as s:
            assert status(lambda: s.convergence()) == _lib.ERR_UNSUPPORTED
