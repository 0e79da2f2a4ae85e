"""GPU: likelihood tempering of a data density (kmc.Sampler(DataDensity, betas=..., temper="likelihood") /
kmc_config.temper_mode = KMC_TEMPER_LIKELIHOOD) against its numpy yardstick (tests/data_tempering_yardstick.py), bit for bit on every
rung; rung 0 against the plain DataDensity sampler; checkpoints and set_positions; the launch count; the evidence of a conjugate
model against its closed forms; the two separated modes; refusals.  Ensembles of at most 256 walkers, so that the sweep kernel's sums
(one workgroup per rung) have a fixed order and `loglike_sum` can be held to the yardstick exactly."""
import warnings

import numpy as np
import pytest

import data_tempering_yardstick as dy
import snooker_yardstick as sy
from test_data_density_cpu import REG_TERM
from test_gpu_data_density import reg_data, reg_terms
from test_gpu_tempering import MODES, MODES_BOUND, two_mode_start

pytestmark = pytest.mark.gpu

GAUSS_PRIOR = "double s = 0.0; for (int k = 0; k < n; ++k) s += x[k] * x[k]; return -0.5 * s;"
BOX_PRIOR = "for (int k = 0; k < n; ++k) if (x[k] < -p[1] || x[k] > p[1]) return -INFINITY; return 0.25 * x[0];"


def gauss_prior(X):
    s = np.zeros(X.shape[0])
    for k in range(X.shape[1]):
        s = s + X[:, k] * X[:, k]
    return -0.5 * s


def box_prior(X, half_width):
    inside = np.all((X >= -half_width) & (X <= half_width), axis=1)
    return np.where(inside, 0.25 * X[:, 0], -np.inf)


def moves(kmc, name):
    return {"stretch": (None, None), "de": (kmc.DEMove(), sy.DE()), "snooker": (kmc.DESnookerMove(), sy.Snooker()),
            "mix": ([(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)], [(sy.DE(), 0.8), (sy.Snooker(), 0.2)])}[name]


def run(kmc, pdf, th, betas, G, nburn=0, nthin=1, seed=11, move=None, swap_every=1, pieces=2, **kw):
    nw, nd = th.shape[-2:]
    with kmc.Sampler(pdf, nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, move=move, betas=betas,
                     swap_every=swap_every, temper="likelihood", **kw) as s:
        s.set_positions(th)
        done = 0
        for i in range(pieces):
            n = G // pieces if i + 1 < pieces else G - done
            s.run(n)
            done += n
        s.sync()
        ch, cl = s.chain()
        return dict(pos=s.rung_positions(), logp=s.rung_logp(), loglike=s.rung_loglike(), logprior=s.rung_logprior(), nacc=s.rung_naccept(),
                    nswap=s.nswap().astype(np.int64), loglike_sum=s.rung_loglike_sum(), logp_sum=s.rung_logp_sum(), chain=ch, chain_logp=cl,
                    pos0=s.positions(), logp0=s.logp(), nacc0=s.naccept(), desc=s.describe(), launches=s.launch_count)


def assert_matches(got, want):
    """Bit for bit: the regression term and the priors compiled with contraction off are exact against numpy."""
    for k in ("nacc", "nswap", "pos", "logp", "loglike", "logprior", "chain", "chain_logp", "loglike_sum"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_allclose(got["logp_sum"], want["logp_sum"], rtol=1e-11)       # (its order is tempering_yardstick's plain sum)
    np.testing.assert_array_equal(got["pos0"], got["pos"][0])                       # the plain read-outs are rung 0's
    np.testing.assert_array_equal(got["logp0"], got["logp"][0])
    np.testing.assert_array_equal(got["nacc0"], got["nacc"][0])
    np.testing.assert_array_equal(got["logp"], got["logprior"] + got["loglike"])


LADDERS = {3: [1.0, 0.3, 0.0], 4: [1.0, 0.5, 0.2, 0.05], 8: [*(1e-3 ** (np.arange(7) / 6.0)), 0.0]}


# ---- 1. device == yardstick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", ["default", "eager"])
@pytest.mark.parametrize("mapping", ["lane", "obs"])
@pytest.mark.parametrize("mv,nw,nd,ndata,G,T,se,prior", [
    ("stretch", 100, 3, 1000, 24, 8, 1, "gauss"),
    ("de", 64, 4, 257, 20, 4, 3, "gauss"),
    ("snooker", 96, 3, 333, 20, 3, 1, "box"),
    ("mix", 256, 5, 100, 16, 8, 3, "gauss"),
    ("stretch", 64, 2, 1, 20, 3, 0, "none"),
], ids=["stretch100x3", "de64x4", "snooker-box", "mix256x5", "noswaps-1obs"])
def test_parity_with_the_yardstick(kmc, kmc_debug, monkeypatch, launch, mapping, mv, nw, nd, ndata, G, T, se, prior):
    kmc_debug.set("data-map", mapping)
    if launch == "eager":
        monkeypatch.setenv("KMC_LAUNCH", "eager")
    D, beta = reg_data(ndata, nd, nw + ndata)
    p0, half_width = 4.0, 1.5
    body = {"gauss": GAUSS_PRIOR, "box": BOX_PRIOR, "none": None}[prior]
    fn = {"gauss": gauss_prior, "box": lambda X: box_prior(X, half_width), "none": None}[prior]
    dd = kmc.DataDensity(REG_TERM, D, prior=body, params=[p0, half_width])
    th = beta + 0.05 * np.random.default_rng(nd).standard_normal((nw, nd))
    lib_move, y_move = moves(kmc, mv)
    nburn, nthin = G // 4, 2
    got = run(kmc, dd, th, LADDERS[T], G, nburn, nthin, seed=7, move=lib_move, swap_every=se)
    assert f"ntemps {T}" in got["desc"] and "likelihood tempering" in got["desc"] and "data_fold_split" in got["desc"], got["desc"]
    assert ("data_partial_lane" if mapping == "lane" else "data_partial_obs") in got["desc"], got["desc"]
    want = dy.emcee_data_tempered(dy.data_logpdf(lambda X: reg_terms(X, D, p0), fn), th, LADDERS[T], G, nburn, nthin, seed=7, move=y_move, swap_every=se)
    assert_matches(got, want)
    assert 0 < got["nacc"].sum() < T * nw * (G - nburn)
    assert (got["nswap"].sum() > 0) == (se > 0)
    # launches: 8 per generation (four per half-step, whatever ntemps is), plus the sweep node where it has work (a stored sample or a sweep)
    ns = (G - nburn) // nthin
    stored = lambda g: g + 1 - nburn > 0 and (g + 1 - nburn) % nthin == 0 and (g + 1 - nburn) // nthin <= ns
    assert got["launches"] == 8 * G + sum(1 for g in range(G) if stored(g) or (se > 0 and (g + 1) % se == 0))


def test_a_ladder_given_rung_by_rung_and_set_positions_evaluates_loglike(kmc):
    T, nw, nd, ndata = 4, 64, 3, 300
    D, beta = reg_data(ndata, nd, 5)
    dd = kmc.DataDensity(REG_TERM, D, prior=GAUSS_PRIOR, params=[2.0])
    th = beta + 0.1 * np.random.default_rng(8).standard_normal((T, nw, nd))
    f2 = dy.data_logpdf(lambda X: reg_terms(X, D, 2.0), gauss_prior)
    with kmc.Sampler(dd, nw, nd, 10, 0, 1, 2.0, 3, betas=LADDERS[4], temper="likelihood") as s:
        s.set_positions(th)
        for t in range(T):                                                # the numpy tree of those rows
            pri, S = f2(th[t])
            np.testing.assert_array_equal(s.rung_loglike()[t], S)
            np.testing.assert_array_equal(s.rung_logprior()[t], pri)
            np.testing.assert_array_equal(s.rung_logp()[t], pri + S)
        s.set_positions(th[1])                                            # [nw, nd]: every rung starts there
        np.testing.assert_array_equal(s.rung_loglike(), np.broadcast_to(f2(th[1])[1], (T, nw)))
    got = run(kmc, dd, th, LADDERS[4], 12, 2, 1, seed=3)
    assert_matches(got, dy.emcee_data_tempered(f2, th, LADDERS[4], 12, 2, 1, seed=3))


# ---- 2. rung 0 is the plain sampler ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", ["stretch", "de", "snooker", "mix"])
def test_rung0_of_a_ladder_without_swaps_is_the_plain_data_density_sampler(kmc, mv):
    nw, nd, ndata, G = 100, 3, 1000, 30
    D, beta = reg_data(ndata, nd, 1)
    dd = kmc.DataDensity(REG_TERM, D, prior=GAUSS_PRIOR, params=[4.0])
    th = beta + 0.05 * np.random.default_rng(0).standard_normal((nw, nd))
    got = run(kmc, dd, th, LADDERS[8], G, 5, 1, seed=19, move=moves(kmc, mv)[0], swap_every=0)
    with kmc.Sampler(dd, nw, nd, G, 5, 1, 2.0, 19, store_chain=True, store_logp=True, move=moves(kmc, mv)[0]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        ch, cl = s.chain()
        np.testing.assert_array_equal(got["pos"][0], s.positions())
        np.testing.assert_array_equal(got["logp"][0], s.logp())
        np.testing.assert_array_equal(got["nacc"][0], s.naccept())
        np.testing.assert_array_equal(got["chain"], ch)
        np.testing.assert_array_equal(got["chain_logp"], cl)
        assert "tempering" not in s.describe()
        with pytest.raises(ValueError):
            s.rung_loglike()
    assert not np.array_equal(got["pos"][1], got["pos"][0])


# ---- 3. state -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", ["stretch", "mix"])
def test_state_restore_resumes_bit_for_bit(kmc, mv):
    nw, nd, ndata = 128, 4, 500
    D, beta = reg_data(ndata, nd, 2)
    dd = kmc.DataDensity(REG_TERM, D, prior=GAUSS_PRIOR, params=[4.0])
    th = beta + 0.05 * np.random.default_rng(3).standard_normal((nw, nd))
    G, cut = 40, 17                                                        # (the cut is no multiple of swap_every)
    mk = lambda: kmc.Sampler(dd, nw, nd, G, 6, 1, 2.0, 9, move=moves(kmc, mv)[0], betas=LADDERS[8], swap_every=3, temper="likelihood")
    read = lambda s: (s.rung_positions(), s.rung_logp(), s.rung_loglike(), s.rung_logprior(), s.rung_naccept(), s.nswap(), s.rung_loglike_sum())
    with mk() as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        want = read(s)
        want_mean = s.rung_loglike_mean()
    with mk() as s:
        s.set_positions(th)
        s.run(cut)
        st = s.state()
    assert st["rung_loglike_sum"].shape == (8,) and np.all(st["rung_loglike_sum"] != 0.0)
    with mk() as s:
        s.restore(st)
        np.testing.assert_array_equal(s.rung_loglike_sum(), st["rung_loglike_sum"])
        s.run(G - cut)
        s.sync()
        got = read(s)
        np.testing.assert_array_equal(s.rung_loglike_mean(), want_mean)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_chains_moments_and_emcee_are_rung_0s(kmc):
    nw, nd, ndata, G = 64, 3, 200, 40
    D, beta = reg_data(ndata, nd, 4)
    dd = kmc.DataDensity(REG_TERM, D, prior=GAUSS_PRIOR, params=[4.0])
    th = beta + 0.05 * np.random.default_rng(5).standard_normal((nw, nd))
    dev = run(kmc, dd, th, LADDERS[4], G, 8, 2, seed=6)
    for kw in (dict(stream_chain=True), dict()):
        with kmc.Sampler(dd, nw, nd, G, 8, 2, 2.0, 6, store_chain=True, store_logp=True, moments=True, betas=LADDERS[4], temper="likelihood", **kw) as s:
            s.set_positions(th)
            s.run(G)
            s.sync()
            ch, cl = s.chain()
            bw, bl = s.chain(by_walker=True)
            msum, msq, n = s.moments()
        np.testing.assert_array_equal(ch, dev["chain"])
        np.testing.assert_array_equal(cl, dev["chain_logp"])
        np.testing.assert_array_equal(bw, dev["chain"].transpose(1, 0, 2))
        np.testing.assert_array_equal(bl, dev["chain_logp"].T)
        assert n == ch.shape[0] * ch.shape[1]
        np.testing.assert_allclose(msum, ch.sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(msq, (ch * ch).sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)
    thetas, acc, logd, blobs = kmc.emcee(dd, th, niter=nw * G, nburnin=nw * 8, nthin=2, use_progress_meter=False, seed=6, betas=LADDERS[4], temper="likelihood")
    np.testing.assert_array_equal(thetas, dev["chain"].transpose(1, 0, 2))
    np.testing.assert_array_equal(logd, dev["chain_logp"].T)
    assert blobs is None and acc.shape == (nw,)


# ---- 4. the evidence ------------------------------------------------------------------------------------------------------
# dy.EvidenceModel: 200 observations, 2 parameters, normalised N(0, 0.3^2 I) prior and normalised term, 24 rungs (23 geometric down to
# 1e-3, then 0), 64 walkers, 1 200 generations of which 400 burned, a sweep after every generation, the stretch move.
# Ten runs of the numpy yardstick on the CPU, seeds 2000 .. 2009 (the device equals the yardstick bit for bit, so seed 2000's figures
# are the device's):
#   worst over the rungs of |rung_loglike_mean - analytic <S>_beta|:  0.145 0.133 0.218 0.129 0.214 0.137 0.110 0.176 0.154 0.192
#   log_evidence - analytic trapezoid:                                  +0.0197 +0.0047 -0.0122 -0.0004 -0.0137 -0.0065 +0.0119 +0.0053 -0.0129 -0.0167
#   log_evidence - exact log Z:                                         -0.0104 -0.0254 -0.0423 -0.0305 -0.0438 -0.0366 -0.0182 -0.0248 -0.0430 -0.0468
# Bounds: twice the worst deviation seen, as MODES_BOUND was set.
EV_MEAN_BOUND = 0.436
EV_TRAP_BOUND = 0.0394
EV_EXACT_BOUND = 0.0936


def test_the_evidence_of_a_conjugate_regression(kmc):
    m = dy.EvidenceModel()
    dd = kmc.DataDensity(dy.EV_TERM, m.D, prior=dy.EV_PRIOR, params=m.params)
    ana = np.array([m.mean_loglike(b) for b in m.betas])
    trap, _ = kmc.thermodynamic_integration(m.betas, ana)
    with kmc.Sampler(dd, m.nw, 2, m.G, m.nburn, 1, 2.0, 2000, betas=m.betas, swap_every=1, temper="likelihood") as s:
        s.set_positions(m.theta0)
        s.run(m.G)
        s.sync()
        mean = s.rung_loglike_mean()
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                # the ladder ends in 0: nothing to warn about
            logz, err = s.log_evidence()
        rates = s.swap_rates()
    print("rung_loglike_mean - analytic:", (mean - ana).round(3), "\nlog_evidence", logz, "+-", err, "analytic trapezoid", trap, "exact", m.log_z(), "swap rates", rates.round(2))
    assert np.all(np.abs(mean - ana) < EV_MEAN_BOUND), mean - ana
    assert abs(logz - trap) < EV_TRAP_BOUND and abs(logz - m.log_z()) < EV_EXACT_BOUND, (logz, trap, m.log_z())
    assert (logz, err) == kmc.thermodynamic_integration(m.betas, mean)
    # a ladder that stops above 0 warns; a sampler without likelihood tempering raises
    with kmc.Sampler(dd, m.nw, 2, 20, 0, 1, 2.0, 1, betas=[1.0, 0.5], temper="likelihood") as s:
        s.set_positions(m.theta0)
        s.run(20)
        with pytest.warns(UserWarning, match="beta = 0.5"):
            s.log_evidence()
    with kmc.Sampler(kmc.GaussianIso(), 64, 2, 20, 0, 1, 2.0, 1, betas=[1.0, 0.5]) as s:
        with pytest.raises(ValueError, match="likelihood"):
            s.log_evidence()


# ---- 5. separated modes ---------------------------------------------------------------------------------------------------
TWO_MODES_TERM = ("double a = 0.0, b = 0.0; for (int i = 0; i < n; ++i) { const double m = (i == 0) ? d[0] : 0.0; a += (x[i] - m) * (x[i] - m); "
                  "b += (x[i] + m) * (x[i] + m); } a = -0.5 * a; b = -0.5 * b; const double mx = a > b ? a : b; return mx + log(exp(a - mx) + exp(b - mx));")


def test_a_likelihood_tempered_ladder_equalises_two_modes_a_plain_data_density_cannot_cross(kmc):
    """test_a_ladder_equalises_two_modes_the_stretch_move_cannot_cross with its target as a data density: ONE observation, the mode
    offset d / 2, whose term is the log-sum of the two unit Gaussians; a flat prior.  Same start, ladder, seed and length, same
    bound.  With a prior of exactly 0, q = 0 + beta S has the bits of beta S, so the shares are the whole-mode test's (0.490 on rung
    0 of the ladder, 0.804 without it)."""
    nw, d, G = MODES["nw"], MODES["d"], MODES["G"]
    th = two_mode_start(nw, d, 0)
    dd = kmc.DataDensity(TWO_MODES_TERM, np.array([[d / 2]]))
    shares = {}
    for name, kw in (("plain", {}), ("tempered", dict(betas=MODES["betas"], swap_every=1, temper="likelihood"))):
        with kmc.Sampler(dd, nw, 4, G, G // 2, 1, 2.0, 1000, store_chain=True, **kw) as s:
            s.set_positions(th)
            s.run(G)
            s.sync()
            ch, _ = s.chain(logp=False)
            assert ("ntemps 6" in s.describe()) == (name == "tempered")
        shares[name] = float(np.mean(ch[:, :, 0] > 0))
    print("share of the first mode:", shares)
    assert abs(shares["tempered"] - 0.5) < MODES_BOUND, shares
    assert abs(shares["plain"] - 0.5) >= MODES_BOUND, shares


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_by_status_and_message(kmc, oracle):
    D, _ = reg_data(300, 3, 1)
    dd = kmc.DataDensity(REG_TERM, D, params=[4.0])
    U = kmc._lib.ERR_UNSUPPORTED
    others = [(kmc.GaussianIso(), 3), (kmc.ExprDensity("-0.5*x*x"), 3), (kmc.CDensity("return -0.5 * x[0] * x[0] - 0.5 * x[1] * x[1];"), 2),
              (kmc.HostLogPdf(lambda X: -0.5 * (np.asarray(X) ** 2).sum(axis=1), vectorized=True), 3)]
    for pdf, nd in others:                                 # nothing says where another density's prior ends
        with pytest.raises(kmc.KmcError) as e:
            kmc.Sampler(pdf, 64, nd, 10, 0, 1, 2.0, 1, betas=[1.0, 0.5], temper="likelihood")
        assert e.value.status == U and "tempering" in str(e.value) and "KMC_DATA_DENSITY" in str(e.value)
    with pytest.raises(kmc.KmcError) as e:                 # the default mode stays refused, and says where to go
        kmc.Sampler(dd, 64, 3, 10, 0, 1, 2.0, 1, betas=[1.0, 0.5])
    assert e.value.status == U and "tempering" in str(e.value) and 'temper="likelihood"' in str(e.value)
    for kw in (dict(dtype="f32"), dict(island_gens=8, island_size=64), dict(shard_count=2), dict(p2p=True), dict(deal_rank=0, deal_count=2)):
        with pytest.raises(kmc.KmcError) as e:
            kmc.Sampler(dd, 64, 3, 10, 0, 1, 2.0, 1, betas=[1.0, 0.5], temper="likelihood", **kw)
        assert e.value.status == U, kw
    with pytest.raises(ValueError):
        kmc.Sampler(dd, 64, 3, 10, 0, 1, 2.0, 1, betas=[1.0, 0.0])                     # beta = 0 in whole mode
    with kmc.Sampler(dd, 64, 3, 10, 0, 1, 2.0, 1, betas=[1.0, 0.5, 0.0], temper="likelihood") as s:
        s.set_positions(np.random.default_rng(0).standard_normal((64, 3)))
        for call, word in ((lambda: s.init_ball(np.zeros(3), np.ones(3)), "init_ball"), (lambda: s.half_step(0), "whole generations"),
                           (lambda: s.bind_positions(16), "tempering")):
            with pytest.raises(kmc.KmcError) as e:
                call()
            assert e.value.status in (U, kmc._lib.ERR_BAD_ARG) and word in str(e.value), str(e.value)
