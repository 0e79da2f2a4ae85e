"""GPU: the adaptive ladder (kmc.Sampler(..., adapt=...) / kmc_config.adapt) against its numpy yardstick
(tests/adaptive_ladder_yardstick.py).  Decisions, counters, positions, the chain, S and round_acc are compared bit for bit, log-pdfs
under DESIGN.md section 6's bar (1e-12: the device's log-density and log against the host's are to rounding, the reservation of
tempering_yardstick's docstring), the betas to T * 4 * 2^-52 relative (one exp per rung and update is to rounding; S is exact on both
sides, so the difference does not accumulate).  Then: the same run in every launch mode and across a checkpoint, the frozen ladder,
the likelihood mode, the guard, refusals, and the convergence case of tests/test_adaptive_ladder_cpu.py."""
import numpy as np
import pytest

import adaptive_ladder_yardstick as ay
import data_tempering_yardstick as dy
import snooker_yardstick as sy
from test_adaptive_ladder_cpu import CONV, CONV_BOUND, conv_start, conv_yardstick, small_evidence_model, spacing_ratio
from test_gpu_de_move import GENERAL_BODY, general_body_host, menu_logpdf

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LADDER5 = [1.0, 0.6, 0.35, 0.2, 0.1]
ADAPT = dict(time=2.0)


def read(s):
    b, S, ra, sk = s._ladder()
    ch, cl = s.chain()
    return dict(pos=s.rung_positions(), logp=s.rung_logp(), nacc=s.rung_naccept(), nswap=s.nswap().astype(np.int64), chain=ch, chain_logp=cl,
                logp_sum=s.rung_logp_sum(), betas=b, S=S, round_acc=ra.astype(np.int64), skipped=sk, desc=s.describe())


def run(kmc, pdf, th, betas, G, nburn, seed=11, move=None, swap_every=1, adapt=ADAPT, half_steps=False, **kw):
    nw, nd = th.shape[-2:]
    with kmc.Sampler(pdf, nw, nd, G, nburn, 1, 2.0, seed, store_chain=True, store_logp=True, move=move, betas=betas, swap_every=swap_every,
                     adapt=adapt, **kw) as s:
        s.set_positions(th)
        if half_steps:
            for _ in range(G):
                s.half_step(0)
                s.half_step(1)
        else:
            s.run(G // 2)
            s.run(G - G // 2)
        s.sync()
        return read(s)


def assert_ladder_matches(got, want):
    T = want["betas"].size
    np.testing.assert_array_equal(got["S"], want["S"])
    np.testing.assert_array_equal(got["round_acc"], want["round_acc"])
    assert got["skipped"] == want["skipped"]
    assert got["betas"][0] == 1.0 and got["betas"][-1] == want["betas"][-1] and np.all(np.diff(got["betas"]) < 0)
    assert np.all(np.abs(got["betas"] - want["betas"]) <= T * 4 * EPS * want["betas"]), (got["betas"] - want["betas"]) / EPS


def assert_matches(got, want):
    for k in ("nacc", "nswap", "pos", "chain"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    tol = lambda a: 1e-12 * np.maximum(1.0, np.abs(a))
    assert np.all(np.abs(got["logp"] - want["logp"]) <= tol(want["logp"]))
    assert np.all(np.abs(got["chain_logp"] - want["chain_logp"]) <= tol(want["chain_logp"]))
    assert np.all(np.abs(got["logp_sum"] - want["logp_sum"]) <= 1e-11 * np.maximum(1.0, np.abs(want["logp_sum"])))
    assert_ladder_matches(got, want)


def assert_identical(a, b):
    for k in ("nacc", "nswap", "pos", "logp", "chain", "chain_logp", "betas", "S", "round_acc"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["skipped"] == b["skipped"]


# ---- 1. device == yardstick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,mv,se", [(40, "stretch", 1), (40, "stretch", 3), (40, "mix", 1), (600, "stretch", 1), (600, "stretch", 3)])
def test_gaussian_matches_the_yardstick(kmc, oracle, nw, mv, se):
    """T = 5, ndim = 3 (a padded row); 40 walkers: one block, no multiple of 64; 600: three blocks per rung, the ticket drawn across
    blocks; 60 generations of which 40 burned, so the ladder moves for 40 (swap_every 3: 13 sweeps, 6 rounds) and is frozen for 20."""
    th = np.random.default_rng(nw).standard_normal((nw, 3))
    lib_move, y_move = {"stretch": (None, None), "mix": ([(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)], [(sy.DE(), 0.8), (sy.Snooker(), 0.2)])}[mv]
    got = run(kmc, kmc.GaussianIso(), th, LADDER5, 60, 40, seed=5, move=lib_move, swap_every=se)
    assert "adaptive ladder: until generation 40, lag 10000, time 2" in got["desc"] and "temper_sweep_adapt<whole>" in got["desc"], got["desc"]
    want = ay.emcee_tempered(menu_logpdf(oracle, 0, [0.0, 1.0]), th, LADDER5, 60, 40, 1, seed=5, move=y_move, swap_every=se, adapt=ADAPT)
    assert_matches(got, want)
    assert np.max(np.abs(got["betas"][1:-1] - np.array(LADDER5)[1:-1])) > 0.01                 # the ladder visibly moved
    assert got["nswap"].sum() > 0


def test_a_function_body_matches_the_yardstick(kmc):
    th = np.random.default_rng(4).standard_normal((40, 3))
    got = run(kmc, kmc.CDensity(GENERAL_BODY, params=[4.0]), th, LADDER5, 60, 40, seed=21)
    want = ay.emcee_tempered(lambda X: general_body_host(X, 4.0), th, LADDER5, 60, 40, 1, seed=21, adapt=ADAPT)
    assert_matches(got, want)


# ---- 2. the same run every way --------------------------------------------------------------------------------------------
def test_launch_modes_and_half_steps_agree(kmc, monkeypatch):
    th = np.random.default_rng(600).standard_normal((600, 3))
    res = {}
    for mode in ("graph", "eager"):
        monkeypatch.setenv("KMC_LAUNCH", mode)
        res[mode] = run(kmc, kmc.GaussianIso(), th, LADDER5, 60, 40, seed=5)
    monkeypatch.delenv("KMC_LAUNCH")
    res["half"] = run(kmc, kmc.GaussianIso(), th, LADDER5, 60, 40, seed=5, half_steps=True)
    assert_identical(res["graph"], res["eager"])
    assert_identical(res["graph"], res["half"])
    assert not np.array_equal(res["graph"]["betas"], LADDER5)


@pytest.mark.parametrize("temper", ["whole", "likelihood"])
def test_state_restore_inside_a_round_resumes_bit_for_bit(kmc, temper):
    """The checkpoint is taken after 7 sweeps: the even sweep of round 3 has counted, its odd sweep has not run."""
    if temper == "whole":
        pdf, nd, betas = kmc.GaussianIso(), 3, LADDER5
        th = np.random.default_rng(1).standard_normal((600, nd))
    else:
        m = small_evidence_model()
        pdf, nd, betas = kmc.DataDensity(dy.EV_TERM, m.D, prior=dy.EV_PRIOR, params=m.params), 2, [1.0, 0.3, 0.05, 0.0]
        th = m.theta0
    nw = th.shape[0]
    mk = lambda: kmc.Sampler(pdf, nw, nd, 30, 20, 1, 2.0, 9, betas=betas, swap_every=1, adapt=ADAPT, temper=temper)   # (no chain: restore refuses it)
    read = lambda s: dict(zip(("betas", "S", "round_acc", "skipped"), s._ladder()), pos=s.rung_positions(), logp=s.rung_logp(),
                          nacc=s.rung_naccept(), nswap=s.nswap(), logp_sum=s.rung_logp_sum())
    with mk() as s:
        s.set_positions(th)
        s.run(30)
        s.sync()
        want = read(s)
    with mk() as s:
        s.set_positions(th)
        s.run(7)
        st = s.state()
        assert st["round_acc"].any() and st["S"].shape == (len(betas) - 2,) and not np.array_equal(st["betas"], betas)
    with mk() as s:
        s.restore(st)
        np.testing.assert_array_equal(s.betas, st["betas"])
        s.run(23)
        s.sync()
        got = read(s)
    for k in ("nacc", "nswap", "pos", "logp", "betas", "S", "round_acc"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["skipped"] == want["skipped"] and not np.array_equal(got["betas"], st["betas"])
    np.testing.assert_allclose(got["logp_sum"], want["logp_sum"], rtol=1e-11)


# ---- 3. the frozen ladder -------------------------------------------------------------------------------------------------
def test_the_ladder_is_frozen_from_adapt_until_on(kmc):
    """A checkpoint restore refuses chain storage, so "the chain after burn-in" is read as the whole ladder's positions, log-pdfs and
    counters after each of the 20 generations that follow burn-in -- every stored sample and more."""
    th = np.random.default_rng(3).standard_normal((40, 3))
    mk = lambda **kw: kmc.Sampler(kmc.GaussianIso(), 40, 3, 60, 40, 1, 2.0, 7, **kw)

    def after_burn_in(s):
        out = []
        for _ in range(20):
            s.run(1)
            out.append((s.rung_positions(), s.rung_logp(), s.rung_naccept(), s.nswap()))
        return out

    def same(a, b):
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                np.testing.assert_array_equal(u, v)

    with mk(betas=LADDER5, adapt=ADAPT) as s:
        s.set_positions(th)
        np.testing.assert_array_equal(s.betas, LADDER5)
        s.run(39)
        b39 = s.betas
        s.run(1)
        b40, st40 = s.betas, s.state()
        traj = after_burn_in(s)
        b60 = s.betas
        np.testing.assert_array_equal(s.betas0, LADDER5)
        assert s.adapt_skipped == 0 and s.generation == 60
    assert not np.array_equal(b39, b40)                                    # the sweep of generation 39 still adapts
    np.testing.assert_array_equal(b40, b60)
    assert traj[-1][3].sum() > 0
    with mk(betas=LADDER5, adapt=dict(time=2.0, until=10)) as s:
        s.set_positions(th)
        s.run(10)
        b10 = s.betas
        s.run(50)
        np.testing.assert_array_equal(s.betas, b10)
        assert not np.array_equal(b10, LADDER5) and "until generation 10" in s.describe()
    # a fixed ladder set to the adapted one reproduces the run after burn-in, both restored from the same state
    with mk(betas=b60) as s:
        assert s.betas is s.betas0 and "adaptive" not in s.describe()
        s.restore(st40)
        same(after_burn_in(s), traj)
    with mk(betas=LADDER5, adapt=ADAPT) as s:
        s.restore(st40)
        same(after_burn_in(s), traj)
        np.testing.assert_array_equal(s.betas, b60)
        s.set_positions(th)                                                # a fresh start: the ladder starts again from the caller's
        np.testing.assert_array_equal(s.betas, LADDER5)
        assert not s._ladder()[2].any()


# ---- 4. likelihood mode ---------------------------------------------------------------------------------------------------
def test_likelihood_mode_matches_the_yardstick_and_the_evidence_uses_the_adapted_ladder(kmc):
    """The conjugate regression of tests/test_gpu_data_tempering.py at 60 observations: 6 rungs ending in the prior rung, 64 walkers,
    80 generations of which 40 burned.  The term and the prior are exact against numpy, so every bit but the betas' is compared."""
    m = small_evidence_model()
    betas = [1.0, 0.5, 0.2, 0.05, 0.01, 0.0]
    dd = kmc.DataDensity(dy.EV_TERM, m.D, prior=dy.EV_PRIOR, params=m.params)
    with kmc.Sampler(dd, m.nw, 2, 80, 40, 1, 2.0, 2000, store_chain=True, store_logp=True, betas=betas, swap_every=1, temper="likelihood",
                     adapt=ADAPT) as s:
        s.set_positions(m.theta0)
        s.run(80)
        s.sync()
        got = read(s)
        got.update(loglike=s.rung_loglike(), logprior=s.rung_logprior(), loglike_sum=s.rung_loglike_sum())
        assert "temper_sweep_adapt<like>" in got["desc"], got["desc"]
        assert s.log_evidence() == kmc.thermodynamic_integration(s.betas, s.rung_loglike_mean())
        assert s.log_evidence() != kmc.thermodynamic_integration(s.betas0, s.rung_loglike_mean())
    want = ay.emcee_data_tempered(dy.data_logpdf(m.term_fn, m.prior_fn), m.theta0, betas, 80, 40, 1, seed=2000, swap_every=1, adapt=ADAPT)
    for k in ("nacc", "nswap", "pos", "logp", "loglike", "logprior", "chain", "chain_logp", "loglike_sum"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_allclose(got["logp_sum"], want["logp_sum"], rtol=1e-11)
    assert_ladder_matches(got, want)
    assert got["betas"][-1] == 0.0 and np.max(np.abs(got["betas"][1:-1] - np.array(betas)[1:-1])) > 0.01


# ---- 5. the guard ---------------------------------------------------------------------------------------------------------
def test_the_guard_skips_rounds_on_the_device_as_in_the_yardstick(kmc, oracle):
    """Four rungs whose last gap is tiny and time = 0.05: a round in which pair 1 accepts more than pair 2 sends beta_2 below the last
    rung; those rounds are not committed (the yardstick skips 12 of the 15 rounds here and commits 3)."""
    betas = [1.0, 0.5, 0.102, 0.1]
    adapt = dict(time=0.05, lag=10000.0)
    th = np.random.default_rng(6).standard_normal((40, 3))
    got = run(kmc, kmc.GaussianIso(), th, betas, 40, 30, seed=13, adapt=adapt)
    want = ay.emcee_tempered(menu_logpdf(oracle, 0, [0.0, 1.0]), th, betas, 40, 30, 1, seed=13, adapt=adapt)
    assert 1 <= want["skipped"] < 15
    assert_matches(got, want)
    assert np.all(np.diff(got["betas"]) < 0) and got["betas"][-1] == 0.1


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_by_status_and_message(kmc):
    from kissmcmc_jl_amd import _lib
    mk = lambda nburn=10, **kw: kmc.Sampler(kmc.GaussianIso(), 40, 3, 20, nburn, **kw)
    for kw in (dict(adapt=True), dict(betas=[1.0, 0.5], adapt=True), dict(betas=LADDER5, swap_every=0, adapt=True),
               dict(betas=LADDER5, adapt=dict(until=-1)), dict(betas=LADDER5, adapt=dict(until=11)), dict(betas=LADDER5, adapt=dict(lag=0.0)),
               dict(betas=LADDER5, adapt=dict(lag=float("inf"))), dict(betas=LADDER5, adapt=dict(time=-1.0)),
               dict(betas=LADDER5, adapt=dict(time=float("nan")))):
        with pytest.raises(kmc.KmcError, match="adaptive ladder") as e:
            mk(**kw)
        assert e.value.status == _lib.ERR_BAD_ARG, kw
    with mk(betas=LADDER5, adapt=True) as s:
        assert "until generation 10, lag 10000, time 100" in s.describe()
    with pytest.raises(kmc.KmcError, match="adaptive ladder"):            # nburnin = 0: nothing to adapt in ... until = 0 means nburnin = 0
        mk(nburn=0, betas=LADDER5, adapt=dict(until=1))
    # what tempering refuses stays refused, in tempering's name
    with pytest.raises(kmc.KmcError, match="parallel tempering.*KMC_F32") as e:
        mk(betas=LADDER5, adapt=True, dtype="f32")
    assert e.value.status == _lib.ERR_UNSUPPORTED and "adaptive" not in str(e.value)
    m = small_evidence_model()
    with pytest.raises(kmc.KmcError, match="parallel tempering.*KMC_DATA_DENSITY in the default temper_mode"):
        kmc.Sampler(kmc.DataDensity(dy.EV_TERM, m.D, prior=dy.EV_PRIOR, params=m.params), 40, 2, 20, 10, betas=LADDER5, adapt=True)
    with pytest.raises(kmc.KmcError, match="parallel tempering.*KMC_HOST_DENSITY"):
        kmc.Sampler(kmc.HostLogPdf(lambda x: -0.5 * float(np.sum(x * x))), 40, 3, 20, 10, betas=LADDER5, adapt=True)
    # a fixed ladder has no ladder state to set, and the first and last rung never move
    with mk(betas=LADDER5) as s:
        assert s.adapt is None and s.adapt_skipped == 0
        z = np.zeros(4, dtype=np.uint64)
        with pytest.raises(kmc.KmcError, match="without an adaptive ladder"):
            _lib.check(s._L.kmc_sampler_set_ladder(s._h, s.betas0.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)), s.betas0.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)),
                                                   z.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)), z.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64))))
    with mk(betas=LADDER5, adapt=True) as s:
        s.set_positions(np.random.default_rng(0).standard_normal((40, 3)))
        st = s.state()
        st["betas"] = np.array([1.0, 0.6, 0.35, 0.2, 0.15])
        with pytest.raises(kmc.KmcError, match="never move"):
            s.restore(st)


# what tempering refuses stays refused with adapt set, in tempering's name: tests/test_gpu_tempering.py's list, adapt=True added (this
# pins the order of the blocks in kmc_validate: tempering's refusals come before the adaptive ladder's)
LADDER3 = [1.0, 0.5, 0.2]


def assert_names_tempering(kmc, status, msg):
    assert status == kmc._lib.ERR_UNSUPPORTED and "tempering" in msg and "adaptive" not in msg, (status, msg)


@pytest.mark.parametrize("kw", [dict(dtype="f32"), dict(island_gens=8, island_size=64), dict(shard_count=2), dict(p2p=True),
                                dict(deal_rank=0, deal_count=2)])
def test_what_tempering_refuses_is_refused_in_its_name_with_adapt_set(kmc, kw):
    with pytest.raises(kmc.KmcError) as e:
        kmc.Sampler(kmc.GaussianIso(), 256, 4, 10, 5, 1, 2.0, 1, betas=LADDER3, adapt=True, **kw)
    assert_names_tempering(kmc, e.value.status, str(e.value))


def test_host_data_and_blob_densities_and_whole_ensemble_calls_are_refused_with_adapt_set(kmc, oracle):
    import ctypes as C
    from test_data_density_cpu import REG_TERM
    from test_gpu_data_density import reg_data
    D, _ = reg_data(300, 3, 1)
    blob = kmc.CDensity("blob[0] = x[0]; return -0.5 * x[0] * x[0] - 0.5 * x[1] * x[1];", nblob=1)
    for pdf, nd in ((kmc.HostLogPdf(menu_logpdf(oracle, 0, [0.0, 1.0]), vectorized=True), 3), (kmc.DataDensity(REG_TERM, D, params=[4.0]), 3), (blob, 2)):
        with pytest.raises(kmc.KmcError) as e:
            kmc.Sampler(pdf, 64, nd, 10, 5, 1, 2.0, 1, betas=LADDER3, adapt=True)
        assert_names_tempering(kmc, e.value.status, str(e.value))
    with kmc.Sampler(kmc.GaussianIso(), 64, 3, 10, 5, 1, 2.0, 1, betas=LADDER3, adapt=True) as s:
        for call in (lambda: s.init_ball(np.zeros(3), np.ones(3)), lambda: s.bind_positions(16)):
            with pytest.raises(kmc.KmcError) as e:
                call()
            assert_names_tempering(kmc, e.value.status, str(e.value))
        z = np.zeros((64, 3))
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        st = s._L.kmc_sampler_set_state(s._h, dp(z), dp(z[:, 0].copy()), None, 0)
        assert_names_tempering(kmc, st, s._L.kmc_last_error().decode())


# ---- 7. what the rule is for ----------------------------------------------------------------------------------------------
def test_a_linear_ladder_over_a_gaussian_becomes_geometric_on_the_device(kmc):
    """The case of test_adaptive_ladder_cpu.test_a_linear_ladder_over_a_gaussian_becomes_geometric at seed 0, with its bound."""
    betas0, th = conv_start(0)
    with kmc.Sampler(kmc.GaussianIso(), CONV["nw"], CONV["nd"], CONV["G"], CONV["G"], 1, 2.0, 0, betas=betas0, swap_every=1,
                     adapt=dict(lag=CONV["lag"], time=CONV["time"])) as s:
        s.set_positions(th)
        s.run(CONV["G"])
        s.sync()
        b, S, ra, sk = s._ladder()
        pos = s.rung_positions()
    ratio = spacing_ratio(b)
    print("interior log-spacings max / min on the device:", ratio, "betas", b)
    assert ratio < CONV_BOUND, ratio
    want = conv_yardstick(0)
    np.testing.assert_array_equal(S, want["S"])
    np.testing.assert_array_equal(pos, want["pos"])
    assert sk == want["skipped"] and np.all(np.abs(b - want["betas"]) <= CONV["T"] * 4 * EPS * want["betas"])
