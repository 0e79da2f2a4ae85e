"""GPU: parallel tempering (kmc.Sampler(..., betas=...) / kmc_config.ntemps) against its numpy yardstick
(tests/tempering_yardstick.py), bit for bit under DESIGN.md section 6's bar on every rung, for the four moves and every kernel route
a tempered sampler takes; rung 0 against the plain sampler; launch paths, half-steps, checkpoints, chains; the ladder's statistics;
the two-mode target the feature is for; refusals.  Modelled test for test on tests/test_gpu_snooker_move.py."""
import numpy as np
import pytest

import snooker_yardstick as sy
import tempering_yardstick as ty
from test_gpu_de_move import GENERAL_BODY, general_body_host, menu_logpdf
from test_gpu_snooker_move import TWO_MODES

pytestmark = pytest.mark.gpu

GAUSS, ROSEN = 0, 2


def moves(kmc, name):
    """(the library's move, the yardstick's)"""
    return {"stretch": (None, None), "de": (kmc.DEMove(), sy.DE()), "snooker": (kmc.DESnookerMove(), sy.Snooker()),
            "mix": ([(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)], [(sy.DE(), 0.8), (sy.Snooker(), 0.2)])}[name]


def run(kmc, pdf, th, betas, G, nburn=0, nthin=1, seed=11, move=None, swap_every=1, half_steps=False, pieces=2, **kw):
    nw, nd = th.shape[-2:]
    with kmc.Sampler(pdf, nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, move=move, betas=betas,
                     swap_every=swap_every, **kw) as s:
        s.set_positions(th)
        if half_steps:
            for _ in range(G):
                s.half_step(0)
                s.half_step(1)
        else:
            done = 0
            for i in range(pieces):
                n = G // pieces if i + 1 < pieces else G - done
                s.run(n)
                done += n
        s.sync()
        ch, cl = s.chain()
        return dict(pos=s.rung_positions(), logp=s.rung_logp(), nacc=s.rung_naccept(), nswap=s.nswap().astype(np.int64), chain=ch,
                    chain_logp=cl, logp_sum=s.rung_logp_sum(), pos0=s.positions(), logp0=s.logp(), nacc0=s.naccept(), desc=s.describe(),
                    rates=s.swap_rates(), attempts=s.swap_attempts(), launches=s.launch_count)


def assert_matches(got, want):
    """DESIGN.md section 6 on every rung: decisions, counters, positions and the chain identical; log-pdfs to 1e-12; the log-density
    sums (an order-free reduction) to 1e-11 relative, the moments' bar."""
    np.testing.assert_array_equal(got["nacc"], want["nacc"])
    np.testing.assert_array_equal(got["nswap"], want["nswap"])
    np.testing.assert_array_equal(got["pos"], want["pos"])
    np.testing.assert_array_equal(got["chain"], want["chain"])
    tol = lambda a: 1e-12 * np.maximum(1.0, np.abs(a))
    assert np.all(np.abs(got["logp"] - want["logp"]) <= tol(want["logp"]))
    assert np.all(np.abs(got["chain_logp"] - want["chain_logp"]) <= tol(want["chain_logp"]))
    assert np.all(np.abs(got["logp_sum"] - want["logp_sum"]) <= 1e-11 * np.maximum(1.0, np.abs(want["logp_sum"])))
    np.testing.assert_array_equal(got["pos0"], got["pos"][0])              # the plain read-outs are rung 0's
    np.testing.assert_array_equal(got["logp0"], got["logp"][0])
    np.testing.assert_array_equal(got["nacc0"], got["nacc"][0])


def assert_identical(a, b):
    for k in ("nacc", "nswap", "pos", "logp", "chain", "chain_logp"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_allclose(a["logp_sum"], b["logp_sum"], rtol=1e-11)


LADDERS = {2: [1.0, 0.3], 5: [1.0, 0.6, 0.35, 0.2, 0.1], 8: list(0.02 ** (np.arange(8) / 7.0))}


# ---- 1. device == yardstick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", ["stretch", "de", "snooker", "mix"])
@pytest.mark.parametrize("dens,params,nw,nd,G,kernel,T,se", [
    (GAUSS, [0.0, 1.0], 64, 4, 40, "vec", 5, 1),
    (ROSEN, [1.0, 100.0, 20.0], 128, 32, 30, "vec", 2, 3),
    (GAUSS, [0.3, 1.5], 96, 5, 30, "vec", 8, 1),
    (GAUSS, [0.0, 1.0], 256, 33, 20, "vec", 5, 3),
    (GAUSS, [0.0, 1.0], 1104, 1100, 6, "generic", 2, 1),
    (GAUSS, [0.0, 1.0], 64, 4, 24, "vec", 8, 0),
    (GAUSS, [0.0, 1.0], 208, 200, 10, "vec L=64 K=2", 2, 1),
    (GAUSS, [0.0, 1.0], 520, 512, 8, "vec L=64 K=4", 5, 3),
], ids=["gauss64x4", "rosen128x32", "ragged5", "ragged33", "ndim1100", "noswaps", "wide200", "wide512"])
def test_menu_densities_match_the_yardstick(kmc, oracle, mv, dens, params, nw, nd, G, kernel, T, se):
    th = np.random.default_rng(nd).standard_normal((nw, nd)) * 0.5 + (1.0 if dens == ROSEN else 0.0)
    pdf = kmc.GaussianIso(*params) if dens == GAUSS else kmc.Rosenbrock(*params)
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, pdf, th, LADDERS[T], G, nburn=G // 3, nthin=2, seed=5, move=lib_move, swap_every=se)
    assert f"ntemps {T}" in got["desc"] and "half_step_temper_" + kernel.split()[0] in got["desc"], got["desc"]
    assert all(word in got["desc"] for word in kernel.split()[1:]), got["desc"]            # (the 64-lane geometries of long rows)
    want = ty.emcee_tempered(menu_logpdf(oracle, dens, params), th, LADDERS[T], G, G // 3, 2, seed=5, move=y_move, swap_every=se)
    assert_matches(got, want)
    assert 0 < got["nacc"].sum() < T * nw * (G - G // 3)
    assert (got["nswap"].sum() > 0) == (se > 0)


def test_a_ladder_given_rung_by_rung_matches_the_yardstick(kmc, oracle):
    T, nw, nd, G = 5, 64, 6, 20
    th = np.random.default_rng(8).standard_normal((T, nw, nd)) / np.sqrt(np.array(LADDERS[5]))[:, None, None]
    got = run(kmc, kmc.GaussianIso(), th, LADDERS[5], G, nburn=5, seed=3)
    want = ty.emcee_tempered(menu_logpdf(oracle, GAUSS, [0.0, 1.0]), th, LADDERS[5], G, 5, 1, seed=3)
    assert_matches(got, want)


@pytest.mark.parametrize("mv", ["stretch", "mix"])
def test_expr_density_matches_the_yardstick(kmc, mv):
    nw, nd, G = 256, 16, 24
    th = np.random.default_rng(3).standard_normal((nw, nd))
    pdf = kmc.ExprDensity("-0.5*((x-p[0])*p[1])*((x-p[0])*p[1])", params=[0.25, 1.0 / 1.5])
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, pdf, th, LADDERS[5], G, nburn=4, seed=8, move=lib_move, swap_every=3)
    assert "half_step_temper_vec" in got["desc"] and "runtime-compiled" in got["desc"], got["desc"]
    f = lambda X: np.array([sum(-0.5 * ((x - 0.25) * (1.0 / 1.5)) * ((x - 0.25) * (1.0 / 1.5)) for x in row) for row in X])
    assert_matches(got, ty.emcee_tempered(f, th, LADDERS[5], G, 4, 1, seed=8, move=y_move, swap_every=3))


@pytest.mark.parametrize("mv", ["stretch", "de", "snooker"])
def test_general_body_matches_the_yardstick(kmc, mv):
    nw, nd, G = 192, 6, 24
    th = np.random.default_rng(4).standard_normal((nw, nd))
    pdf = kmc.CDensity(GENERAL_BODY, params=[4.0])
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, pdf, th, LADDERS[8], G, nburn=6, nthin=3, seed=21, move=lib_move)
    assert "ntemps 8" in got["desc"], got["desc"]
    assert_matches(got, ty.emcee_tempered(lambda X: general_body_host(X, 4.0), th, LADDERS[8], G, 6, 3, seed=21, move=y_move))


def test_a_recognised_body_matches_the_yardstick(kmc, oracle):
    nw, nd, G = 128, 8, 20
    th = np.random.default_rng(14).standard_normal((nw, nd))
    body = kmc.CDensity("double s = 0.0; for (int i = 0; i < n; ++i) { double t = (x[i] - p[0]) * p[1]; s += t * t; } return -0.5 * s;", params=[0.0, 1.0])
    got = run(kmc, body, th, LADDERS[2], G, nburn=3, seed=6)
    assert body.separable and "half_step_temper_vec" in got["desc"], got["desc"]
    assert_matches(got, ty.emcee_tempered(menu_logpdf(oracle, GAUSS, [0.0, 1.0]), th, LADDERS[2], G, 3, 1, seed=6))


# ---- 2. rung 0 is the plain sampler ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", ["stretch", "de"])
@pytest.mark.parametrize("nw,nd", [(256, 5), (4096, 32)])
def test_rung0_of_a_ladder_without_swaps_is_the_plain_sampler(kmc, monkeypatch, mv, nw, nd):
    """Bit for bit against the plain sampler in the same kernel family (the two-launch kernels, which a small plain stretch sampler
    leaves for the resident or one-launch kernels -- whose log-pdf sums round in another order); in its default mode the plain
    sampler agrees under DESIGN.md section 6's bar: everything identical, log-pdfs to 1e-12."""
    th = np.random.default_rng(0).standard_normal((nw, nd))
    G = 30
    got = run(kmc, kmc.GaussianIso(), th, LADDERS[5], G, nburn=5, seed=19, move=moves(kmc, mv)[0], swap_every=0)
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, 5, 1, 2.0, 19, store_chain=True, store_logp=True, move=moves(kmc, mv)[0]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        np.testing.assert_array_equal(got["pos"][0], s.positions())
        np.testing.assert_array_equal(got["nacc"][0], s.naccept())
        np.testing.assert_array_equal(got["chain"], s.chain()[0])
        assert np.all(np.abs(got["logp"][0] - s.logp()) <= 1e-12 * np.maximum(1.0, np.abs(s.logp())))
    monkeypatch.setenv("KMC_DEBUG", "fused=0,no-resident")
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, 5, 1, 2.0, 19, store_chain=True, store_logp=True, move=moves(kmc, mv)[0]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        ch, cl = s.chain()
        np.testing.assert_array_equal(got["pos"][0], s.positions())
        np.testing.assert_array_equal(got["logp"][0], s.logp())
        np.testing.assert_array_equal(got["nacc"][0], s.naccept())
        np.testing.assert_array_equal(got["chain"], ch)
        np.testing.assert_array_equal(got["chain_logp"], cl)
        assert "tempering" not in s.describe() and "multi-launch" in s.describe()
    assert not np.array_equal(got["pos"][1], got["pos"][0])


def test_tempering_spelled_off_changes_nothing(kmc):
    th = np.random.default_rng(0).standard_normal((4096, 32))
    outs = []
    for kw in ({}, dict(ntemps=0), dict(betas=None, swap_every=7)):
        with kmc.Sampler(kmc.GaussianIso(), 4096, 32, 30, 5, 1, 2.0, 19, store_chain=True, store_logp=True, moments=True, **kw) as s:
            s.set_positions(th)
            s.run(30)
            s.sync()
            ch, cl = s.chain()
            outs.append((s.positions(), s.logp(), s.naccept(), ch, cl, *s.moments(), s.describe()))
            with pytest.raises(ValueError):
                s.rung_positions()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            if isinstance(a, np.ndarray):
                np.testing.assert_array_equal(a, b)
            else:
                assert a == b


# ---- 3. launch paths, half-steps, checkpoints, chains ---------------------------------------------------------------------
@pytest.fixture
def c2ish():
    return np.random.default_rng(0).standard_normal((8192, 32))


@pytest.mark.parametrize("mv", ["stretch", "de", "mix"])
def test_launch_paths_agree(kmc, monkeypatch, c2ish, mv):
    res = {}
    G, nburn, nthin, swap_every = 150, 10, 3, 3
    for mode in ("graph", "eager", "updated"):
        monkeypatch.setenv("KMC_LAUNCH", mode)
        res[mode] = run(kmc, kmc.GaussianIso(), c2ish[:2048], LADDERS[5], G, nburn=nburn, nthin=nthin, seed=3, move=moves(kmc, mv)[0], swap_every=swap_every, pieces=1)
    monkeypatch.delenv("KMC_LAUNCH")
    # launches: a replayed chunk of 64 generations has the sweep node in every generation (3 per generation); a generation launched eagerly has its two
    # half-steps and the sweep only where it has work -- a sample to store (the schedule's rule) or an exchange
    nsamples = (G - nburn) // nthin
    stores = lambda g: g + 1 - nburn > 0 and (g + 1 - nburn) % nthin == 0 and (g + 1 - nburn) // nthin - 1 < nsamples
    eagerly = lambda g0: sum(2 + (stores(g) or (g + 1) % swap_every == 0) for g in range(g0, G))
    replayed = G // 64 * 64
    assert res["eager"]["launches"] == eagerly(0)
    assert res["graph"]["launches"] == 3 * replayed + eagerly(replayed)
    assert res["updated"]["launches"] == res["graph"]["launches"]          # (a ladder falls back to the table graph)
    assert "half_step_temper_vec" in res["graph"]["desc"]
    assert_identical(res["graph"], res["eager"])
    assert_identical(res["graph"], res["updated"])
    assert "fell back to the table graph" in res["updated"]["desc"] and "fell back" not in res["graph"]["desc"]      # the fallback is said


@pytest.mark.parametrize("mv", ["stretch", "snooker"])
def test_half_steps_equal_run(kmc, c2ish, mv):
    th = c2ish[:1024]
    a = run(kmc, kmc.GaussianIso(), th, LADDERS[8], 20, nburn=5, seed=4, move=moves(kmc, mv)[0], swap_every=3)
    b = run(kmc, kmc.GaussianIso(), th, LADDERS[8], 20, nburn=5, seed=4, move=moves(kmc, mv)[0], swap_every=3, half_steps=True)
    assert_identical(a, b)


@pytest.mark.parametrize("mv", ["stretch", "de"])
def test_state_restore_resumes_bit_for_bit(kmc, c2ish, mv):
    th = c2ish[:2048]
    G, cut, seed, se = 100, 41, 9, 3                                       # (the cut is no multiple of swap_every)
    mk = lambda: kmc.Sampler(kmc.GaussianIso(), 2048, 32, G, 10, 1, 2.0, seed, move=moves(kmc, mv)[0], betas=LADDERS[5], swap_every=se)
    with mk() as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        want = s.rung_positions(), s.rung_logp(), s.rung_naccept(), s.nswap()
    with mk() as s:
        s.set_positions(th)
        s.run(cut)
        st = s.state()
    assert st["positions"].shape == (5, 2048, 32) and st["nswap"].shape == (4,)
    with mk() as s:
        s.restore(st)
        s.run(G - cut)
        s.sync()
        got = s.rung_positions(), s.rung_logp(), s.rung_naccept(), s.nswap()
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_stream_chain_and_by_walker_equal_the_device_chain(kmc, c2ish):
    th = c2ish[:1024]
    G = 40
    dev = run(kmc, kmc.GaussianIso(), th, LADDERS[5], G, nburn=8, nthin=2, seed=6)
    with kmc.Sampler(kmc.GaussianIso(), 1024, 32, G, 8, 2, 2.0, 6, store_chain=True, store_logp=True, stream_chain=True, betas=LADDERS[5]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        ch, cl = s.chain()
    np.testing.assert_array_equal(ch, dev["chain"])
    np.testing.assert_array_equal(cl, dev["chain_logp"])
    with kmc.Sampler(kmc.GaussianIso(), 1024, 32, G, 8, 2, 2.0, 6, store_chain=True, store_logp=True, betas=LADDERS[5]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        bw, bl = s.chain(by_walker=True)
    np.testing.assert_array_equal(bw, dev["chain"].transpose(1, 0, 2))
    np.testing.assert_array_equal(bl, dev["chain_logp"].T)


@pytest.mark.parametrize("nw,nd", [(1024, 32), (256, 200)])
def test_moments_are_rung_0s(kmc, nw, nd):
    """The streaming moments are sojourn-weighted; a walker that leaves rung 0 in an exchange is credited by the sweep kernel
    (rows of 200: the 64-lane kernels, whose moments go through the ring of posted rows)."""
    th = np.random.default_rng(0).standard_normal((nw, nd))
    G = 60
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, 8, 2, 2.0, 6, store_chain=True, moments=True, betas=LADDERS[5]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        ch, _ = s.chain(logp=False)
        msum, msq, n = s.moments()
    assert n == ch.shape[0] * ch.shape[1]
    np.testing.assert_allclose(msum, ch.sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(msq, (ch * ch).sum(axis=(0, 1)), rtol=1e-11, atol=1e-9)


# ---- 4. statistics --------------------------------------------------------------------------------------------------------
def test_every_rung_has_its_stationary_variance_and_swaps_happen(kmc):
    """Unit Gaussian in 8-D: rung t is a Gaussian of variance 1 / beta_t.  test_stationary_variance_of_the_unit_gaussian holds
    |var - 1| < 0.01 and |mean| < 0.01 for the moments of 4096 walkers x 2000 generations; here a rung's moments come from 40
    read-outs of 4096 walkers, 50 generations apart (after 1000 of burn-in): 1 / 50 of the sample count, so the tolerances are
    0.01 sqrt(50) / beta_t for the variance and 0.01 sqrt(50) / sqrt(beta_t) for the mean (it scales with the standard deviation)."""
    nw, nd, reads, every = 4096, 8, 40, 50
    betas = np.array(LADDERS[5])
    th = np.random.default_rng(12).standard_normal((nw, nd))
    acc_sum, acc_sq = np.zeros((5, nd)), np.zeros((5, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, 1000 + reads * every, 1000, 1, 2.0, 17, betas=betas) as s:
        s.set_positions(th)
        s.run(1000)
        for _ in range(reads):
            s.run(every)
            p = s.rung_positions()
            acc_sum += p.sum(axis=1)
            acc_sq += (p * p).sum(axis=1)
        rates = s.swap_rates()
        assert np.all(s.swap_attempts() == reads * every // 2 * nw)
    n = reads * nw
    mean, var = acc_sum / n, acc_sq / n - (acc_sum / n) ** 2
    tol = 0.01 * np.sqrt(2000.0 / reads) / betas
    print("variance x beta per rung:", (var * betas[:, None]).mean(axis=1), "swap rates:", rates)
    assert np.all(np.abs(var - 1.0 / betas[:, None]) < tol[:, None]), (var, tol)
    assert np.all(np.abs(mean) < (0.01 * np.sqrt(2000.0 / reads) / np.sqrt(betas))[:, None]), mean
    assert np.all(rates > 0.0) and np.all(rates < 1.0), rates


# ---- 5. what the feature is for -------------------------------------------------------------------------------------------
MODES = dict(nw=256, d=10.0, G=3000, betas=list(0.05 ** (np.arange(6) / 5.0)))


def two_mode_start(nw, d, k):
    r = np.random.default_rng(k)
    th = r.standard_normal((nw, 4))
    sign = np.where(np.arange(nw) < int(0.9 * nw), 1.0, -1.0)
    r.shuffle(sign)
    th[:, 0] += sign * d / 2
    return th


def test_a_ladder_equalises_two_modes_the_stretch_move_cannot_cross(kmc):
    """The log-sum of two unit Gaussians in 4-D (the target of test_the_mixture_equalises_two_modes), here 10 apart along the first
    axis; 256 walkers, 90 % started in one mode and 10 % in the other; the stretch move; 3 000 generations, 1 500 burned.  The share
    of stored samples in the first mode comes to 1/2 on rung 0 of a ladder of six rungs (betas geometric from 1 to 0.05, a sweep
    after every generation) and stays near where it started without the ladder.

    Bound 0.03.  The numpy yardstick at this size, seeds 1000 .. 1009 (starts 0 .. 9), gave on rung 0 of the ladder
    0.490 0.505 0.504 0.503 0.501 0.503 0.501 0.505 0.504 0.501 -- worst |share - 1/2| = 0.010, a third of the bound -- and
    without the ladder (the same yardstick's rung 0 with no sweeps: the plain stretch sampler, bit for bit)
    0.804 0.805 0.818 0.799 0.793 0.836 0.826 0.812 0.784 0.791 -- every run at least 0.28 from 1/2: all ten miss the bound.
    (At 1 500 generations the ladder's worst was 0.018 and the plain runs stood at 0.83 .. 0.87.)  The device run reproduces the
    yardstick's shares for its seed (0.490 and 0.804), since the device equals the yardstick bit for bit."""
    nw, d, G = MODES["nw"], MODES["d"], MODES["G"]
    th = two_mode_start(nw, d, 0)
    assert np.mean(th[:, 0] > 0) > 0.85
    pdf = kmc.CDensity(TWO_MODES, params=[d / 2])
    shares = {}
    for name, kw in (("untempered", {}), ("tempered", dict(betas=MODES["betas"], swap_every=1))):
        with kmc.Sampler(pdf, nw, 4, G, G // 2, 1, 2.0, 1000, store_chain=True, **kw) as s:
            s.set_positions(th)
            s.run(G)
            s.sync()
            ch, _ = s.chain(logp=False)
            assert ("ntemps 6" in s.describe()) == (name == "tempered")
        shares[name] = float(np.mean(ch[:, :, 0] > 0))
    print("share of the first mode:", shares)
    assert abs(shares["tempered"] - 0.5) < MODES_BOUND, shares
    assert abs(shares["untempered"] - 0.5) >= MODES_BOUND, shares


MODES_BOUND = 0.03


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dtype="f32"), dict(island_gens=8, island_size=64), dict(shard_count=2), dict(p2p=True),
                                dict(deal_rank=0, deal_count=2)])
def test_refusals_are_unsupported_and_name_tempering(kmc, kw):
    with pytest.raises(kmc.KmcError) as e:
        kmc.Sampler(kmc.GaussianIso(), 256, 4, 10, 0, 1, 2.0, 1, betas=[1.0, 0.5], **kw)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED and "tempering" in str(e.value)


def test_host_data_and_blob_densities_and_the_initial_ball_are_refused(kmc, oracle):
    from test_data_density_cpu import REG_TERM
    from test_gpu_data_density import reg_data
    D, _ = reg_data(300, 3, 1)
    blob = kmc.CDensity("blob[0] = x[0]; return -0.5 * x[0] * x[0] - 0.5 * x[1] * x[1];", nblob=1)
    for pdf, nd in ((kmc.HostLogPdf(menu_logpdf(oracle, GAUSS, [0.0, 1.0]), vectorized=True), 3), (kmc.DataDensity(REG_TERM, D, params=[4.0]), 3), (blob, 2)):
        with pytest.raises(kmc.KmcError) as e:
            kmc.Sampler(pdf, 64, nd, 10, 0, 1, 2.0, 1, betas=[1.0, 0.5])
        assert e.value.status == kmc._lib.ERR_UNSUPPORTED and "tempering" in str(e.value)
    with kmc.Sampler(kmc.GaussianIso(), 64, 3, 10, 0, 1, 2.0, 1, betas=[1.0, 0.5]) as s:
        with pytest.raises(kmc.KmcError) as e:
            s.init_ball(np.zeros(3), np.ones(3))
        assert e.value.status == kmc._lib.ERR_UNSUPPORTED and "tempering" in str(e.value)
        import ctypes as C
        z = np.zeros((64, 3))
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        st = s._L.kmc_sampler_set_state(s._h, dp(z), dp(z[:, 0].copy()), None, 0)         # one ensemble: the ladder goes through set_rung_state
        assert st == kmc._lib.ERR_UNSUPPORTED and "tempering" in s._L.kmc_last_error().decode()


@pytest.mark.parametrize("betas,word", [([0.9, 0.5], "betas[0]"), ([1.0, 0.5, 0.5], "decreasing"), ([1.0, 0.0], "> 0"),
                                        ([1.0] + list(0.9 ** np.arange(1, 65)), "ntemps")])
def test_bad_ladders_are_bad_arguments(kmc, betas, word):
    from kissmcmc_jl_amd import _lib
    import ctypes as C
    # (the Python layer checks first; the library's own check is reached through the C ABI)
    with pytest.raises(ValueError):
        kmc.Sampler(kmc.GaussianIso(), 64, 4, 10, 0, 1, 2.0, 1, betas=betas)
    c = _lib.Config()
    c.dtype, c.density = _lib.F64, _lib.GAUSSIAN_ISO
    c.params[0], c.params[1] = 0.0, 1.0
    c.nwalkers, c.ndim, c.ngenerations, c.nburnin, c.nthin, c.a_scale, c.shard_count = 64, 4, 10, 0, 1, 2.0, 1
    keep = (C.c_double * len(betas))(*betas)
    c.betas, c.ntemps = C.cast(keep, C.c_void_p), len(betas)
    h = C.c_void_p()
    st = _lib.lib().kmc_sampler_create(C.byref(c), C.byref(h))
    assert st == _lib.ERR_BAD_ARG and word in _lib.lib().kmc_last_error().decode()


# ---- 7. the reference's call ----------------------------------------------------------------------------------------------
def test_emcee_returns_the_reference_tuple_with_a_ladder(kmc):
    th = np.random.default_rng(2).standard_normal((64, 4))
    thetas, acc, logd, blobs = kmc.emcee(kmc.GaussianIso(), th, niter=64 * 40, use_progress_meter=False, seed=3, betas=[1.0, 0.5, 0.2], swap_every=2)
    assert thetas.shape == (64, 20, 4) and logd.shape == (64, 20) and acc.shape == (64,) and blobs is None
    assert np.all((0.0 <= acc) & (acc <= 1.0))
    t2, a2, l2, _ = kmc.emcee(kmc.GaussianIso(), th, niter=64 * 40, use_progress_meter=False, seed=3, ntemps=3, beta_min=0.2, swap_every=2)
    assert t2.shape == thetas.shape and a2.shape == acc.shape and l2.shape == logd.shape
