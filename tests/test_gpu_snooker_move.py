"""GPU: the snooker move (kmc.DESnookerMove / KMC_MOVE_SNOOKER) and the DE / snooker mixtures (KMC_MOVE_MIX) against their numpy
yardstick (tests/snooker_yardstick.py), bit for bit under DESIGN.md section 6's bar, on every route such a sampler takes (vector and
generic kernels, runtime-compiled, host and data densities), across launch paths; their statistics; their refusals; and the stretch
and DE moves left as they were.  Modelled test for test on tests/test_gpu_de_move.py."""
import numpy as np
import pytest

import de_yardstick as yd
import snooker_yardstick as ys
from test_gpu_de_move import GENERAL_BODY, assert_identical, assert_matches, general_body_host, menu_logpdf

pytestmark = pytest.mark.gpu

GAUSS, ROSEN = 0, 2


def moves(kmc, name):
    """(the library's move, the yardstick's)"""
    if name == "snooker":
        return kmc.DESnookerMove(), ys.Snooker()
    if name == "mix":
        return [(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)], [(ys.DE(), 0.8), (ys.Snooker(), 0.2)]
    raise ValueError(name)


TAG = {"snooker": "KMC_MOVE_SNOOKER", "mix": "KMC_MOVE_MIX"}


def run(kmc, pdf, th, G, nburn=0, nthin=1, seed=11, move=None, half_steps=False, **kw):
    nw, nd = th.shape
    with kmc.Sampler(pdf, nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, moments=True, move=move, **kw) as s:
        s.set_positions(th)
        if half_steps:
            for _ in range(G):
                s.half_step(0)
                s.half_step(1)
        else:
            s.run(G // 2)
            s.run(G - G // 2)
        s.sync()
        ch, cl = s.chain()
        m = s.moments()
        return dict(pos=s.positions(), logp=s.logp(), nacc=s.naccept(), chain=ch, chain_logp=cl, sum=m[0], sumsq=m[1], n=m[2],
                    desc=s.describe())


@pytest.mark.parametrize("mv", ["snooker", "mix"])
@pytest.mark.parametrize("dens,params,nw,nd,G,kernel", [
    (GAUSS, [0.0, 1.0], 64, 4, 40, None),
    (ROSEN, [1.0, 100.0, 20.0], 128, 32, 30, "vec"),
    (GAUSS, [0.3, 1.5], 96, 5, 30, "vec"),
    (GAUSS, [0.0, 1.0], 256, 33, 20, "vec"),
    (GAUSS, [0.0, 1.0], 1104, 1100, 6, "generic"),
], ids=["gauss64x4", "rosen128x32", "ragged5", "ragged33", "ndim1100"])
def test_menu_densities_match_the_yardstick(kmc, oracle, mv, dens, params, nw, nd, G, kernel):
    th = np.random.default_rng(nd).standard_normal((nw, nd)) * 0.5 + (1.0 if dens == ROSEN else 0.0)
    pdf = kmc.GaussianIso(*params) if dens == GAUSS else kmc.Rosenbrock(*params)
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, pdf, th, G, nburn=G // 3, nthin=2, seed=5, move=lib_move)
    name = {"snooker": "half_step_snooker_", "mix": "half_step_mix_"}[mv]
    assert TAG[mv] in got["desc"] and (kernel is None or name + kernel in got["desc"]), got["desc"]
    want = ys.emcee_moves(menu_logpdf(oracle, dens, params), th, G, G // 3, 2, seed=5, move=y_move)
    if mv == "mix":
        assert 0 < np.sum(want["members"] == 1) < len(want["members"])          # both members were used
    assert_matches(got, want)
    assert 0 < got["nacc"].sum() < nw * (G - G // 3)


@pytest.mark.parametrize("plan", ["generic", "4,1,1", "8,2,1", "16,2,2", "64,2,1"])
def test_the_sums_do_not_depend_on_the_geometry(kmc, oracle, monkeypatch, plan):
    """The reduction order T is a function of ndim alone: a forced geometry (KMC_PLAN: L, K, ITER; or the one-walker-per-lane kernel)
    gives the bits the yardstick gives, at a ragged row length."""
    nw, nd, G = 128, 5 if plan in ("generic", "4,1,1") else 29, 12
    th = np.random.default_rng(41).standard_normal((nw, nd))
    monkeypatch.setenv("KMC_PLAN", plan)
    got = run(kmc, kmc.GaussianIso(), th, G, nburn=2, seed=15, move=kmc.DESnookerMove())
    monkeypatch.delenv("KMC_PLAN")
    want = ys.emcee_moves(menu_logpdf(oracle, GAUSS, [0.0, 1.0]), th, G, 2, 1, seed=15, move=ys.Snooker())
    assert_matches(got, want)


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_expr_density_matches_the_yardstick(kmc, oracle, mv):
    nw, nd, G = 256, 16, 24
    th = np.random.default_rng(3).standard_normal((nw, nd))
    pdf = kmc.ExprDensity("-0.5*((x-p[0])*p[1])*((x-p[0])*p[1])", params=[0.25, 1.0 / 1.5])
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, pdf, th, G, nburn=4, nthin=1, seed=8, move=lib_move)
    assert {"snooker": "half_step_snooker_vec", "mix": "half_step_mix_vec"}[mv] in got["desc"], got["desc"]
    f = lambda X: np.array([sum(-0.5 * ((x - 0.25) * (1.0 / 1.5)) * ((x - 0.25) * (1.0 / 1.5)) for x in row) for row in X])
    assert_matches(got, ys.emcee_moves(f, th, G, 4, 1, seed=8, move=y_move))


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_general_body_matches_the_yardstick(kmc, mv):
    nw, nd, G = 192, 6, 24
    th = np.random.default_rng(4).standard_normal((nw, nd))
    pdf = kmc.CDensity(GENERAL_BODY, params=[4.0])
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, pdf, th, G, nburn=6, nthin=3, seed=21, move=lib_move)
    assert TAG[mv] in got["desc"], got["desc"]
    assert_matches(got, ys.emcee_moves(lambda X: general_body_host(X, 4.0), th, G, 6, 3, seed=21, move=y_move))


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_host_logpdf_matches_the_yardstick(kmc, oracle, mv):
    nw, nd, G = 128, 3, 20
    th = np.random.default_rng(6).standard_normal((nw, nd))
    f = menu_logpdf(oracle, GAUSS, [0.0, 2.0])
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, kmc.HostLogPdf(f, vectorized=True), th, G, nburn=5, nthin=1, seed=2, move=lib_move)
    assert {"snooker": "half_step_snooker_generic", "mix": "half_step_mix_generic"}[mv] in got["desc"], got["desc"]
    assert_matches(got, ys.emcee_moves(f, th, G, 5, 1, seed=2, move=y_move))


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_data_density_matches_the_yardstick(kmc, mv):
    from test_data_density_cpu import REG_TERM, pairwise
    from test_gpu_data_density import reg_data, reg_terms
    D, beta = reg_data(3000, 3, 1)
    nw, nd, G = 64, 3, 16
    th = beta + 0.1 * np.random.default_rng(7).standard_normal((nw, nd))
    pdf = kmc.DataDensity(REG_TERM, D, params=[4.0])
    lib_move, y_move = moves(kmc, mv)
    got = run(kmc, pdf, th, G, nburn=4, seed=13, move=lib_move)
    assert "data density" in got["desc"] and TAG[mv] in got["desc"], got["desc"]
    assert_matches(got, ys.emcee_moves(lambda X: pairwise(reg_terms(np.asarray(X), D, 4.0)), th, G, 4, 1, seed=13, move=y_move))


@pytest.fixture
def c2ish():
    return np.random.default_rng(0).standard_normal((8192, 32))


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_launch_paths_agree(kmc, monkeypatch, c2ish, mv):
    res = {}
    for mode in ("graph", "eager", "updated"):
        monkeypatch.setenv("KMC_LAUNCH", mode)
        res[mode] = run(kmc, kmc.GaussianIso(), c2ish, 70, nburn=10, seed=3, move=moves(kmc, mv)[0])
    monkeypatch.delenv("KMC_LAUNCH")
    assert {"snooker": "half_step_snooker_vec", "mix": "half_step_mix_vec"}[mv] in res["graph"]["desc"]
    assert_identical(res["graph"], res["eager"])
    assert_identical(res["graph"], res["updated"])


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_half_steps_equal_run(kmc, c2ish, mv):
    th = c2ish[:1024]
    a = run(kmc, kmc.GaussianIso(), th, 20, nburn=5, seed=4, move=moves(kmc, mv)[0])
    b = run(kmc, kmc.GaussianIso(), th, 20, nburn=5, seed=4, move=moves(kmc, mv)[0], half_steps=True)
    assert_identical(a, b)


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_state_restore_resumes_bit_for_bit(kmc, c2ish, mv):
    th = c2ish[:2048]
    G, cut, seed = 30, 12, 9
    if mv == "mix":     # the resume crosses a point where the mixture switches member (the choice is a function of (seed, step) alone)
        members = ys.mix_choices(seed, np.arange(2 * G), ys.mix_weights([0.8, 0.2])[1])
        assert len(set(members[:2 * cut])) == 2 and len(set(members[2 * cut:])) == 2, members
    mk = lambda: kmc.Sampler(kmc.GaussianIso(), 2048, 32, G, 0, 1, 2.0, seed, move=moves(kmc, mv)[0])
    with mk() as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        want = s.positions(), s.logp(), s.naccept()
    with mk() as s:
        s.set_positions(th)
        s.run(cut)
        st = s.state()
    with mk() as s:
        s.restore(st)
        s.run(G - cut)
        s.sync()
        got = s.positions(), s.logp(), s.naccept()
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_stream_chain_and_by_walker_equal_the_device_chain(kmc, c2ish, mv):
    th = c2ish[:1024]
    G = 40
    dev = run(kmc, kmc.GaussianIso(), th, G, nburn=8, nthin=2, seed=6, move=moves(kmc, mv)[0])
    with kmc.Sampler(kmc.GaussianIso(), 1024, 32, G, 8, 2, 2.0, 6, store_chain=True, store_logp=True, stream_chain=True,
                     move=moves(kmc, mv)[0]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        ch, cl = s.chain()
    np.testing.assert_array_equal(ch, dev["chain"])
    np.testing.assert_array_equal(cl, dev["chain_logp"])
    with kmc.Sampler(kmc.GaussianIso(), 1024, 32, G, 8, 2, 2.0, 6, store_chain=True, store_logp=True, move=moves(kmc, mv)[0]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        bw, bl = s.chain(by_walker=True)
    np.testing.assert_array_equal(bw, dev["chain"].transpose(1, 0, 2))
    np.testing.assert_array_equal(bl, dev["chain_logp"].T)


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_stationary_variance_of_the_unit_gaussian(kmc, mv):
    nw, nd, G = 4096, 8, 2000
    th = np.random.default_rng(12).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, 0, 1, 2.0, 17, moments=True, move=moves(kmc, mv)[0]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        msum, msq, n = s.moments()
        acc = s.naccept().sum() / (nw * G)
    mean, var = msum / n, msq / n - (msum / n) ** 2
    assert np.all(np.abs(mean) < 0.01) and np.all(np.abs(var - 1.0) < 0.01), (mean, var)
    assert 0.2 < acc < 0.6


@pytest.mark.parametrize("mv", ["snooker", "mix"])
@pytest.mark.parametrize("kw", [dict(dtype="f32"), dict(island_gens=8, island_size=64), dict(shard_count=2)])
def test_refusals_are_unsupported_and_name_the_move(kmc, mv, kw):
    with pytest.raises(kmc.KmcError) as e:
        kmc.Sampler(kmc.GaussianIso(), 256, 4, 10, 0, 1, 2.0, 1, move=moves(kmc, mv)[0], **kw)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED and TAG[mv] in str(e.value)


@pytest.mark.parametrize("mv", ["snooker", "mix"])
def test_device_blobs_are_refused(kmc, mv):
    pdf = kmc.CDensity("blob[0] = x[0]; return -0.5 * x[0] * x[0] - 0.5 * x[1] * x[1];", nblob=1)
    with pytest.raises(kmc.KmcError) as e:
        kmc.Sampler(pdf, 64, 2, 10, 0, 1, 2.0, 1, move=moves(kmc, mv)[0], store_chain=True, store_blobs=True)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED and TAG[mv] in str(e.value)


def test_one_dimension_and_a_stretch_member_are_refused(kmc):
    with pytest.raises(kmc.KmcError) as e:
        kmc.Sampler(kmc.GaussianIso(), 64, 1, 10, 0, 1, 2.0, 1, move=kmc.DESnookerMove())
    assert e.value.status == kmc._lib.ERR_BAD_ARG and "KMC_MOVE_SNOOKER" in str(e.value)
    with pytest.raises(ValueError, match="stretch"):
        kmc.Sampler(kmc.GaussianIso(), 64, 4, 10, 0, 1, 2.0, 1, move=[(None, 0.5), (kmc.DESnookerMove(), 0.5)])


def test_a_mixture_with_all_weight_on_de_is_the_de_move(kmc, c2ish):
    for th in (c2ish[:256, :5], c2ish[:4096]):
        a = run(kmc, kmc.GaussianIso(), th, 24, nburn=4, seed=23, move=kmc.DEMove())
        b = run(kmc, kmc.GaussianIso(), th, 24, nburn=4, seed=23, move=[(kmc.DEMove(), 1.0), (kmc.DESnookerMove(), 1e-300)])
        assert "KMC_MOVE_MIX" in b["desc"] and "KMC_MOVE_DE" in a["desc"]
        assert_identical(a, b)


def test_emcee_returns_the_reference_tuple_with_a_mixture(kmc):
    th = np.random.default_rng(2).standard_normal((64, 4))
    out = kmc.emcee(kmc.GaussianIso(), th, niter=64 * 40, use_progress_meter=False, seed=3, move=[(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)])
    thetas, acc, logd, blobs = out
    assert len(thetas) == 64 and len(logd) == 64 and len(acc) == 64
    assert all(len(t) == len(thetas[0]) > 0 for t in thetas) and all(0.0 <= a <= 1.0 for a in acc)


TWO_MODES = ("double a = 0.0, b = 0.0; for (int i = 0; i < n; ++i) { const double m = (i == 0) ? p[0] : 0.0; a += (x[i] - m) * (x[i] - m); "
             "b += (x[i] + m) * (x[i] + m); } a = -0.5 * a; b = -0.5 * b; const double mx = a > b ? a : b; return mx + log(exp(a - mx) + exp(b - mx));")


def test_the_mixture_equalises_two_modes(kmc):
    """The log-sum of two unit Gaussians in 4-D, 6 apart along the first axis; 256 walkers, 90 % started in one mode and 10 % in the
    other; 1 500 generations, 750 burned.  The share of stored samples in the first mode comes to 1/2 under the 0.8 / 0.2 mixture.

    Bound 0.03.  The numpy yardstick at this size, seeds 1000 .. 1009 (starts 0 .. 9), gave shares
    0.506 0.506 0.497 0.495 0.504 0.496 0.504 0.507 0.496 0.505 -- worst |share - 1/2| = 0.007, under half the bound.
    (At 4 and 5 apart with 400 and 800 generations the worst seeds were 0.013 and 0.012.  Snooker alone: worst 0.031 at 6 apart.)
    No contrast with the stretch move is asserted: the yardstick restates DE and snooker only, so it says nothing about where
    the stretch move stands at this size."""
    nw, d, G = 256, 6.0, 1500
    r = np.random.default_rng(0)
    th = r.standard_normal((nw, 4))
    sign = np.where(np.arange(nw) < int(0.9 * nw), 1.0, -1.0)
    r.shuffle(sign)
    th[:, 0] += sign * d / 2
    assert np.mean(th[:, 0] > 0) > 0.85
    pdf = kmc.CDensity(TWO_MODES, params=[d / 2])
    with kmc.Sampler(pdf, nw, 4, G, G // 2, 1, 2.0, 1000, store_chain=True, move=[(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)]) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        ch, _ = s.chain(logp=False)
        assert "KMC_MOVE_MIX" in s.describe()
    share = float(np.mean(ch[:, :, 0] > 0))
    print("share of the first mode:", share)
    assert abs(share - 0.5) < 0.03, share


def test_stretch_and_de_are_what_they_were(kmc, c2ish, oracle):
    """move=None twice and against an omitted move=, and DEMove twice and against its own yardstick: the new enum values change neither."""
    for th in (c2ish[:256, :4], c2ish[:4096]):
        nw, nd = th.shape
        outs = []
        for kw in ({}, dict(move=None), dict(move=None)):
            with kmc.Sampler(kmc.GaussianIso(), nw, nd, 30, 5, 1, 2.0, 19, store_chain=True, store_logp=True, moments=True, **kw) as s:
                s.set_positions(th)
                s.run(30)
                s.sync()
                ch, cl = s.chain()
                outs.append((s.positions(), s.logp(), s.naccept(), ch, cl, *s.moments(), s.describe()))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                if isinstance(a, np.ndarray):
                    np.testing.assert_array_equal(a, b)
                else:
                    assert a == b
        assert "KMC_MOVE" not in outs[0][-1]
    th = c2ish[:256, :6]
    a = run(kmc, kmc.GaussianIso(), th, 20, nburn=4, seed=29, move=kmc.DEMove())
    b = run(kmc, kmc.GaussianIso(), th, 20, nburn=4, seed=29, move=kmc.DEMove())
    assert_identical(a, b)
    assert_matches(a, yd.emcee_de(menu_logpdf(oracle, GAUSS, [0.0, 1.0]), th, 20, 4, 1, seed=29))
