"""GPU: the differential-evolution move (kmc.DEMove / KMC_MOVE_DE) against its numpy yardstick (tests/de_yardstick.py), bit for bit
under DESIGN.md section 6's bar, on every route a DE sampler takes (vector and generic kernels, runtime-compiled, host and data
densities), across launch paths; its statistics and mixing; its refusals; and the default left as it was."""
import math

import numpy as np
import pytest

import de_yardstick as yd
import refcases

pytestmark = pytest.mark.gpu

GAUSS, ROSEN = 0, 2


def run(kmc, pdf, th, G, nburn=0, nthin=1, seed=11, move="de", half_steps=False, **kw):
    nw, nd = th.shape
    mv = kmc.DEMove() if move == "de" else move
    with kmc.Sampler(pdf, nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, moments=True, move=mv, **kw) as s:
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


def menu_logpdf(oracle, dens, params):
    return lambda X: oracle.logpdf_batch(dens, params, X)


def assert_matches(got, want):
    """decisions, counters, positions and chains identical; log-pdfs to 1e-12, moments to 1e-11."""
    np.testing.assert_array_equal(got["nacc"], want["nacc"])
    np.testing.assert_array_equal(got["pos"], want["pos"])
    np.testing.assert_array_equal(got["chain"], want["chain"])
    tol = lambda a: 1e-12 * np.maximum(1.0, np.abs(a))
    assert np.all(np.abs(got["logp"] - want["logp"]) <= tol(want["logp"]))
    assert np.all(np.abs(got["chain_logp"] - want["chain_logp"]) <= tol(want["chain_logp"]))
    assert got["n"] == want["n"]
    np.testing.assert_allclose(got["sum"], want["sum"], rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(got["sumsq"], want["sumsq"], rtol=1e-11, atol=1e-9)


def assert_identical(a, b):
    for k in ("nacc", "pos", "logp", "chain", "chain_logp", "sum", "sumsq"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["n"] == b["n"]


@pytest.mark.parametrize("dens,params,nw,nd,G,kernel", [
    (GAUSS, [0.0, 1.0], 64, 4, 40, None),
    (ROSEN, [1.0, 100.0, 20.0], 128, 32, 30, "half_step_de_vec"),
    (GAUSS, [0.3, 1.5], 96, 5, 30, "half_step_de_vec"),
    (GAUSS, [0.0, 1.0], 256, 33, 20, "half_step_de_vec"),
    (GAUSS, [0.0, 1.0], 1104, 1100, 6, "half_step_de_generic"),
], ids=["gauss64x4", "rosen128x32", "ragged5", "ragged33", "ndim1100"])
def test_menu_densities_match_the_yardstick(kmc, oracle, dens, params, nw, nd, G, kernel):
    th = np.random.default_rng(nd).standard_normal((nw, nd)) * 0.5 + (1.0 if dens == ROSEN else 0.0)
    pdf = kmc.GaussianIso(*params) if dens == GAUSS else kmc.Rosenbrock(*params)
    got = run(kmc, pdf, th, G, nburn=G // 3, nthin=2, seed=5)
    assert "KMC_MOVE_DE" in got["desc"] and (kernel is None or kernel in got["desc"]), got["desc"]
    want = yd.emcee_de(menu_logpdf(oracle, dens, params), th, G, G // 3, 2, seed=5)
    assert_matches(got, want)
    assert 0 < got["nacc"].sum() < nw * (G - G // 3)


def test_expr_density_matches_the_yardstick(kmc, oracle):
    nw, nd, G = 256, 16, 24
    th = np.random.default_rng(3).standard_normal((nw, nd))
    pdf = kmc.ExprDensity("-0.5*((x-p[0])*p[1])*((x-p[0])*p[1])", params=[0.25, 1.0 / 1.5])
    got = run(kmc, pdf, th, G, nburn=4, nthin=1, seed=8)
    assert "half_step_de_vec" in got["desc"], got["desc"]
    # the yardstick evaluates the same expression element by element in index order (the vector kernel sums by a tree: to rounding)
    f = lambda X: np.array([sum(-0.5 * ((x - 0.25) * (1.0 / 1.5)) * ((x - 0.25) * (1.0 / 1.5)) for x in row) for row in X])
    want = yd.emcee_de(f, th, G, 4, 1, seed=8)
    assert_matches(got, want)


GENERAL_BODY = ("double m = 0.0; for (int i = 0; i < n; ++i) m += x[i]; m = m / n; double s = 0.0; "
                "for (int i = 0; i < n; ++i) { double t = x[i] - m; s += t * t; } return -0.5 * s - 0.5 * p[0] * m * m;")


def general_body_host(X, p0):
    out = np.empty(X.shape[0])
    for r, x in enumerate(X):
        n = len(x)
        m = 0.0
        for v in x:
            m += v
        m = m / n
        s = 0.0
        for v in x:
            t = v - m
            s += t * t
        out[r] = -0.5 * s - 0.5 * p0 * m * m
    return out


def test_general_body_matches_the_yardstick(kmc):
    nw, nd, G = 192, 6, 24
    th = np.random.default_rng(4).standard_normal((nw, nd))
    pdf = kmc.CDensity(GENERAL_BODY, params=[4.0])
    got = run(kmc, pdf, th, G, nburn=6, nthin=3, seed=21)
    assert "KMC_MOVE_DE" in got["desc"], got["desc"]
    want = yd.emcee_de(lambda X: general_body_host(X, 4.0), th, G, 6, 3, seed=21)
    assert_matches(got, want)


def test_host_logpdf_matches_the_yardstick(kmc, oracle):
    nw, nd, G = 128, 3, 20
    th = np.random.default_rng(6).standard_normal((nw, nd))
    f = menu_logpdf(oracle, GAUSS, [0.0, 2.0])
    got = run(kmc, kmc.HostLogPdf(f, vectorized=True), th, G, nburn=5, nthin=1, seed=2)
    assert "half_step_de_generic" in got["desc"], got["desc"]
    assert_matches(got, yd.emcee_de(f, th, G, 5, 1, seed=2))


def test_data_density_matches_the_yardstick(kmc):
    from test_data_density_cpu import REG_TERM, pairwise
    from test_gpu_data_density import reg_data, reg_terms
    D, beta = reg_data(3000, 3, 1)
    nw, nd, G = 64, 3, 16
    th = beta + 0.1 * np.random.default_rng(7).standard_normal((nw, nd))
    pdf = kmc.DataDensity(REG_TERM, D, params=[4.0])
    got = run(kmc, pdf, th, G, nburn=4, seed=13)
    assert "data density" in got["desc"] and "KMC_MOVE_DE" in got["desc"], got["desc"]
    want = yd.emcee_de(lambda X: pairwise(reg_terms(np.asarray(X), D, 4.0)), th, G, 4, 1, seed=13)
    assert_matches(got, want)


@pytest.fixture
def c2ish():
    return np.random.default_rng(0).standard_normal((8192, 32))


def test_launch_paths_agree(kmc, monkeypatch, c2ish):
    res = {}
    for mode in ("graph", "eager", "updated"):
        monkeypatch.setenv("KMC_LAUNCH", mode)
        res[mode] = run(kmc, kmc.GaussianIso(), c2ish, 70, nburn=10, seed=3)
    monkeypatch.delenv("KMC_LAUNCH")
    assert "half_step_de_vec" in res["graph"]["desc"]
    assert_identical(res["graph"], res["eager"])
    assert_identical(res["graph"], res["updated"])


def test_half_steps_equal_run(kmc, c2ish):
    th = c2ish[:1024]
    a = run(kmc, kmc.GaussianIso(), th, 20, nburn=5, seed=4)
    b = run(kmc, kmc.GaussianIso(), th, 20, nburn=5, seed=4, half_steps=True)
    assert_identical(a, b)


def test_state_restore_resumes_bit_for_bit(kmc, c2ish):
    th = c2ish[:2048]
    G = 30
    with kmc.Sampler(kmc.GaussianIso(), 2048, 32, G, 0, 1, 2.0, 9, move=kmc.DEMove()) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        want = s.positions(), s.logp(), s.naccept()
    with kmc.Sampler(kmc.GaussianIso(), 2048, 32, G, 0, 1, 2.0, 9, move=kmc.DEMove()) as s:
        s.set_positions(th)
        s.run(12)
        st = s.state()
    with kmc.Sampler(kmc.GaussianIso(), 2048, 32, G, 0, 1, 2.0, 9, move=kmc.DEMove()) as s:
        s.restore(st)
        s.run(G - 12)
        s.sync()
        got = s.positions(), s.logp(), s.naccept()
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_stream_chain_and_by_walker_equal_the_device_chain(kmc, c2ish):
    th = c2ish[:1024]
    G = 40
    dev = run(kmc, kmc.GaussianIso(), th, G, nburn=8, nthin=2, seed=6)
    with kmc.Sampler(kmc.GaussianIso(), 1024, 32, G, 8, 2, 2.0, 6, store_chain=True, store_logp=True, stream_chain=True,
                     move=kmc.DEMove()) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        ch, cl = s.chain()
    np.testing.assert_array_equal(ch, dev["chain"])
    np.testing.assert_array_equal(cl, dev["chain_logp"])
    with kmc.Sampler(kmc.GaussianIso(), 1024, 32, G, 8, 2, 2.0, 6, store_chain=True, store_logp=True, move=kmc.DEMove()) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        bw, bl = s.chain(by_walker=True)
    np.testing.assert_array_equal(bw, dev["chain"].transpose(1, 0, 2))
    np.testing.assert_array_equal(bl, dev["chain_logp"].T)


def test_stationary_variance_of_the_unit_gaussian(kmc):
    nw, nd, G = 4096, 8, 2000
    th = np.random.default_rng(12).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, 0, 1, 2.0, 17, moments=True, move=kmc.DEMove()) as s:
        s.set_positions(th)
        s.run(G)
        s.sync()
        msum, msq, n = s.moments()
        acc = s.naccept().sum() / (nw * G)
    mean, var = msum / n, msq / n - (msum / n) ** 2
    assert np.all(np.abs(mean) < 0.01) and np.all(np.abs(var - 1.0) < 0.01), (mean, var)
    assert 0.2 < acc < 0.6


def test_reference_rosenbrock_case_with_de(kmc):
    case = next(c for c in refcases.CASES if c["name"] == "rosenbrock2")
    pdf = kmc.Rosenbrock(*case["params"])
    nw, niter = refcases.NWALKERS, case["niter"]
    theta0s = kmc.make_theta0s(case["theta0"], refcases.BALL_RADIUS, pdf, nw, rng=42)
    samples = kmc.emcee(pdf, theta0s, niter=niter, use_progress_meter=False, seed=4242, move=kmc.DEMove())
    thetas, accept_ratio, logdensities, blobs = kmc.squash_walkers(*samples, verbose=False)
    # (the reference pins the stretch move's acceptance above 0.1 here; DE's on this banana with the Gaussian-optimal gamma0 measured 0.035)
    assert accept_ratio > 0.02
    refcases.check_mean_std(thetas, case)


def test_de_mixes_at_least_twice_as_fast_as_stretch_in_32_dims(kmc):
    """Seeded: 256 walkers on the 32-D unit Gaussian, 6 000 generations, 1 000 burned; median tau_int of DE <= 0.5 x stretch's
    (the numpy estimate of the issue: 0.28)."""
    nw, nd, G, nb = 256, 32, 6000, 1000
    th = np.random.default_rng(31).standard_normal((nw, nd))
    taus = {}
    for name, mv in (("stretch", None), ("de", kmc.DEMove())):
        with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, nb, 1, 2.0, 77, store_chain=True, move=mv) as s:
            s.set_positions(th)
            s.run(G)
            s.sync()
            ch, _ = s.chain(logp=False, by_walker=True)
        tau, _ = kmc.int_acorr(ch, warn=False)
        taus[name] = float(np.median(tau))
    assert taus["de"] <= 0.5 * taus["stretch"], taus


@pytest.mark.parametrize("kw", [dict(dtype="f32"), dict(island_gens=8, island_size=64), dict(shard_count=2)])
def test_refusals_are_unsupported_and_name_the_move(kmc, kw):
    with pytest.raises(kmc.KmcError) as e:
        kmc.Sampler(kmc.GaussianIso(), 256, 4, 10, 0, 1, 2.0, 1, move=kmc.DEMove(), **kw)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED and "KMC_MOVE_DE" in str(e.value)


def test_device_blobs_are_refused_with_de(kmc):
    pdf = kmc.CDensity("blob[0] = x[0]; return -0.5 * x[0] * x[0];", nblob=1)
    with pytest.raises(kmc.KmcError) as e:
        kmc.Sampler(pdf, 64, 1, 10, 0, 1, 2.0, 1, move=kmc.DEMove(), store_chain=True, store_blobs=True)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED and "KMC_MOVE_DE" in str(e.value)


def test_host_callable_blobs_keep_working_with_de(kmc):
    def f(x):
        return -0.5 * float(np.dot(x, x)), float(x[0])
    th = np.random.default_rng(2).standard_normal((32, 2))
    thetas, acc, logd, blobs = kmc.emcee(f, th, niter=32 * 40, hasblob=True, use_progress_meter=False, seed=3, move=kmc.DEMove())
    assert len(blobs) == 32 and all(len(b) == len(thetas[0]) for b in blobs)
    assert all(b == t[0] for w in range(32) for b, t in zip(blobs[w], thetas[w]))


def test_move_none_is_the_default(kmc, c2ish):
    for th in (c2ish[:256, :4], c2ish[:4096]):
        nw, nd = th.shape
        outs = []
        for kw in ({}, dict(move=None)):
            with kmc.Sampler(kmc.GaussianIso(), nw, nd, 30, 5, 1, 2.0, 19, store_chain=True, store_logp=True, moments=True, **kw) as s:
                s.set_positions(th)
                s.run(30)
                s.sync()
                ch, cl = s.chain()
                outs.append((s.positions(), s.logp(), s.naccept(), ch, cl, *s.moments(), s.describe()))
        for a, b in zip(*outs):
            if isinstance(a, np.ndarray):
                np.testing.assert_array_equal(a, b)
            else:
                assert a == b
        assert "KMC_MOVE_DE" not in outs[0][-1]
