"""GPU: data densities (kmc.DataDensity / KMC_DATA_DENSITY) -- a log-prior plus per-observation terms summed over a dataset on the
device.  The yardstick is the host route (HostLogPdf(vectorized=True), itself bit-identical to the oracle, test_gpu_hostdensity.py)
with the numpy restatement of the value contract as its callable: terms in the body's operation order, then the pairwise tree."""
import numpy as np
import pytest

from test_data_density_cpu import REG_TERM, pairwise

pytestmark = pytest.mark.gpu

POISSON_TERM = "double eta = x[0] + x[1] * d[0]; return d[1] * eta - exp(eta);"


def reg_terms(X, D, p0):
    """REG_TERM for every (row, observation): x[0] + sum_k x[k] d[k-1] in order, residual against d[n-1]."""
    n = X.shape[1]
    mu = np.repeat(X[:, 0:1], D.shape[0], axis=1)
    for k in range(1, n):
        mu = mu + X[:, k:k + 1] * D[None, :, k - 1]
    r = D[None, :, n - 1] - mu
    return -0.5 * p0 * r * r


def reg_data(ndata, nd, seed):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((ndata, nd - 1))
    beta = np.linspace(0.5, -0.5, nd)
    y = beta[0] + Z @ beta[1:] + 0.5 * rng.standard_normal(ndata)
    return np.column_stack([Z, y]), beta


def host_yardstick(kmc, term_fn, prior_fn=None):
    def f(X):
        X = np.asarray(X, dtype=np.float64)
        lp = pairwise(term_fn(X))
        if prior_fn is not None:
            pr = prior_fn(X)
            lp = np.where(pr == -np.inf, -np.inf, pr + lp)
        return lp
    return kmc.HostLogPdf(f, vectorized=True)


def run(kmc, pdf, th, G, nburn=0, nthin=1, seed=11, **kw):
    nw, nd = th.shape
    with kmc.Sampler(pdf, nw, nd, G, nburn, nthin, 2.0, seed, store_chain=True, store_logp=True, moments=True, **kw) as s:
        s.set_positions(th)
        s.run(G // 2)
        s.run(G - G // 2)
        s.sync()
        desc = s.describe()
        ch, cl = s.chain()
        m = s.moments()
        return dict(pos=s.positions(), logp=s.logp(), nacc=s.naccept(), chain=ch, chain_logp=cl, sum=m[0], sumsq=m[1], n=m[2], desc=desc,
                    mode=s.launch_mode(), launches=s.launch_count)


def assert_same(got, want, moments=True):
    np.testing.assert_array_equal(got["nacc"], want["nacc"])
    np.testing.assert_array_equal(got["pos"], want["pos"])
    np.testing.assert_array_equal(got["logp"], want["logp"])
    np.testing.assert_array_equal(got["chain"], want["chain"])
    np.testing.assert_array_equal(got["chain_logp"], want["chain_logp"])
    if moments:
        assert got["n"] == want["n"]
        np.testing.assert_allclose(got["sum"], want["sum"], rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(got["sumsq"], want["sumsq"], rtol=1e-11, atol=1e-11)


SHAPES = [(100, 3, 1000), (256, 8, 4096), (256, 8, 4097), (2050, 5, 257), (64, 2, 1)]


@pytest.mark.parametrize("nw,nd,ndata", SHAPES)
def test_regression_is_bit_identical_to_the_host_route(kmc, nw, nd, ndata):
    D, beta = reg_data(ndata, nd, nw + ndata)
    p0 = 4.0
    dd = kmc.DataDensity(REG_TERM, D, params=[p0])
    host = host_yardstick(kmc, lambda X: reg_terms(X, D, p0))
    th = beta + 0.05 * np.random.default_rng(nd).standard_normal((nw, nd))
    G = 30
    got, want = run(kmc, dd, th, G, 5, 2), run(kmc, host, th, G, 5, 2)
    assert "data density" in got["desc"]
    assert got["mode"] == want["mode"]            # reported as the host route is
    assert got["launches"] == 8 * G               # per half-step: PROPOSE, partial sums, fold, ACCEPT
    assert_same(got, want)
    assert got["nacc"].sum() > 0
    # the stateless evaluation (make_theta0s' pdf(theta)) is the same value as the sampler's
    np.testing.assert_array_equal(dd.finite_rows(got["pos"]), np.isfinite(got["logp"]))
    np.testing.assert_array_equal(dd._eval_rows(got["pos"]), got["logp"])


@pytest.mark.parametrize("nw,nd,ndata", [(100, 3, 1000), (2050, 5, 257)])
def test_both_mappings_give_identical_results(kmc, kmc_debug, nw, nd, ndata):
    D, beta = reg_data(ndata, nd, 3)
    dd = kmc.DataDensity(REG_TERM, D, params=[2.0])
    th = beta + 0.05 * np.random.default_rng(1).standard_normal((nw, nd))
    out = {}
    for m in ("lane", "obs"):
        kmc_debug.set("data-map", m)
        out[m] = run(kmc, dd, th, 20, 2, 1)
        assert ("data_partial_lane" if m == "lane" else "data_partial_obs") in out[m]["desc"]
    assert_same(out["lane"], out["obs"])


def test_many_rounds_per_wave_and_a_ragged_last_chunk(kmc, kmc_debug):
    """4 096 x 4 over 20 001 observations: the lane mapping runs 8 chunks of 16 per wave (the binary-counter stack over chunks, a last block
    of 33 observations: two whole chunks and one of a single row), the observation-per-lane mapping forced runs 128 rounds of 64 per wave."""
    nw, nd, ndata = 4096, 4, 20001
    D, beta = reg_data(ndata, nd, 31)
    dd = kmc.DataDensity(REG_TERM, D, params=[4.0])
    th = beta + 0.05 * np.random.default_rng(4).standard_normal((nw, nd))
    want = run(kmc, host_yardstick(kmc, lambda X: reg_terms(X, D, 4.0)), th, 4, 1, 1)
    lane = run(kmc, dd, th, 4, 1, 1)
    assert "data_partial_lane" in lane["desc"] and "8 rounds per wave" in lane["desc"]
    assert_same(lane, want)
    kmc_debug.set("data-map", "obs")
    obs = run(kmc, dd, th, 4, 1, 1)
    assert "data_partial_obs" in obs["desc"] and "128 rounds per wave" in obs["desc"]
    assert_same(obs, want)


def test_mapping_switch_after_creation_keeps_the_sampler_s_plan(kmc, kmc_debug):
    """KMC_DEBUG=data-map is read when a sampler is created; changing it afterwards changes nothing about that sampler (its scratch
    buffer is sized for the plan it was created with)."""
    D, beta = reg_data(1000, 3, 5)
    dd = kmc.DataDensity(REG_TERM, D, params=[2.0])
    th = beta + 0.05 * np.random.default_rng(6).standard_normal((100, 3))
    ref = run(kmc, dd, th, 20, 2, 1)
    kmc_debug.set("data-map", "obs")
    with kmc.Sampler(dd, 100, 3, 20, 2, 1, 2.0, 11, store_chain=True, store_logp=True, moments=True) as s:
        kmc_debug.set("data-map", "lane")                    # (lane would need 16 blocks x 50 proposals of scratch; obs was sized for 4 x 100)
        s.set_positions(th)
        s.run(20)
        s.sync()
        assert "data_partial_obs" in s.describe()
        ch, cl = s.chain()
        np.testing.assert_array_equal(ch, ref["chain"])
        np.testing.assert_array_equal(cl, ref["chain_logp"])
        np.testing.assert_array_equal(s.naccept(), ref["nacc"])


def test_transcendental_terms_match_to_rounding(kmc):
    rng = np.random.default_rng(7)
    t = rng.uniform(-1, 1, 3000)
    y = rng.poisson(np.exp(0.3 + 0.8 * t)).astype(np.float64)
    D = np.column_stack([t, y])
    dd = kmc.DataDensity(POISSON_TERM, D)

    def terms(X):
        eta = X[:, 0:1] + X[:, 1:2] * D[None, :, 0]
        return D[None, :, 1] * eta - np.exp(eta)

    host = host_yardstick(kmc, terms)
    th = np.array([0.3, 0.8]) + 0.02 * rng.standard_normal((128, 2))
    got, want = run(kmc, dd, th, 40, 10, 1), run(kmc, host, th, 40, 10, 1)
    np.testing.assert_array_equal(got["nacc"], want["nacc"])
    np.testing.assert_array_equal(got["pos"], want["pos"])
    np.testing.assert_allclose(got["logp"], want["logp"], rtol=1e-12)
    np.testing.assert_allclose(got["chain_logp"], want["chain_logp"], rtol=1e-12)


def test_minus_inf_prior_is_never_entered(kmc):
    D, beta = reg_data(500, 3, 9)
    prior = "return x[2] <= 0.0 ? -INFINITY : -x[2];"
    dd = kmc.DataDensity(REG_TERM, D, prior=prior, params=[1.0])
    host = host_yardstick(kmc, lambda X: reg_terms(X, D, 1.0), lambda X: np.where(X[:, 2] <= 0.0, -np.inf, -X[:, 2]))
    th = np.abs(beta) + 0.05 * np.abs(np.random.default_rng(2).standard_normal((64, 3)))
    got, want = run(kmc, dd, th, 60, 0, 1), run(kmc, host, th, 60, 0, 1)
    assert_same(got, want)
    assert np.all(got["chain"][:, :, 2] > 0.0) and np.all(np.isfinite(got["chain_logp"]))
    bad = th.copy()
    bad[5, 2] = -0.1
    with kmc.Sampler(dd, 64, 3, 10) as s:
        with pytest.raises(kmc.KmcError) as e:
            s.set_positions(bad)
        assert e.value.status == kmc._lib.ERR_NONFINITE_LOGP and "walker 5" in str(e.value)


def test_emcee_drop_in_recovers_the_least_squares_posterior(kmc):
    nd, sigma = 3, 0.5
    D, beta = reg_data(2000, nd, 21)
    A = np.column_stack([np.ones(len(D)), D[:, :nd - 1]])
    bhat = np.linalg.lstsq(A, D[:, nd - 1], rcond=None)[0]
    post_sd = sigma * np.sqrt(np.diag(np.linalg.inv(A.T @ A)))       # flat prior, known noise: N(bhat, sigma^2 (A'A)^-1)
    dd = kmc.DataDensity(REG_TERM, D, params=[1.0 / sigma ** 2])
    theta0s = kmc.make_theta0s(bhat, 0.1 * post_sd, dd, 64, rng=4)
    thetas, acc, logd, _ = kmc.emcee(dd, theta0s, niter=64 * 1500, nburnin=64 * 300, seed=5, use_progress_meter=False)
    samples = thetas.reshape(-1, nd)
    assert 0.2 < acc.mean() < 0.9
    assert np.all(np.abs(samples.mean(axis=0) - bhat) < 0.25 * post_sd)                          # within a quarter posterior sd
    np.testing.assert_allclose(samples.std(axis=0), post_sd, rtol=0.15)


def test_stream_chain_and_resume_equal_one_resident_run(kmc):
    D, beta = reg_data(700, 4, 13)
    dd = kmc.DataDensity(REG_TERM, D, params=[3.0])
    nw, nd, G = 128, 4, 40
    th = beta + 0.05 * np.random.default_rng(3).standard_normal((nw, nd))
    ref = run(kmc, dd, th, G)
    streamed = run(kmc, dd, th, G, stream_chain=True)
    assert "streamed" in streamed["desc"]
    assert_same(streamed, ref)
    with kmc.Sampler(dd, nw, nd, G, 0, 1, 2.0, 11) as a:
        a.set_positions(th)
        a.run(17)
        st = a.state()
    with kmc.Sampler(dd, nw, nd, G, 0, 1, 2.0, 11) as b:
        b.restore(st)
        b.run(G - 17)
        np.testing.assert_array_equal(b.positions(), ref["pos"])
        np.testing.assert_array_equal(b.logp(), ref["logp"])
        np.testing.assert_array_equal(b.naccept(), ref["nacc"])


def test_refusals_are_worded_errors(kmc):
    D, beta = reg_data(300, 3, 17)
    dd = kmc.DataDensity(REG_TERM, D, params=[1.0])
    th = beta + 0.05 * np.random.default_rng(8).standard_normal((64, 3))
    refused = [dict(dtype="f32"), dict(island_gens=4, island_size=64), dict(shard_count=2), dict(deal_count=2), dict(store_blobs=True)]
    for kw in refused:
        with pytest.raises(kmc.KmcError) as e:
            kmc.Sampler(dd, 64, 3, 10, **kw)
        assert e.value.status == kmc._lib.ERR_UNSUPPORTED, kw
        assert "KMC_DATA_DENSITY" in str(e.value), kw
    with kmc.Sampler(dd, 64, 3, 10) as s:
        with pytest.raises(kmc.KmcError, match="init_ball") as e:
            s.init_ball(beta, 0.1)
        assert e.value.status == kmc._lib.ERR_UNSUPPORTED
        s.set_positions(th)
        with pytest.raises(kmc.KmcError, match="whole generations") as e:
            s.half_step(0)
        assert e.value.status == kmc._lib.ERR_UNSUPPORTED
    with pytest.raises(kmc.KmcError, match="ndim") as e:
        kmc.Sampler(kmc.DataDensity(REG_TERM, np.zeros((4, 33))[:, :16], params=[1.0]), 70, 33, 10)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED
    with pytest.raises(kmc.KmcError, match="metropolis") as e:
        kmc.metropolis(dd, kmc.GaussianStep(0.1), beta, niter=100, use_progress_meter=False)
    assert e.value.status == kmc._lib.ERR_UNSUPPORTED


def test_the_library_copies_the_data_at_creation(kmc):
    """kmc_data_density_create itself copies: a handle made from a temporary array that is overwritten and dropped before the handle's first
    use (the first use is when the data goes to the device) evaluates exactly as a density made from the original data."""
    import ctypes as C
    from kissmcmc_jl_amd import _lib
    L = _lib.lib()
    D, beta = reg_data(1000, 3, 19)
    rows = np.ascontiguousarray(beta + 0.1 * np.random.default_rng(9).standard_normal((64, 3)))
    dp = C.POINTER(C.c_double)
    T = D.copy()
    h = C.c_void_p()
    _lib.check(L.kmc_data_density_create(REG_TERM.encode(), None, T.ctypes.data_as(dp), T.shape[0], T.shape[1], C.byref(h)))
    try:
        T[:] = 123.0
        del T
        cfg = _lib.Config()
        cfg.dtype, cfg.density, cfg.user_density = _lib.F64, _lib.DATA_DENSITY, h
        cfg.params[0] = 1.0
        cfg.nwalkers, cfg.ndim, cfg.nthin, cfg.a_scale = 64, 3, 1, 2.0
        got = np.empty(64)
        _lib.check(L.kmc_logpdf_eval_host(C.byref(cfg), rows.ctypes.data_as(dp), got.ctypes.data_as(dp), 64))
    finally:
        L.kmc_user_density_destroy(h)
    want = kmc.DataDensity(REG_TERM, D, params=[1.0])._eval_rows(rows)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want, pairwise(reg_terms(rows, D, 1.0)))
