"""The HMC step of the many-chain Metropolis sampler on the device (kmc.HMCStep) against its restatement (tests/hmc_yardstick.py:
the reference's loop, src/samplers.jl:96-126, with the leapfrog proposal, fed the stream's draws and the log-densities of the CPU oracle).

Tolerances are those of tests/test_gpu_mvnormal_step.py, for its reason: the device's log / sincospi are within 1 ulp of glibc's in the
normals, so positions agree to 1e-11 and log-pdfs and sums to 1e-10, while accept decisions are identical -- as long as no decision
is a near-tie.  Every comparison with the yardstick therefore asserts first that the yardstick's smallest |(p1 - K1) - (p0 - K0) - log u|
is above 1e-9: a condition on the inputs (the seeds below were chosen for it).  That a leapfrog trajectory keeps a 1-ulp difference of
its inputs far below these tolerances holds for the step sizes used here (the targets' scales; a divergent trajectory amplifies it)."""
import ctypes as C

import numpy as np
import pytest

import hmc_yardstick as hy

pytestmark = pytest.mark.gpu

MU, SIGMA = 0.1, 1.3
NC, NITER, NBURN, NTHIN = 777, 70, 21, 3
NLEAP, JITTER = 5, 0.2
_CACHE = {}
BITS = ("naccept", "chain", "chain_logp", "final_pos", "final_logp", "chain_sum", "chain_sumsq")


def starts(nc, nd, seed=5):
    return MU + 0.5 * np.random.default_rng(seed).standard_normal((nc, nd))


def spread(nd):
    """Step sizes per dimension, spread over 0.9 .. 1.3."""
    return np.linspace(0.9, 1.3, nd) if nd > 1 else np.array([1.1])


def reference(oracle, key, density, density_id, params, th, step, nleap, jitter, niter, nburn, nthin, seed, logpdf=None, grad=None):
    """The yardstick's run, computed once per key and shared."""
    if key not in _CACHE:
        nc, nd = th.shape
        ref = hy.metropolis(logpdf or hy.oracle_logpdf(oracle, density_id, params), grad or hy.grad_of(density, params),
                            hy.oracle_draws(oracle, seed, nc, nd), th, step, nleap, jitter, niter, nburn, nthin)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def gauss_reference(oracle, key, th, step, nleap, jitter, seed, niter=NITER, nburn=NBURN, nthin=NTHIN):
    return reference(oracle, key, "gaussian_iso", oracle.GAUSSIAN_ISO, [MU, SIGMA], th, step, nleap, jitter, niter, nburn, nthin, seed)


def assert_equals_reference(r, ref, what=""):
    print(f"{what}: yardstick margin {ref['margin']:.3e}, max |dx| {np.max(np.abs(r['chain'] - ref['chain']), initial=0.0):.3e}, "
          f"max |dlogp| {np.nanmax(np.abs(r['chain_logp'] - ref['chain_logp']), initial=0.0):.3e}, acceptance {ref['naccept'].mean() / max(1, NITER - NBURN):.3f}")
    assert ref["margin"] > 1e-9, "the inputs hold a near-tie: choose another seed"
    np.testing.assert_array_equal(r["naccept"], ref["naccept"])
    np.testing.assert_allclose(r["chain"], ref["chain"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(r["final_pos"], ref["final_pos"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(r["chain_logp"], ref["chain_logp"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["final_logp"], ref["final_logp"], rtol=1e-10, atol=1e-10)
    if r.get("chain_sum") is not None:
        np.testing.assert_allclose(r["chain_sum"], ref["chain"].sum(axis=0), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(r["chain_sumsq"], (ref["chain"] ** 2).sum(axis=0), rtol=1e-10, atol=1e-10)


# ---- every geometry against the yardstick ----
@pytest.mark.parametrize("nd", [1, 2, 3, 5, 8, 13, 16, 17, 32])
def test_every_geometry_equals_the_yardstick(kmc, oracle, nd):
    """The six register geometries with ragged tails, 777 chains (a ragged last workgroup), a step size per dimension, jitter, moments."""
    from kissmcmc_jl_amd.metropolis import run_chains
    seed = 40 + nd
    th, step = starts(NC, nd), spread(nd)
    ref = gauss_reference(oracle, ("geom", nd), th, step, NLEAP, JITTER, seed)
    r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.HMCStep(step, nleap=NLEAP, jitter=JITTER), th, NITER, NBURN, NTHIN, seed, moments=True)
    assert_equals_reference(r, ref, f"ndim {nd}")
    assert 0 < ref["naccept"].sum() < NC * (NITER - NBURN)                # (both branches of the accept test)
    np.testing.assert_array_equal(r["chol"], np.diag(step))


# ---- coupled and bounded targets ----
@pytest.mark.parametrize("nd,eps", [(2, 0.08), (5, 0.05)])
def test_rosenbrock_equals_the_yardstick(kmc, oracle, nd, eps):
    from kissmcmc_jl_amd.metropolis import run_chains
    params, seed, nc = [1.0, 100.0, 20.0], 70 + nd, 300
    th = 0.5 + 0.3 * np.random.default_rng(3).standard_normal((nc, nd))
    ref = reference(oracle, ("rosen", nd), "rosenbrock", oracle.ROSENBROCK, params, th, eps, 6, JITTER, NITER, NBURN, NTHIN, seed)
    r = run_chains(kmc.Rosenbrock(*params), kmc.HMCStep(eps, nleap=6, jitter=JITTER), th, NITER, NBURN, NTHIN, seed, moments=True)
    assert_equals_reference(r, ref, f"Rosenbrock {nd}-D")


def test_mvnormal2_with_correlation_equals_the_yardstick(kmc, oracle):
    from kissmcmc_jl_amd.metropolis import run_chains
    rho, seed, nc = 0.95, 21, 300
    pdf = kmc.MvNormal2([0.5, -0.25], [[1.0, rho], [rho, 1.0]])
    th = np.array([0.5, -0.25]) + 0.3 * np.random.default_rng(4).standard_normal((nc, 2))
    ref = reference(oracle, ("mvn2",), "mvnormal2", oracle.MVNORMAL2, pdf.params(), th, [0.15, 0.2], 8, JITTER, NITER, NBURN, NTHIN, seed)
    r = run_chains(pdf, kmc.HMCStep([0.15, 0.2], nleap=8, jitter=JITTER), th, NITER, NBURN, NTHIN, seed, moments=True)
    assert_equals_reference(r, ref, "MvNormal2 rho 0.95")
    assert 0 < ref["naccept"].sum() < nc * (NITER - NBURN)


@pytest.mark.parametrize("name", ["lognormal", "exponential"])
def test_trajectories_that_leave_the_support_are_rejected(kmc, oracle, name):
    """Chains started close to 0: some trajectories end outside the support, where the log-density is -inf; they are rejected (the
    gradient there is finite by definition: nothing propagates but the -inf)."""
    from kissmcmc_jl_amd.metropolis import run_chains
    nc, nd, seed = 300, 3, 31
    th = 0.15 + 0.25 * np.random.default_rng(6).random((nc, nd))
    if name == "lognormal":
        pdf, did, params, eps, nleap = kmc.LogNormal(0.0, 1.0), oracle.LOGNORMAL, [0.0, 1.0], 0.12, 4
    else:
        pdf, did, params, eps, nleap = kmc.Exponential(1.0), oracle.EXPONENTIAL, [1.0], 0.3, 3
    ref = reference(oracle, ("support", name), name, did, params, th, eps, nleap, JITTER, NITER, NBURN, NTHIN, seed)
    r = run_chains(pdf, kmc.HMCStep(eps, nleap=nleap, jitter=JITTER), th, NITER, NBURN, NTHIN, seed, moments=True)
    print(f"{name}: {ref['nonfinite']} of {nc * NITER} proposals outside the support")
    assert ref["nonfinite"] > 0 and ref["nonfinite_accepted"] == 0
    assert_equals_reference(r, ref, name)
    assert np.all(r["chain"] >= 0.0) and np.all(np.isfinite(r["chain_logp"])) and np.all(np.isfinite(r["final_logp"]))
    assert ref["naccept"].sum() > 0


# ---- a runtime-compiled density with the caller's gradient ----
GAUSS_BODY = "double s = 0.0; for (int i = 0; i < n; ++i) { double t = (x[i] - p[0]) * p[1]; s += t * t; } return -0.5 * s;"
GAUSS_GRAD = "for (int i = 0; i < n; ++i) { double t = (x[i] - p[0]) * p[1]; g[i] = -(t * p[1]); }"
BANANA_BODY = ("double s = 0; for (int i = 0; i + 1 < n; ++i) { double d = x[i+1] - x[i]*x[i]; s += p[1]*d*d + (p[0]-x[i])*(p[0]-x[i]); } "
               "return -s / p[2];")
BANANA_GRAD = ("for (int k = 0; k < n; ++k) { double a = 0.0; "
               "if (k >= 1) { double d = x[k] - x[k-1]*x[k-1]; a = 2.0*p[1]*d; } "
               "if (k + 1 < n) { double d = x[k+1] - x[k]*x[k]; a = a - 4.0*p[1]*x[k]*d; a = a - 2.0*(p[0] - x[k]); } "
               "g[k] = -a / p[2]; }")


def banana_logpdf(p):
    def f(X):
        X = np.atleast_2d(X)
        s = np.zeros(X.shape[0])
        for i in range(X.shape[1] - 1):
            d = X[:, i + 1] - X[:, i] * X[:, i]
            s = s + ((p[1] * d) * d + (p[0] - X[:, i]) * (p[0] - X[:, i]))
        return -s / p[2]
    return f


def banana_grad(p):
    def f(X):
        X = np.atleast_2d(X)
        n = X.shape[1]
        g = np.empty_like(X)
        for k in range(n):
            a = np.zeros(X.shape[0])
            if k >= 1:
                d = X[:, k] - X[:, k - 1] * X[:, k - 1]
                a = (2.0 * p[1]) * d
            if k + 1 < n:
                d = X[:, k + 1] - X[:, k] * X[:, k]
                a = a - ((4.0 * p[1]) * X[:, k]) * d
                a = a - 2.0 * (p[0] - X[:, k])
            g[:, k] = -a / p[2]
        return g
    return f


@pytest.mark.parametrize("nd", [5, 32])
def test_user_gradient_restating_the_menu_gaussian_agrees_with_the_menu_run(kmc, nd):
    from kissmcmc_jl_amd.metropolis import run_chains
    th, step = starts(300, nd), spread(nd) / np.sqrt(max(1.0, nd / 8.0))
    hmc = kmc.HMCStep(step, nleap=NLEAP, jitter=JITTER)
    menu = run_chains(kmc.GaussianIso(MU, SIGMA), hmc, th, NITER, NBURN, NTHIN, 9, moments=True)
    user = run_chains(kmc.CDensity(GAUSS_BODY, params=[MU, 1.0 / SIGMA], grad=GAUSS_GRAD), hmc, th, NITER, NBURN, NTHIN, 9, moments=True)
    np.testing.assert_array_equal(user["naccept"], menu["naccept"])
    assert 0 < menu["naccept"].sum() < 300 * (NITER - NBURN)
    for k in ("chain", "final_pos"):
        np.testing.assert_allclose(user[k], menu[k], rtol=1e-11, atol=1e-11, err_msg=k)
    for k in ("chain_logp", "final_logp", "chain_sum", "chain_sumsq"):
        np.testing.assert_allclose(user[k], menu[k], rtol=1e-10, atol=1e-10, err_msg=k)


def test_coupled_user_body_equals_the_yardstick(kmc, oracle):
    """The banana of CDensity's docstring in four dimensions, its gradient written by the caller; the yardstick gets both restated
    in numpy in the bodies' operation order."""
    from kissmcmc_jl_amd.metropolis import run_chains
    p, nc, nd, seed = [1.0, 100.0, 20.0], 300, 4, 13
    th = 0.5 + 0.3 * np.random.default_rng(8).standard_normal((nc, nd))
    ref = reference(oracle, ("banana",), None, None, None, th, 0.05, 6, JITTER, NITER, NBURN, NTHIN, seed, logpdf=banana_logpdf(p), grad=banana_grad(p))
    pdf = kmc.CDensity(BANANA_BODY, params=p, grad=BANANA_GRAD)
    r = run_chains(pdf, kmc.HMCStep(0.05, nleap=6, jitter=JITTER), th, NITER, NBURN, NTHIN, seed, moments=True)
    assert_equals_reference(r, ref, "banana body")


# ---- kmc.grad, kmc.check_grad ----
def test_grad_equals_the_yardsticks_gradients(kmc):
    rng = np.random.default_rng(12)
    cases = [("gaussian_iso", kmc.GaussianIso(MU, SIGMA), [1, 5, 13, 32]), ("exponential", kmc.Exponential(1.7), [3]),
             ("rosenbrock", kmc.Rosenbrock(1.0, 100.0, 20.0), [2, 5, 17, 32]),
             ("mvnormal2", kmc.MvNormal2([0.5, -0.25], [[1.0, 0.95], [0.95, 1.0]]), [2]), ("lognormal", kmc.LogNormal(0.3, 0.8), [1, 4, 9])]
    for name, pdf, dims in cases:
        for nd in dims:
            X = rng.standard_normal((301, nd))                            # (negative entries: outside the support of two of them)
            X[0] = 0.0
            want = hy.grad_of(name, pdf.params())(X)
            got = kmc.grad(pdf, X)
            assert got.shape == X.shape
            if name == "lognormal":
                np.testing.assert_allclose(got, want, rtol=1e-13, atol=0.0, err_msg=f"{name} {nd}")
                assert np.all(got[X <= 0.0] == 0.0)
            else:
                np.testing.assert_array_equal(got, want, err_msg=f"{name} {nd}")
            np.testing.assert_array_equal(kmc.grad(pdf, X[5]), got[5])        # one point
    p = [1.0, 100.0, 20.0]
    X = 0.5 + 0.3 * rng.standard_normal((64, 4))
    np.testing.assert_array_equal(kmc.grad(kmc.CDensity(BANANA_BODY, params=p, grad=BANANA_GRAD), X), banana_grad(p)(X))
    with pytest.raises(kmc.KmcError, match="kmc_user_density_set_grad"):
        kmc.grad(kmc.CDensity(BANANA_BODY, params=p), X)


def test_check_grad_flags_a_wrong_gradient_and_passes_a_right_one(kmc):
    p = [1.0, 100.0, 20.0]
    X = 0.5 + 0.3 * np.random.default_rng(14).standard_normal((64, 4))
    right = kmc.check_grad(kmc.CDensity(BANANA_BODY, params=p, grad=BANANA_GRAD), X)
    wrong = kmc.check_grad(kmc.CDensity(BANANA_BODY, params=p, grad=BANANA_GRAD.replace("4.0*p[1]", "2.0*p[1]")), X)
    menu = kmc.check_grad(kmc.Rosenbrock(*p), X)
    print(f"check_grad: right {right:.3e}, wrong {wrong:.3e}, menu Rosenbrock {menu:.3e}")
    assert right < 1e-6 and menu < 1e-6
    assert wrong > 0.1


def test_a_second_gradient_replaces_the_first_everywhere(kmc):
    """set_grad(A), use it at some ndim, set_grad(B): kmc.grad, kmc.check_grad and a run at the SAME ndim follow B; and back to A
    (the modules of a gradient are keyed by its text, so nothing of a replaced one is served again)."""
    from kissmcmc_jl_amd.metropolis import run_chains
    wrong = GAUSS_GRAD.replace("-(t * p[1])", "-(t * p[1]) * 0.25")            # a quarter of the gradient: legal, but costs acceptance
    X, th = starts(64, 5, seed=2), starts(300, 5)
    want = hy.grad_of("gaussian_iso", [MU, SIGMA])(X)
    hmc = kmc.HMCStep(spread(5), nleap=NLEAP, jitter=JITTER)
    pdf = kmc.CDensity(GAUSS_BODY, params=[MU, 1.0 / SIGMA], grad=wrong)
    np.testing.assert_array_equal(kmc.grad(pdf, X), want * 0.25)
    assert kmc.check_grad(pdf, X) > 0.1
    r_wrong = run_chains(pdf, hmc, th, NITER, NBURN, NTHIN, 9)
    ref = run_chains(kmc.CDensity(GAUSS_BODY, params=[MU, 1.0 / SIGMA], grad=GAUSS_GRAD), hmc, th, NITER, NBURN, NTHIN, 9)
    assert r_wrong["naccept"].sum() < 0.8 * ref["naccept"].sum()
    pdf.set_grad(GAUSS_GRAD)
    np.testing.assert_array_equal(kmc.grad(pdf, X), want)
    assert kmc.check_grad(pdf, X) < 1e-6
    r = run_chains(pdf, hmc, th, NITER, NBURN, NTHIN, 9)
    for k in ("naccept", "chain", "chain_logp", "final_pos", "final_logp"):
        np.testing.assert_array_equal(r[k], ref[k], err_msg=k)
    with pytest.raises(kmc.KmcError, match="does not compile"):
        pdf.set_grad("g[0] = undeclared_name;")
    np.testing.assert_array_equal(kmc.grad(pdf, X), want)                       # (a refused body leaves the gradient in force)
    pdf.set_grad(wrong)
    np.testing.assert_array_equal(kmc.grad(pdf, X), want * 0.25)
    np.testing.assert_array_equal(run_chains(pdf, hmc, th, NITER, NBURN, NTHIN, 9)["chain"], r_wrong["chain"])


# ---- seams between launches ----
def test_launch_seams_change_nothing(kmc, kmc_debug):
    from kissmcmc_jl_amd.metropolis import run_chains
    th = starts(300, 5)
    hmc = kmc.HMCStep(spread(5), nleap=NLEAP, jitter=JITTER)
    for pdf in (kmc.GaussianIso(MU, SIGMA), kmc.CDensity(GAUSS_BODY, params=[MU, 1.0 / SIGMA], grad=GAUSS_GRAD)):
        kmc_debug.unset("metro-hmc-iters")
        one = run_chains(pdf, hmc, th, NITER, NBURN, NTHIN, 3, moments=True)
        kmc_debug.set("metro-hmc-iters", 7)
        cut = run_chains(pdf, hmc, th, NITER, NBURN, NTHIN, 3, moments=True)
        for k in BITS:
            np.testing.assert_array_equal(cut[k], one[k], err_msg=k)
        assert one["naccept"].sum() > 0


# ---- edges ----
def test_one_leapfrog_step_and_no_jitter(kmc, oracle):
    from kissmcmc_jl_amd.metropolis import run_chains
    th, step = starts(300, 5), spread(5)
    ref = gauss_reference(oracle, ("nleap1",), th, step, 1, JITTER, 51)
    r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.HMCStep(step, nleap=1, jitter=JITTER), th, NITER, NBURN, NTHIN, 51, moments=True)
    assert_equals_reference(r, ref, "nleap 1")
    ref = gauss_reference(oracle, ("jitter0",), th, step, NLEAP, 0.0, 52)                # f == 1.0 exactly
    r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.HMCStep(step, nleap=NLEAP), th, NITER, NBURN, NTHIN, 52, moments=True)
    assert_equals_reference(r, ref, "jitter 0")


def test_a_huge_step_rejects_everything_and_stores_no_nan(kmc):
    from kissmcmc_jl_amd.metropolis import run_chains
    th = starts(300, 5)
    r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.HMCStep(1e6, nleap=NLEAP, jitter=JITTER), th, 30, 9, 2, 5, moments=True)
    assert not r["naccept"].any()
    np.testing.assert_array_equal(r["final_pos"], th)
    np.testing.assert_array_equal(r["chain"], np.broadcast_to(th, r["chain"].shape))
    for k in ("chain", "chain_logp", "final_logp", "chain_sum", "chain_sumsq"):
        assert np.all(np.isfinite(r[k])), k


def test_a_start_outside_the_support_is_carried_until_a_finite_proposal(kmc, oracle):
    from kissmcmc_jl_amd.metropolis import run_chains
    nc, nd, seed = 300, 2, 61
    th = 0.3 + 0.3 * np.random.default_rng(9).standard_normal((nc, nd))
    ref = reference(oracle, ("minf",), "exponential", oracle.EXPONENTIAL, [1.0], th, 0.4, 3, JITTER, NITER, NBURN, NTHIN, seed)
    outside = np.any(th < 0.0, axis=1)
    assert outside.sum() > 10
    r = run_chains(kmc.Exponential(1.0), kmc.HMCStep(0.4, nleap=3, jitter=JITTER), th, NITER, NBURN, NTHIN, seed, moments=True)
    assert ref["margin"] > 1e-9
    np.testing.assert_array_equal(r["naccept"], ref["naccept"])
    np.testing.assert_array_equal(np.isfinite(r["final_logp"]), np.isfinite(ref["final_logp"]))
    assert np.isfinite(r["final_logp"][outside]).sum() > 0                # (chains that started at -inf and found the support)
    fin = np.isfinite(ref["chain_logp"])
    np.testing.assert_array_equal(np.isfinite(r["chain_logp"]), fin)
    np.testing.assert_allclose(r["chain"], ref["chain"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(r["chain_logp"][fin], ref["chain_logp"][fin], rtol=1e-10, atol=1e-10)


def _logpdf_eval_host(pdf, rows):
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.densities import _eval_config
    rows = np.ascontiguousarray(rows)
    out = np.empty(rows.shape[0])
    dp = C.POINTER(C.c_double)
    cfg = _eval_config(pdf, rows.shape[0], rows.shape[1])
    _lib.check(_lib.lib().kmc_logpdf_eval_host(C.byref(cfg), rows.ctypes.data_as(dp), out.ctypes.data_as(dp), rows.shape[0]))
    return out


def test_stored_logp_is_the_log_density_of_the_stored_position_bit_for_bit(kmc):
    from kissmcmc_jl_amd.metropolis import run_chains
    for pdf, nd in ((kmc.GaussianIso(MU, SIGMA), 13), (kmc.Rosenbrock(1.0, 100.0, 20.0), 5),
                    (kmc.CDensity(BANANA_BODY, params=[1.0, 100.0, 20.0], grad=BANANA_GRAD), 4)):
        eps = spread(nd) if nd == 13 else 0.05
        r = run_chains(pdf, kmc.HMCStep(eps, nleap=NLEAP, jitter=JITTER), starts(300, nd), NITER, NBURN, NTHIN, 17)
        want = _logpdf_eval_host(pdf, r["chain"].reshape(-1, nd)).reshape(r["chain_logp"].shape)
        np.testing.assert_array_equal(r["chain_logp"], want)
        np.testing.assert_array_equal(r["final_logp"], _logpdf_eval_host(pdf, r["final_pos"]))


def test_by_chain_ordering_and_one_chain_through_metropolis(kmc):
    from kissmcmc_jl_amd.metropolis import run_chains
    th, hmc = starts(130, 3), kmc.HMCStep(spread(3), nleap=NLEAP, jitter=JITTER)
    pdf = kmc.GaussianIso(MU, SIGMA)
    a = run_chains(pdf, hmc, th, NITER, NBURN, NTHIN, 23)
    b = run_chains(pdf, hmc, th, NITER, NBURN, NTHIN, 23, by_chain=True)
    np.testing.assert_array_equal(b["chain"], a["chain"].transpose(1, 0, 2))
    np.testing.assert_array_equal(b["chain_logp"], a["chain_logp"].T)
    np.testing.assert_array_equal(b["naccept"], a["naccept"])
    # chain 0 of a run is the one chain of kmc.metropolis (a chain's result is a function of seed, chain index and inputs)
    thetas, acc, logd, blobs = kmc.metropolis(pdf, hmc, th[0], niter=NITER, nburnin=NBURN, nthin=NTHIN, seed=23)
    np.testing.assert_array_equal(thetas, a["chain"][:, 0, :])
    np.testing.assert_array_equal(logd, a["chain_logp"][:, 0])
    assert acc == a["accept_ratio"][0] and blobs is None
    th1, ac1, _, _ = kmc.metropolis_chains(pdf, hmc, th, niter=NITER, nburnin=NBURN, nthin=NTHIN, seed=23)
    np.testing.assert_array_equal(th1, b["chain"])
    np.testing.assert_array_equal(ac1, a["accept_ratio"])


# ---- statistical ----
def test_final_states_have_the_targets_mean_and_variance(kmc):
    """The shape of tests/test_hmc_cpu.py's stationarity test on the device: the final states of 4096 chains as independent draws."""
    from kissmcmc_jl_amd.metropolis import run_chains
    s = hy.STAT
    th = np.full((s["nchains"], s["ndim"]), MU)
    r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.HMCStep(s["eps"], nleap=s["nleap"], jitter=s["jitter"]), th, s["niter"], s["nburnin"], 1, 77,
                   store_chain=False, store_logp=False)
    rm, rv = hy.stat_errors(r["final_pos"], MU, SIGMA)
    acc = float(r["accept_ratio"].mean())
    print(f"mean off by {rm:.2f} se, variance by {rv:.2f} se, acceptance {acc:.4f}")
    assert rm < 5.0 and rv < 5.0
    assert 0.90 < acc < 0.99
