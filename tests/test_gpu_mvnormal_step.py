"""The covariance-shaped Metropolis proposal on the device (kmc.MVNormalStep, kmc.TunedStep) against its restatement
(tests/mvnormal_step_yardstick.py: the reference's loop, src/samplers.jl:96-126, fed the stream's draws by the CPU oracle).

Tolerances are those of tests/test_gpu_metropolis.py, for its reason: the device's log / sincospi are within 1 ulp of glibc's in the
normals, so positions agree to 1e-11 and log-pdfs and sums to 1e-10, while accept decisions are identical -- as long as no decision
is a near-tie.  Every comparison with the yardstick therefore asserts first that the yardstick's smallest |p1 - p0 - log u| is above
1e-9: a condition on the inputs (the seeds below were chosen for it), so a near-tie cannot masquerade as a kernel fault."""
import math

import numpy as np
import pytest

import mvnormal_step_yardstick as my

pytestmark = pytest.mark.gpu

MU, SIGMA = 0.1, 1.3
NC, NITER, NBURN, NTHIN = 777, 70, 21, 3
_CACHE = {}


def dense_factor(nd, seed=0):
    """A dense lower-triangular L, entries of order 0.3, diagonal positive."""
    rng = np.random.default_rng(1000 + 7 * nd + seed)
    L = np.tril(0.3 * rng.standard_normal((nd, nd)), -1)
    L[np.diag_indices(nd)] = 0.15 + 0.3 * rng.random(nd)
    return L


def starts(nc, nd, seed=5):
    return MU + 0.5 * np.random.default_rng(seed).standard_normal((nc, nd))


def reference(oracle, key, th, L, niter, nburn, nthin, seed, rounds=0, scale=None):
    """The yardstick's run, computed once per key and shared."""
    if key not in _CACHE:
        nd = th.shape[1]
        ref = my.metropolis(lambda v: oracle.logpdf(oracle.GAUSSIAN_ISO, [MU, SIGMA], v), lambda it, c: oracle.metropolis_draw(seed, it, c, nd),
                            th, L, niter, nburn, nthin, rounds=rounds, scale=scale)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def assert_equals_reference(r, ref, what=""):
    print(f"{what}: yardstick margin {ref['margin']:.3e}, max |dx| {np.max(np.abs(r['chain'] - ref['chain']), initial=0.0):.3e}, "
          f"max |dlogp| {np.max(np.abs(r['chain_logp'] - ref['chain_logp']), initial=0.0):.3e}")
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
@pytest.mark.parametrize("table", ["0", "1"])
@pytest.mark.parametrize("nd", [1, 2, 3, 5, 8, 13, 16, 17, 32, 33, 40])
def test_every_geometry_equals_the_yardstick(kmc, oracle, kmc_debug, nd, table):
    """The six register geometries with ragged tails and the chain-in-memory kernel, 777 chains (a ragged last workgroup), by both
    draw routes (the table serves menu densities up to 8 dimensions; beyond, both settings run the in-kernel draws)."""
    from kissmcmc_jl_amd.metropolis import run_chains
    seed = 40 + nd
    th, L = starts(NC, nd), dense_factor(nd)
    ref = reference(oracle, ("geom", nd), th, L, NITER, NBURN, NTHIN, seed)
    kmc_debug.set("metro-table", table)
    r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.MVNormalStep(chol=L), th, NITER, NBURN, NTHIN, seed, moments=True)
    assert_equals_reference(r, ref, f"ndim {nd} table {table}")
    np.testing.assert_array_equal(r["chol"], L)
    assert r["tune_skipped"] == 0


# ---- routes agree bit for bit ----
EXPR = "-0.5 * ((x - p[0]) * p[1]) * ((x - p[0]) * p[1])"
BITS = ("naccept", "chain", "chain_logp", "final_pos", "final_logp", "chain_sum", "chain_sumsq")


@pytest.mark.parametrize("nd", [2, 5, 32])
def test_table_and_in_kernel_draws_agree_bit_for_bit(kmc, kmc_debug, nd):
    """The few-chains table (delta = L z in the table, the table kernel with a step of 1.0) against the draws made in the kernel, at
    chain counts around a wave; the table also cut into launches of 16 steps.  32 dimensions: a runtime-compiled density (the table
    serves menu densities up to 8)."""
    from kissmcmc_jl_amd.metropolis import run_chains
    pdf = kmc.GaussianIso(MU, SIGMA) if nd <= 8 else kmc.ExprDensity(EXPR, params=[MU, 1.0 / SIGMA])
    L = dense_factor(nd) / math.sqrt(nd)                         # (steps short enough that the chains move, whatever the dimension)
    for nc in (1, 63, 64, 65, 130):
        th = starts(nc, nd, seed=nc)
        out = {}
        for mode, steps in (("0", None), ("1", None), ("1", 16)):
            kmc_debug.set("metro-table", mode)
            if steps:
                kmc_debug.set("metro-table-steps", steps)
            else:
                kmc_debug.unset("metro-table-steps")
            out[mode, steps] = run_chains(pdf, kmc.MVNormalStep(chol=L), th, NITER, NBURN, NTHIN, 3, moments=True)
        for k in BITS:
            np.testing.assert_array_equal(out["1", None][k], out["0", None][k], err_msg=f"{k} nchains {nc}")
            np.testing.assert_array_equal(out["1", 16][k], out["0", None][k], err_msg=f"{k} nchains {nc}, table cut")
        assert nc == 1 or out["0", None]["naccept"].sum() > 0


def test_host_logpdf_route_equals_the_in_kernel_route(kmc, oracle):
    """pdf = a closure evaluating the oracle's density, the proposal theta + L z made on the device (metro_host_propose_mv): the
    log-pdfs are the oracle's, so the run equals the yardstick's; and the in-kernel route agrees to the tolerances."""
    from kissmcmc_jl_amd.metropolis import run_chains
    nc, nd, seed = 96, 5, 17
    th, L = starts(nc, nd), dense_factor(nd)
    ref = reference(oracle, ("host", nd), th, L, NITER, NBURN, NTHIN, seed)
    pdf = kmc.HostLogPdf(lambda X: oracle.logpdf_batch(oracle.GAUSSIAN_ISO, [MU, SIGMA], X), vectorized=True)
    r = run_chains(pdf, kmc.MVNormalStep(chol=L), th, NITER, NBURN, NTHIN, seed, moments=True)
    assert_equals_reference(r, ref, "host log-pdf")
    fast = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.MVNormalStep(chol=L), th, NITER, NBURN, NTHIN, seed)
    np.testing.assert_array_equal(fast["naccept"], r["naccept"])
    np.testing.assert_allclose(fast["chain"], r["chain"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(fast["final_pos"], r["final_pos"], rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("nd", [5, 33])
def test_runtime_compiled_densities_equal_the_menu_density(kmc, kmc_debug, nd):
    """An ExprDensity (the register kernel, the memory kernel beyond 32 dimensions) and a CDensity with nblob = 2 (the memory kernel
    with blobs) writing the menu Gaussian: the same function, the same chains."""
    from kissmcmc_jl_amd.metropolis import run_chains
    kmc_debug.set("metro-table", "0")
    th, L = starts(300, nd), dense_factor(nd)
    step = kmc.MVNormalStep(chol=L)
    menu = run_chains(kmc.GaussianIso(MU, SIGMA), step, th, NITER, NBURN, NTHIN, 9)
    expr = run_chains(kmc.ExprDensity(EXPR, params=[MU, 1.0 / SIGMA]), step, th, NITER, NBURN, NTHIN, 9)
    body = ("double s = 0.0; for (int i = 0; i < n; ++i) { double d = (x[i] - p[0]) * p[1]; s += d * d; } "
            "blob[0] = x[0]; blob[1] = -0.5 * s; return -0.5 * s;")
    cden = run_chains(kmc.CDensity(body, params=[MU, 1.0 / SIGMA], nblob=2), step, th, NITER, NBURN, NTHIN, 9, store_blobs=True)
    for r, name in ((expr, "ExprDensity"), (cden, "CDensity")):
        np.testing.assert_array_equal(r["naccept"], menu["naccept"], err_msg=name)
        np.testing.assert_allclose(r["chain"], menu["chain"], rtol=1e-12, atol=1e-12, err_msg=name)
    np.testing.assert_array_equal(cden["blobs"][:, :, 0], cden["chain"][:, :, 0])          # the blob of a stored sample is that state's
    np.testing.assert_array_equal(cden["blobs"][:, :, 1], cden["chain_logp"])


# ---- L with structure ----
@pytest.mark.parametrize("nd", [3, 40])
def test_a_diagonal_factor_agrees_with_gaussian_step_to_rounding(kmc, oracle, kmc_debug, nd):
    """L = diag(step): x + (step z) against fma(step, z, x) -- one rounding more, so equal to 1e-11 and in every accept decision
    (no near-tie among them: the yardstick's margin), not bit for bit."""
    from kissmcmc_jl_amd.metropolis import run_chains
    kmc_debug.set("metro-table", "0")
    seed = 23
    th = starts(200, nd)
    step = 0.2 + 0.5 * np.random.default_rng(3).random(nd)
    ref = reference(oracle, ("diag", nd), th, np.diag(step), NITER, NBURN, NTHIN, seed)
    assert ref["margin"] > 1e-9
    a = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.MVNormalStep(chol=np.diag(step)), th, NITER, NBURN, NTHIN, seed)
    b = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.GaussianStep(step), th, NITER, NBURN, NTHIN, seed)
    np.testing.assert_array_equal(a["naccept"], b["naccept"])
    np.testing.assert_allclose(a["chain"], b["chain"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(a["final_pos"], b["final_pos"], rtol=1e-11, atol=1e-11)
    np.testing.assert_array_equal(b["chol"], np.diag(step))


def test_a_factor_with_a_zero_first_column_equals_the_yardstick(kmc, oracle, kmc_debug):
    """Every j <= i is evaluated, zeros included: 0.0 * z_0 opens every row's sum."""
    from kissmcmc_jl_amd.metropolis import run_chains
    for nd, table in ((5, "0"), (5, "1"), (33, "0")):
        L = dense_factor(nd, seed=1)
        L[1:, 0] = 0.0
        th = starts(130, nd)
        ref = reference(oracle, ("zerocol", nd), th, L, NITER, NBURN, NTHIN, 31)
        kmc_debug.set("metro-table", table)
        r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.MVNormalStep(chol=L), th, NITER, NBURN, NTHIN, 31, moments=True)
        assert_equals_reference(r, ref, f"zero first column, ndim {nd} table {table}")


def test_128_dimensions_run_and_129_are_refused(kmc, oracle):
    from kissmcmc_jl_amd import _lib
    from kissmcmc_jl_amd.metropolis import run_chains
    nd, nc, niter, nburn = 128, 70, 12, 4
    L = dense_factor(nd) / 8.0                                   # (steps short enough to be accepted now and then in 128 dimensions)
    th = starts(nc, nd)
    ref = reference(oracle, ("nd128",), th, L, niter, nburn, 1, 77)
    r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.MVNormalStep(chol=L), th, niter, nburn, 1, 77)
    assert_equals_reference(r, ref, "ndim 128")
    assert ref["naccept"].sum() > 0
    with pytest.raises(_lib.KmcError, match="129") as e:
        run_chains(kmc.GaussianIso(MU, SIGMA), kmc.MVNormalStep(chol=np.eye(129)), starts(8, 129), 4, 2, 1, 1)
    assert e.value.status == _lib.ERR_UNSUPPORTED


# ---- tuning, exact part ----
TUNE = dict(nburnin=40, rounds=3, niter=70, nthin=3)


@pytest.mark.parametrize("nd", [2, 5, 33])
def test_tuned_run_equals_the_yardstick_and_its_factor_is_the_covariance_s(kmc, oracle, nd):
    """chol_out is kmc.cholesky_lower(scale^2 kmc.covariance(states at the last boundary)) bit for bit -- those states are the
    final_pos of a second run stopped at the last boundary -- and the whole run equals the yardstick's, whose covariance is numpy's
    (so its L differs from the device's in the last bits: inside the tolerances)."""
    from kissmcmc_jl_amd.metropolis import run_chains, tune_boundaries
    seed = 60 + nd
    th = starts(NC, nd)
    init = kmc.GaussianStep(0.4 / math.sqrt(nd))
    tuned = kmc.TunedStep(init, rounds=TUNE["rounds"])
    pdf = kmc.GaussianIso(MU, SIGMA)
    r = run_chains(pdf, tuned, th, TUNE["niter"], TUNE["nburnin"], TUNE["nthin"], seed, moments=True)
    bounds = tune_boundaries(TUNE["nburnin"], TUNE["rounds"])
    assert bounds == [10, 20, 30] and r["tune_skipped"] == 0
    # a run stopped at the last boundary, with the same boundaries before it
    bR = bounds[-1]
    assert tune_boundaries(bR, TUNE["rounds"] - 1) == bounds[:-1]
    stop = run_chains(pdf, kmc.TunedStep(init, rounds=TUNE["rounds"] - 1), th, bR, bR, TUNE["nthin"], seed)
    states = stop["final_pos"]
    sc = my.default_scale(nd)
    cov = kmc.covariance(states[:, None, :])["cov"]
    np.testing.assert_array_equal(r["chol"], kmc.cholesky_lower((sc * sc) * cov))
    ref = reference(oracle, ("tune", nd), th, np.diag(np.full(nd, 0.4 / math.sqrt(nd))), TUNE["niter"], TUNE["nburnin"], TUNE["nthin"], seed,
                    rounds=TUNE["rounds"])
    assert ref["tune_skipped"] == 0
    np.testing.assert_allclose(states, ref["states_at"][bR], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(r["chol"], ref["chol"], rtol=1e-10, atol=1e-12)
    assert_equals_reference(r, ref, f"tuned, ndim {nd}")
    # an explicit scale, from an MVNormalStep: the same rule
    r2 = run_chains(pdf, kmc.TunedStep(kmc.MVNormalStep(chol=np.diag(np.full(nd, 0.4 / math.sqrt(nd)))), rounds=TUNE["rounds"], scale=sc), th,
                    TUNE["niter"], TUNE["nburnin"], TUNE["nthin"], seed, moments=True)
    for k in BITS + ("chol",):
        np.testing.assert_array_equal(r2[k], r[k], err_msg=k)


SKIP_SEED = 5


def test_a_round_with_a_zero_covariance_is_skipped(kmc, oracle, kmc_debug):
    """Every chain starts at one point (0.5: sums of it are exact, so the mean is the point and Sigma is exactly 0 while nobody has
    moved) with a first proposal so long that, for this seed, no chain accepts in iteration 0 and some do in iteration 1.  With
    nburnin = 4 and three rounds the boundaries are 1, 2, 3: the first round finds Sigma = 0 and is skipped -- the run goes on with the
    initial proposal -- and the second finds a positive variance.  The seed is a condition on the inputs: the yardstick says the same."""
    from kissmcmc_jl_amd.metropolis import run_chains
    nd, seed, niter, nburnin, rounds = 1, SKIP_SEED, 12, 4, 3
    th = np.full((NC, nd), 0.5)
    L0 = np.array([[1000.0]])
    ref = reference(oracle, ("skip",), th, L0, niter, nburnin, 2, seed, rounds=rounds)
    assert ref["tune_skipped"] == 1
    for table in ("0", "1"):
        kmc_debug.set("metro-table", table)
        r = run_chains(kmc.GaussianIso(MU, SIGMA), kmc.TunedStep(kmc.MVNormalStep(chol=L0), rounds=rounds), th, niter, nburnin, 2, seed, moments=True)
        assert r["tune_skipped"] == 1
        np.testing.assert_allclose(r["chol"], ref["chol"], rtol=1e-10)
        assert_equals_reference(r, ref, f"skipped round, table {table}")


# ---- tuning, statistical part ----
def test_tuned_chains_sample_a_correlated_target(kmc):
    """MvNormal2 with correlation 0.95, 4096 chains started at the mean with GaussianStep(0.05), four tuning rounds in 2000 iterations
    of burn-in.  The chains' final states are independent draws: their mean, every entry of their sample covariance and
    chol chol^T / scale^2 lie within 5 standard errors of the target's (se of the mean sigma / sqrt(4096); of a covariance entry
    se^2 = (S_ii S_jj + S_ij^2) / 4095).  tests/test_mvnormal_step_cpu.py shows the same bounds for the rule itself over ten seeds
    (largest ratios there: 1.75, 1.78, 2.49).  The tuned proposal also accepts at the rate 2.38 / sqrt(2) gives on a Gaussian (about
    0.35; the rule's own range over those seeds is 0.351 .. 0.362), where the untuned GaussianStep(0.05) accepts nearly always
    because it hardly moves."""
    from kissmcmc_jl_amd.metropolis import run_chains
    S = my.STAT
    cov = np.array([[1.0, S["rho"]], [S["rho"], 1.0]])
    mean = np.array(S["mean"])
    th = np.tile(mean, (S["nchains"], 1))
    r = run_chains(kmc.MvNormal2(mean, cov), kmc.TunedStep(kmc.GaussianStep(S["step0"]), rounds=S["rounds"]), th, S["niter"], S["nburnin"], 100, 12)
    assert r["nsamples"] == 4 and r["tune_skipped"] == 0
    rm, rc, rl = my.stat_bounds(r["final_pos"], r["chol"], mean, cov, my.default_scale(2))
    acc = r["accept_ratio"].mean()
    print(f"|error| / se: mean {rm:.2f}, covariance {rc:.2f}, L L^T {rl:.2f}; acceptance {acc:.3f}")
    assert rm < 5.0 and rc < 5.0 and rl < 5.0
    assert 0.25 < acc < 0.45
