"""The HMC step of the many-chain Metropolis sampler without a device: the rule itself on the yardstick (tests/hmc_yardstick.py:
reversibility, the order of the integrator, stationarity), every refusal of kmc_metropolis_validate, the argument errors of
kmc.HMCStep and kmc.CDensity(grad=), and a gradient body that does not compile."""
import ctypes as C

import numpy as np
import pytest

import hmc_yardstick as hy
from kissmcmc_jl_amd.metropolis import HMCStep  # noqa: F401  (the step under test: without it nothing in this file has a subject)

MU, SIGMA = 0.1, 1.3


def gauss_logpdf(X):
    t = (X - MU) * (1.0 / SIGMA)
    return -0.5 * np.sum(t * t, axis=1)


GRAD = hy.grad_of("gaussian_iso", [MU, SIGMA])


def test_trajectory_is_reversible():
    """Forward, negate the momentum, forward again: the start comes back to 1e-12 relative (the leapfrog map is its own inverse
    up to rounding; GaussianIso, step sizes per dimension, a jittered factor per chain)."""
    rng = np.random.default_rng(1)
    nc, nd = 64, 8
    x0 = MU + SIGMA * rng.standard_normal((nc, nd))
    m0 = rng.standard_normal((nc, nd))
    step = np.linspace(0.3, 0.6, nd)
    f = hy.jitter_factor(rng.integers(0, 4096, nc), 0.3)
    y, m = hy.leapfrog(GRAD, x0, m0, step, f, 7)
    assert np.max(np.abs(y - x0)) > 0.1                                   # (the trajectory went somewhere)
    xb, mb = hy.leapfrog(GRAD, y, -m, step, f, 7)
    scale = np.max(np.abs(x0))
    assert np.max(np.abs(xb - x0)) <= 1e-12 * scale
    assert np.max(np.abs(mb + m0)) <= 1e-12 * np.max(np.abs(m0))


def test_energy_error_falls_fourfold_when_eps_halves():
    """A second-order integrator: over the same trajectory length the energy error at eps / 2 is a quarter of that at eps, up to
    the next order (a relative eps^2 / sigma^2 of it, 2 % here: the bounds are 3.5 and 4.5)."""
    rng = np.random.default_rng(2)
    nc, nd = 256, 8
    x0 = MU + SIGMA * rng.standard_normal((nc, nd))
    m0 = rng.standard_normal((nc, nd))
    ones = np.ones(nc)

    def err(eps, nleap):
        y, m = hy.leapfrog(GRAD, x0, m0, eps, ones, nleap)
        return np.abs((gauss_logpdf(y) - hy.kinetic(m)) - (gauss_logpdf(x0) - hy.kinetic(m0)))

    e1, e2 = err(0.2, 6), err(0.1, 12)
    ratio = float(np.mean(e1) / np.mean(e2))
    print(f"mean |dH| {np.mean(e1):.3e} at eps 0.2, {np.mean(e2):.3e} at eps 0.1: ratio {ratio:.3f}")
    assert 3.5 < ratio < 4.5


def test_rule_leaves_the_target_stationary():
    """4096 chains started at the mean of an 8-D GaussianIso(0.1, 1.3), numpy's generator feeding the yardstick: after 300
    iterations the final states have the target's mean and variance within 5 standard errors."""
    s = hy.STAT
    rng = np.random.default_rng(7)
    th = np.full((s["nchains"], s["ndim"]), MU)
    r = hy.metropolis(gauss_logpdf, GRAD, hy.numpy_draws(rng, s["nchains"], s["ndim"]), th, s["eps"], s["nleap"], s["jitter"],
                      s["niter"], s["nburnin"], 1)
    acc = r["naccept"].sum() / (s["nchains"] * (s["niter"] - s["nburnin"]))
    rm, rv = hy.stat_errors(r["final_pos"], MU, SIGMA)
    print(f"mean off by {rm:.2f} se, variance by {rv:.2f} se, acceptance {acc:.4f}")
    assert rm < 5.0 and rv < 5.0
    assert 0.90 < acc < 0.99


def test_metropolis_validate_refuses_what_the_hmc_step_cannot_do(kmc):
    from kissmcmc_jl_amd import _lib
    lib = _lib.lib()
    dp = C.POINTER(C.c_double)
    keep = []

    def arr(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(dp)

    def cfg(ndim=3, **kw):
        c = _lib.MetropolisConfig()
        c.dtype, c.density = _lib.F64, _lib.GAUSSIAN_ISO
        c.params[0], c.params[1] = 0.0, 1.0
        c.nchains, c.ndim, c.niter, c.nburnin, c.nthin = 16, ndim, 40, 20, 1
        c.step = arr(np.full(ndim, 0.5))
        c.hmc_nleap = 4
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def ok(c):
        assert lib.kmc_metropolis_validate(C.byref(c)) == _lib.OK, lib.kmc_last_error().decode()

    def refused(c, status, *words):
        assert lib.kmc_metropolis_validate(C.byref(c)) == status
        msg = lib.kmc_last_error().decode()
        for w in words:
            assert str(w) in msg, (w, msg)

    ok(cfg())
    ok(cfg(hmc_nleap=1024, hmc_jitter=0.999))
    ok(cfg(ndim=32))
    ok(cfg(hmc_nleap=0))                                                  # the struct as it was: the random walk
    # hmc_nleap, hmc_jitter
    refused(cfg(hmc_nleap=-1), _lib.ERR_BAD_ARG, "hmc_nleap = -1")
    refused(cfg(hmc_nleap=1025), _lib.ERR_BAD_ARG, "hmc_nleap = 1025", "1024")
    refused(cfg(hmc_jitter=1.0), _lib.ERR_BAD_ARG, "hmc_jitter = 1")
    refused(cfg(hmc_jitter=-0.25), _lib.ERR_BAD_ARG, "hmc_jitter = -0.25")
    refused(cfg(hmc_jitter=np.nan), _lib.ERR_BAD_ARG, "hmc_jitter = nan")
    refused(cfg(hmc_jitter=np.inf), _lib.ERR_BAD_ARG, "hmc_jitter = inf")
    refused(cfg(hmc_nleap=0, hmc_jitter=0.5), _lib.ERR_BAD_ARG, "hmc_jitter = 0.5", "hmc_nleap = 0")
    # the step sizes
    refused(cfg(step=arr([0.5, 0.0, 0.5])), _lib.ERR_BAD_ARG, "step[1] = 0")
    refused(cfg(step=arr([0.5, 0.5, -2.5])), _lib.ERR_BAD_ARG, "step[2] = -2.5")
    refused(cfg(step=arr([np.inf, 0.5, 0.5])), _lib.ERR_BAD_ARG, "step")
    ok(cfg(hmc_nleap=0, step=arr([0.5, 0.0, -1.0])))                      # (the random walk takes any finite scale, as before)
    # what does not go with it
    L3 = np.eye(3)
    refused(cfg(step=None, chol=arr(L3)), _lib.ERR_UNSUPPORTED, "hmc_nleap = 4", "chol")
    refused(cfg(tune_rounds=2), _lib.ERR_UNSUPPORTED, "hmc_nleap = 4", "tune_rounds = 2")
    pb = _lib.HOST_PROPOSE_FN(lambda rows, n, nd, out, user: 0)
    refused(cfg(host_propose=C.cast(pb, C.c_void_p)), _lib.ERR_UNSUPPORTED, "hmc_nleap = 4", "host_propose")
    cb = _lib.HOST_LOGPDF_FN(lambda rows, n, nd, out, user: 0)
    refused(cfg(density=_lib.HOST_DENSITY, host_logpdf=C.cast(cb, C.c_void_p)), _lib.ERR_UNSUPPORTED, "hmc_nleap = 4", "KMC_HOST_DENSITY")
    refused(cfg(ndim=33), _lib.ERR_UNSUPPORTED, "ndim = 33", "32")
    body = "double s = 0.0; for (int i = 0; i < n; ++i) s += x[i] * x[i]; return -0.5 * s;"
    plain = kmc.CDensity(body)
    refused(cfg(density=_lib.USER_DENSITY, user_density=plain.user_handle), _lib.ERR_BAD_ARG, "hmc_nleap = 4", "without a gradient", "kmc_user_density_set_grad")
    expr = kmc.ExprDensity("-0.5 * x * x")
    refused(cfg(density=_lib.USER_DENSITY, user_density=expr.user_handle), _lib.ERR_UNSUPPORTED, "hmc_nleap = 4", "term / pair")
    blob = kmc.CDensity("blob[0] = x[0]; return -0.5 * x[0] * x[0];", nblob=1)
    refused(cfg(density=_lib.USER_DENSITY, user_density=blob.user_handle), _lib.ERR_UNSUPPORTED, "hmc_nleap = 4", "blobs", "nblob = 1")
    withgrad = kmc.CDensity(body, grad="for (int i = 0; i < n; ++i) g[i] = -x[i];")
    ok(cfg(density=_lib.USER_DENSITY, user_density=withgrad.user_handle))
    # what Metropolis refused before stays refused, in its own words
    refused(cfg(nthin=0), _lib.ERR_BAD_ARG, "nthin")
    refused(cfg(dtype=_lib.F32), _lib.ERR_UNSUPPORTED, "KMC_F64")
    refused(cfg(density=_lib.DATA_DENSITY), _lib.ERR_UNSUPPORTED, "KMC_DATA_DENSITY")
    refused(cfg(step=None), _lib.ERR_BAD_ARG, "neither step nor chol")
    refused(cfg(chol=arr(L3)), _lib.ERR_BAD_ARG, "both step and chol")
    refused(cfg(ndim=1, density=_lib.ROSENBROCK), _lib.ERR_BAD_ARG)
    refused(cfg(flags=1 << 20), _lib.ERR_BAD_ARG, "metropolis flags")
    # the stateless gradient call refuses without a device too
    c = _lib.Config()
    c.density, c.ndim, c.nwalkers = _lib.GAUSSIAN_ISO, 33, 2
    c.params[1] = 1.0
    x = np.zeros((1, 33))
    assert lib.kmc_grad_eval_host(C.byref(c), x.ctypes.data_as(dp), x.copy().ctypes.data_as(dp), 1) == _lib.ERR_UNSUPPORTED
    assert "ndim = 33" in lib.kmc_last_error().decode()
    c.ndim, c.density, c.user_density = 2, _lib.USER_DENSITY, plain.user_handle
    assert lib.kmc_grad_eval_host(C.byref(c), x.ctypes.data_as(dp), x.copy().ctypes.data_as(dp), 1) == _lib.ERR_BAD_ARG
    assert "kmc_user_density_set_grad" in lib.kmc_last_error().decode()


def test_hmc_step_and_cdensity_argument_errors(kmc):
    s = kmc.HMCStep(0.3)
    assert s.nleap == 8 and s.jitter == 0.0
    np.testing.assert_array_equal(s.scales(3), [0.3, 0.3, 0.3])
    np.testing.assert_array_equal(kmc.HMCStep([0.1, 0.2], nleap=3, jitter=0.5).scales(2), [0.1, 0.2])
    assert "nleap=3" in repr(kmc.HMCStep([0.1, 0.2], nleap=3))
    with pytest.raises(ValueError, match="2 step sizes for 3"):
        kmc.HMCStep([0.1, 0.2]).scales(3)
    for bad in (0.0, -1.0, np.nan, np.inf, [0.1, 0.0], [[0.1, 0.2]], []):
        with pytest.raises(ValueError, match="eps"):
            kmc.HMCStep(bad)
    for bad in (0, -3, 1025, 2.5, True):
        with pytest.raises(ValueError, match="nleap"):
            kmc.HMCStep(0.1, nleap=bad)
    for bad in (-0.1, 1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="jitter"):
            kmc.HMCStep(0.1, jitter=bad)
    with pytest.raises(TypeError, match="TunedStep"):
        kmc.TunedStep(kmc.HMCStep(0.1))                                   # nothing tunes the step sizes
    body = "return -0.5 * x[0] * x[0];"
    for bad in ("", "   ", 3, b"g[0] = -x[0];"):
        with pytest.raises(ValueError, match="grad"):
            kmc.CDensity(body, grad=bad)
    with pytest.raises(ValueError, match="nblob"):
        kmc.CDensity("blob[0] = 1.0; " + body, nblob=1, grad="g[0] = -x[0];")
    with pytest.raises(TypeError, match="menu density"):
        kmc.grad(lambda x: 0.0, [0.0])
    with pytest.raises(ValueError, match="2-dimensional"):
        kmc.grad(kmc.MvNormal2([0, 0], np.eye(2)), [0.0, 1.0, 2.0])


def test_gradient_body_that_does_not_compile_is_refused_with_the_compilers_message(kmc):
    from kissmcmc_jl_amd import _lib
    body = "return -0.5 * x[0] * x[0];"
    with pytest.raises(kmc.KmcError) as e:
        kmc.CDensity(body, grad="g[0] = -x[0] * undeclared_name;")
    assert e.value.status == _lib.ERR_BAD_ARG
    assert "does not compile" in str(e.value) and "undeclared_name" in str(e.value)
    # the handle's own refusals, and a second gradient replacing the first
    lib = _lib.lib()
    d = kmc.CDensity(body, grad="g[0] = -x[0];")
    with pytest.raises(kmc.KmcError, match="undeclared_name"):
        d.set_grad("g[0] = undeclared_name;")
    assert d.grad_body == "g[0] = -x[0];"
    d.set_grad("g[0] = -(1.0 * x[0]);")
    assert d.grad_body == "g[0] = -(1.0 * x[0]);"
    with pytest.raises(ValueError, match="grad"):
        d.set_grad("")
    assert lib.kmc_user_density_set_grad(d.user_handle, b"g[0] = -(x[0] * 1.0);") == _lib.OK
    assert lib.kmc_user_density_set_grad(d.user_handle, b"g[0] = -x[0]") == _lib.ERR_BAD_ARG       # (no semicolon)
    assert lib.kmc_user_density_set_grad(d.user_handle, b"") == _lib.ERR_BAD_ARG
    assert lib.kmc_user_density_set_grad(None, b"g[0] = 0.0;") == _lib.ERR_BAD_ARG
    assert lib.kmc_user_density_set_grad(kmc.ExprDensity("-0.5 * x * x").user_handle, b"g[0] = 0.0;") == _lib.ERR_BAD_ARG
    assert "kmc_user_density_create_body" in lib.kmc_last_error().decode()
