"""Every route of kmc_metropolis_run through the set-up and the read-out they share (kmc_metropolis_api.hip: metropolis_setup,
metropolis_read_out), crossed with every proposal and both chain layouts.

The neighbouring files compare each route with the CPU oracle, mostly sample-major and with one proposal.  Here the claims are exact
ones about the outputs themselves: the by-chain layout is the sample-major one with its first two axes swapped, everything else is the
same bits in both runs, the final state is the last stored sample, the ratios are the counts over niter - nburnin, and the few-chains
table gives the bits of the in-kernel draws.  300 chains are two workgroups of 256, the second ragged; 90 iterations, 30 of burn-in,
thinned by 3: 20 stored samples, the last iteration stored; the tuning boundaries of two rounds are 10 and 20, and a table of 7 steps
puts launch seams between them and inside the run.  Only the moments are compared with a tolerance: the sums of the stored samples
formed by numpy, to the 1e-10 of tests/test_gpu_metropolis.py (20 terms of order one: rounding alone is some 1e-15)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MU, SIGMA = 0.1, 1.3
NC, NITER, NBURN, NTHIN, NSAMPLES, SEED = 300, 90, 30, 3, 20, 11
BODY = ("double s = 0.0; for (int i = 0; i < n; ++i) { double d = (x[i] - p[0]) * p[1]; s += d * d; } "
        "blob[0] = x[0]; blob[1] = -0.5 * s; return -0.5 * s;")
# route -> ndim, KMC_DEBUG options
ROUTES = {
    "register": (3, {"metro-table": "0"}),
    "memory": (33, {"metro-table": "0"}),
    "table": (3, {"metro-table": "1", "metro-table-steps": 7}),
    "blobs": (3, {}),
    "host-logpdf": (3, {}),
    "host-proposal": (3, {}),
}
# (what kmc_metropolis_validate refuses is left out: chol or tuning with a host proposal)
CASES = [(route, prop) for route in ROUTES if route != "host-proposal" for prop in ("gaussian", "mvnormal", "tuned")] + [("host-proposal", "closure")]
SAME = ("final_pos", "final_logp", "final_blob", "naccept", "accept_ratio", "chain_sum", "chain_sumsq", "chol", "tune_skipped")
_DENSITIES = {}


def starts(nd):
    return MU + 0.5 * np.random.default_rng(5).standard_normal((NC, nd))


def factor(nd):
    """A dense lower-triangular L with a positive diagonal, short enough that the chains move in nd dimensions."""
    rng = np.random.default_rng(1000 + nd)
    L = np.tril(0.3 * rng.standard_normal((nd, nd)), -1)
    L[np.diag_indices(nd)] = 0.15 + 0.3 * rng.random(nd)
    return L / math.sqrt(nd)


def density(kmc, oracle, route):
    if route == "blobs":                         # (one object for every case: its programs are compiled once)
        if "blobs" not in _DENSITIES:
            _DENSITIES["blobs"] = kmc.CDensity(BODY, params=[MU, 1.0 / SIGMA], nblob=2)
        return _DENSITIES["blobs"]
    if route == "host-logpdf":
        return kmc.HostLogPdf(lambda X: oracle.logpdf_batch(oracle.GAUSSIAN_ISO, [MU, SIGMA], X), vectorized=True)
    return kmc.GaussianIso(MU, SIGMA)


def proposal(kmc, prop, nd):
    from kissmcmc_jl_amd.metropolis import HostProposal
    if prop == "gaussian":
        return kmc.GaussianStep(0.4 / math.sqrt(nd))
    if prop == "mvnormal":
        return kmc.MVNormalStep(chol=factor(nd))
    if prop == "tuned":
        return kmc.TunedStep(kmc.GaussianStep(0.4 / math.sqrt(nd)), rounds=2)
    calls = {"n": 0}                             # a closure with a fixed schedule: the same proposals in every run that starts it afresh

    def fn(X):
        calls["n"] += 1
        return X + 0.4 * np.cos(calls["n"] + np.arange(X.size).reshape(X.shape))
    return HostProposal(fn, vectorized=True)


def run(kmc, oracle, kmc_debug, route, prop, by_chain):
    from kissmcmc_jl_amd.metropolis import run_chains
    nd, opts = ROUTES[route]
    for k, v in opts.items():
        kmc_debug.set(k, v)
    return run_chains(density(kmc, oracle, route), proposal(kmc, prop, nd), starts(nd), NITER, NBURN, NTHIN, SEED, moments=True, store_logp=True,
                      by_chain=by_chain, store_blobs=route == "blobs")


def same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
    else:
        np.testing.assert_array_equal(a, b, err_msg=what)


@pytest.mark.parametrize("route,prop", CASES)
def test_both_layouts_of_every_route_and_proposal(kmc, oracle, kmc_debug, route, prop):
    sm = run(kmc, oracle, kmc_debug, route, prop, by_chain=False)
    bc = run(kmc, oracle, kmc_debug, route, prop, by_chain=True)
    nd = ROUTES[route][0]
    assert sm["nsamples"] == NSAMPLES and bc["nsamples"] == NSAMPLES
    assert sm["chain"].shape == (NSAMPLES, NC, nd) and bc["chain"].shape == (NC, NSAMPLES, nd)
    np.testing.assert_array_equal(bc["chain"], np.swapaxes(sm["chain"], 0, 1))
    np.testing.assert_array_equal(bc["chain_logp"], np.swapaxes(sm["chain_logp"], 0, 1))
    if route == "blobs":
        assert sm["blobs"].shape == (NSAMPLES, NC, 2)
        np.testing.assert_array_equal(bc["blobs"], np.swapaxes(sm["blobs"], 0, 1))
        np.testing.assert_array_equal(sm["blobs"][:, :, 0], sm["chain"][:, :, 0])      # (the blob of a stored sample is that state's)
        np.testing.assert_array_equal(sm["blobs"][:, :, 1], sm["chain_logp"])
        np.testing.assert_array_equal(sm["final_blob"], sm["blobs"][-1])
    else:
        assert sm["blobs"] is None and sm["final_blob"] is None
    for k in SAME:
        same(bc[k], sm[k], f"{k}, by chain against sample-major")
    assert (sm["chol"] is None) == (route == "host-proposal")
    np.testing.assert_array_equal(sm["final_pos"], sm["chain"][-1])
    np.testing.assert_array_equal(sm["final_logp"], sm["chain_logp"][-1])
    np.testing.assert_array_equal(sm["accept_ratio"], sm["naccept"] / (NITER - NBURN))
    assert sm["naccept"].sum() > 0
    np.testing.assert_allclose(sm["chain_sum"], sm["chain"].sum(axis=0), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(sm["chain_sumsq"], (sm["chain"] ** 2).sum(axis=0), rtol=1e-10, atol=1e-10)


def test_table_and_in_kernel_draws_agree_bit_for_bit_with_gaussian_step(kmc, oracle, kmc_debug):
    """What tests/test_gpu_mvnormal_step.py claims for MVNormalStep, for the isotropic proposal: the table, cut into launches of 7
    steps, against the draws made in the register kernel, on every output."""
    reg = run(kmc, oracle, kmc_debug, "register", "gaussian", by_chain=False)
    tab = run(kmc, oracle, kmc_debug, "table", "gaussian", by_chain=False)
    for k in ("chain", "chain_logp") + SAME:
        same(tab[k], reg[k], f"{k}, table against in-kernel draws")
    assert tab["nsamples"] == reg["nsamples"] == NSAMPLES
