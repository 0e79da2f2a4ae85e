"""GPU: the phase-specialised instance of the lane-striped half-step kernel (kmc_kernels.hpp: Spec::Credit) against the generic
kernel it was cut from, BIT FOR BIT -- positions, log-pdfs, naccept, the moments msum, msumsq and n (and the chain where one is stored) -- and
against the oracle with the parity tests' helpers and tolerances (test_gpu_parity.py).

The updated-graph launch mode keeps a graph per kernel variant; a replay of 128 generations runs the specialised variant only when all of them
are counted and the sampler credits moments and stores nothing per sample (kmc_updated.hip: spec_of_chunk); burn-in replays keep the generic kernel.
KMC_DEBUG=spec=0 forces the generic kernel everywhere: every case below runs twice, with and without it.  4 096 walkers x 32 under KMC_PLAN=8,2,2
is C2's kernel on a grid of 64 workgroups that is exactly full (2 048 active walkers = 64 x 32); KMC_DEBUG=fused=0 keeps this small state off the
one-launch-per-generation route."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_parity import LOGP_RTOL, _compare, _densities, _theta0

pytestmark = pytest.mark.gpu

NW, ND, G, SEED = 4096, 32, 600, 77
SPEC = "phase-specialised kernel instance in counted replays"


def _oracle_chain_run(oracle, name, nw, nd, g, nburn, nthin, seed, chain=True):
    _, did, params = _oracle_density(oracle, name)
    th = _theta0(name, nw, nd, seed)
    return oracle.emcee(oracle.make_config(did, params, nw, nd, g, nburn, nthin, 2.0, seed, nthreads=8), th, store_chain=chain)


@functools.lru_cache(maxsize=None)
def _oracle_run(oracle, name, nw, nd, g, nburn, nthin, seed):
    """The oracle's run without its chain, computed once and shared."""
    ref = _oracle_chain_run(oracle, name, nw, nd, g, nburn, nthin, seed, chain=False)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)          # shared among the tests: left unchanged
    return ref


MV_MEAN, MV_COV = [0.5, -0.25], [[1.0, 0.6], [0.6, 2.0]]


def _mv_params():
    """{m1, m2, P11, P12, P22}: the precision matrix, as MvNormal2.params() hands it to the kernels."""
    P = np.linalg.inv(np.asarray(MV_COV, dtype=np.float64))
    return [MV_MEAN[0], MV_MEAN[1], float(P[0, 0]), float(0.5 * (P[0, 1] + P[1, 0])), float(P[1, 1])]


def _oracle_density(oracle, name):
    table = {"gauss": (oracle.GAUSSIAN_ISO, [0.0, 1.0]), "expo": (oracle.EXPONENTIAL, [1.0]), "rosen": (oracle.ROSENBROCK, [1.0, 100.0, 20.0]),
             "lognormal": (oracle.LOGNORMAL, [0.0, 1.0]), "mvnormal2": (oracle.MVNORMAL2, _mv_params())}
    return (None,) + table[name]


def _pdf(kmc, oracle, name):
    if name == "mvnormal2":
        pdf = kmc.MvNormal2(MV_MEAN, MV_COV)
        assert pdf.params() == _mv_params()
        return pdf
    return _densities(kmc, oracle)[name][0]


def _env(monkeypatch, spec, launch="updated", plan="8,2,2"):
    monkeypatch.setenv("KMC_DEBUG", "fused=0" + ("" if spec else ",spec=0"))
    monkeypatch.setenv("KMC_LAUNCH", launch)
    if plan:
        monkeypatch.setenv("KMC_PLAN", plan)
    else:
        monkeypatch.delenv("KMC_PLAN", raising=False)


def _job(kmc, oracle, monkeypatch, spec, name="gauss", nw=NW, nd=ND, g=G, nburn=200, nthin=1, pieces=None, launch="updated", plan="8,2,2",
         moments=True, store_chain=False, store_logp=False, between=None, **kw):
    """One job run in `pieces` (default: one run of g generations); between(s, i) is called after piece i."""
    _env(monkeypatch, spec, launch, plan)
    with kmc.Sampler(_pdf(kmc, oracle, name), nw, nd, g, nburn, nthin, 2.0, SEED, store_chain=store_chain, store_logp=store_logp, moments=moments, **kw) as s:
        s.set_positions(_theta0(name, nw, nd, SEED))
        for i, n in enumerate(pieces or [g]):
            s.run(n)
            if between:
                between(s, i)
        s.sync()
        got = dict(final_pos=s.positions(), final_logp=s.logp(), naccept=s.naccept(), accept_ratio=s.accept_ratio(), desc=s.describe())
        if moments:
            got["sum"], got["sumsq"], got["nmoment"] = s.moments()
        if store_chain:
            got["chain"], got["chain_logp"] = s.chain(logp=store_logp)
        elif store_logp:                 # (Sampler.chain always asks for the positions: the log-pdfs alone through the C entry point)
            lp = np.empty(((g - nburn) // nthin, nw))
            kmc._lib.check(kmc._lib.lib().kmc_sampler_get_chain(s._h, None, lp.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
            got["chain"], got["chain_logp"] = None, lp
    return got


def _same_bits(a, b):
    for key in ("final_pos", "final_logp", "naccept", "sum", "sumsq", "chain", "chain_logp"):
        assert (key in a) == (key in b)
        if key in a and a[key] is not None:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a.get("nmoment") == b.get("nmoment")


def _against_oracle(ref, got, moments=True):
    """test_gpu_parity._compare without a stored chain: the same quantities, the same tolerances."""
    assert ref["status"] == 0
    np.testing.assert_array_equal(got["naccept"], ref["naccept"])
    np.testing.assert_array_equal(got["final_pos"], ref["final_pos"])
    assert np.all(np.abs(got["final_logp"] - ref["final_logp"]) <= LOGP_RTOL * np.maximum(1.0, np.abs(ref["final_logp"])))
    if moments:
        assert got["nmoment"] == ref["nmoment"]
        np.testing.assert_allclose(got["sum"], ref["sum"], rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(got["sumsq"], ref["sumsq"], rtol=1e-11, atol=1e-9)


def _ab(kmc, oracle, monkeypatch, **kw):
    new, old = _job(kmc, oracle, monkeypatch, True, **kw), _job(kmc, oracle, monkeypatch, False, **kw)
    _same_bits(new, old)
    return new, old


@pytest.mark.parametrize("nburn", [200, 0, G, 256])
def test_replays_on_either_side_of_the_phase_change(kmc, oracle, monkeypatch, nburn):
    """600 generations = four replays of 128 and a remainder.  nburnin = 200: burn-in (generic) / straddling (generic) / credit / credit; 0: credit
    only; 600: burn-in only; 256: the phase changes exactly between two replays."""
    new, old = _ab(kmc, oracle, monkeypatch, nburn=nburn)
    assert "half_step_vec L=8 K=2 ITER=2 exact-size, grid 64 x 128" in new["desc"] and SPEC in new["desc"], new["desc"]
    assert "generic kernel in every phase (KMC_DEBUG=spec=0)" in old["desc"], old["desc"]
    _against_oracle(_oracle_run(oracle, "gauss", NW, ND, G, nburn, 1, SEED), new)


def test_a_grid_that_is_not_full_keeps_the_generic_kernel(kmc, oracle, monkeypatch):
    new, _ = _ab(kmc, oracle, monkeypatch, nw=NW + 2)
    assert "grid 65 x 128" in new["desc"] and "generic kernel in every phase (grid not full)" in new["desc"], new["desc"]
    _against_oracle(_oracle_run(oracle, "gauss", NW + 2, ND, G, 200, 1, SEED), new)


@pytest.mark.parametrize("what,kw,why", [("moments_off", dict(moments=False), "moments off"),
                                         ("chain_thin1", dict(store_chain=True, store_logp=True), "chain on"),
                                         ("chain_thin7", dict(store_chain=True, nthin=7), "chain on"),
                                         ("chain_logp", dict(store_logp=True), "chain on")])
def test_samplers_that_store_per_sample_or_credit_nothing_never_run_the_credit_instance(kmc, oracle, monkeypatch, what, kw, why):
    new, _ = _ab(kmc, oracle, monkeypatch, **kw)
    assert "generic kernel in every phase (" + why + ")" in new["desc"], new["desc"]
    ref = (_oracle_chain_run if kw.get("store_chain") else _oracle_run)(oracle, "gauss", NW, ND, G, 200, kw.get("nthin", 1), SEED)
    if kw.get("store_chain") and kw.get("store_logp") and kw.get("moments", True):
        _compare(ref, new)
    else:
        _against_oracle(ref, new, moments=kw.get("moments", True))
        if kw.get("store_chain"):
            np.testing.assert_array_equal(new["chain"], ref["chain"])
        if kw.get("store_logp"):
            lp = _oracle_chain_run(oracle, "gauss", NW, ND, G, 200, 1, SEED)["chain_logp"]
            assert np.all(np.abs(new["chain_logp"] - lp) <= LOGP_RTOL * np.maximum(1.0, np.abs(lp)))


@pytest.mark.parametrize("pieces,g,nburn", [([100] * 6, G, 200), ([1024, 76], 1100, 300)])
def test_run_in_pieces(kmc, oracle, monkeypatch, pieces, g, nburn):
    """Pieces of 100 never hold a whole replay (table graph and eager launches: generic); 1024 + 76 is eight replays and a remainder."""
    new, _ = _ab(kmc, oracle, monkeypatch, g=g, nburn=nburn, pieces=pieces)
    _against_oracle(_oracle_run(oracle, "gauss", NW, ND, g, nburn, 1, SEED), new)


def test_set_positions_in_the_middle(kmc, oracle, monkeypatch):
    """(Compared with the generic kernels only: the oracle runs one uninterrupted job.)"""
    th = _theta0("gauss", NW, ND, SEED + 1)
    _ab(kmc, oracle, monkeypatch, pieces=[300, 300], between=lambda s, i: s.set_positions(th) if i == 0 else None)


def test_state_and_restore_across_the_phase_change(kmc, oracle, monkeypatch):
    """A checkpoint taken in burn-in and restored into the same sampler before the counted phase: the walkers end where the uninterrupted run
    ends (moments restart at a restore -- those are compared with the generic kernels' only)."""
    def between(s, i):
        if i == 0:
            s.sync()
            s.restore(s.state())
    new, _ = _ab(kmc, oracle, monkeypatch, pieces=[128, G - 128], between=between)
    _against_oracle(_oracle_run(oracle, "gauss", NW, ND, G, 200, 1, SEED), new, moments=False)


@pytest.mark.parametrize("launch", ["graph", "eager"])
def test_other_launch_modes_keep_the_generic_kernel(kmc, oracle, monkeypatch, launch):
    new, _ = _ab(kmc, oracle, monkeypatch, launch=launch)
    assert "phase-specialised" not in new["desc"], new["desc"]
    _against_oracle(_oracle_run(oracle, "gauss", NW, ND, G, 200, 1, SEED), new)


@pytest.mark.parametrize("name,nd,geometry", [("expo", 16, "L=4 K=2 ITER=1 exact-size, grid 64 x 128"), ("rosen", 64, "L=16 K=2 ITER=1 exact-size, grid 512 x 64"),
                                              ("lognormal", 128, "L=32 K=2 ITER=1 exact-size, grid 256 x 256"), ("mvnormal2", 2, "L=1 K=1 ITER=1 exact-size, grid 16 x 128")])
def test_other_menu_densities_at_their_planners_geometry(kmc, oracle, monkeypatch, name, nd, geometry):
    """No KMC_PLAN: what make_plan picks for 4 096 walkers of this row length (one walker per group: 2 048 active walkers are fewer than the
    3 072 single-walker waves from which it pairs them).  L = 16 and 32 carry the draw ring."""
    ref = _oracle_run(oracle, name, NW, nd, G, 200, 1, SEED)
    assert ref["status"] == 0                      # (the oracle alone accepts the shape)
    new, _ = _ab(kmc, oracle, monkeypatch, name=name, nd=nd, plan=None)
    assert geometry in new["desc"] and SPEC in new["desc"], new["desc"]
    _against_oracle(ref, new)


def test_a_de_sampler_keeps_the_generic_route(kmc, oracle, monkeypatch):
    new, _ = _ab(kmc, oracle, monkeypatch, plan=None, move=kmc.DEMove())
    assert "half_step_de_vec" in new["desc"] and "generic kernel in every phase (no instance for this move, row type or geometry)" in new["desc"], new["desc"]


def test_a_tempered_sampler_keeps_the_generic_route(kmc, oracle, monkeypatch):
    """(Walkers bit for bit.  The swap sweep credits exchanged rows with atomic adds, in an order that changes from run to run of the SAME
    kernels: the moments at the parity tests' tolerance.)"""
    new, old = (_job(kmc, oracle, monkeypatch, spec, plan=None, betas=[1.0, 0.5, 0.25]) for spec in (True, False))
    assert "half_step_temper_vec" in new["desc"] and "phase-specialised" not in new["desc"], new["desc"]
    for key in ("final_pos", "final_logp", "naccept"):
        np.testing.assert_array_equal(new[key], old[key], err_msg=key)
    assert new["nmoment"] == old["nmoment"]
    np.testing.assert_allclose(new["sum"], old["sum"], rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(new["sumsq"], old["sumsq"], rtol=1e-11, atol=1e-9)
