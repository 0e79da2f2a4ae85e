"""CPU: the workgroup-shared-draws instance of the half-step kernel for burn-in (kmc_shared_draws.hpp) as the host sees it -- the lookup holds one entry per
served geometry and none beyond, SHARE <= L / ITER, the variant a replay runs follows the phase, the grid and the debug switches, and the clause
kmc_sampler_describe appends leaves what bench.py reads out of a describe string as it was."""
import pytest

import bench
from kissmcmc_jl_amd import _lib

PLANNER_GEOMETRIES = [(1, 1), (2, 1), (4, 1), (4, 2), (8, 2), (16, 2), (32, 2), (64, 2), (64, 4), (64, 8)]      # kmc_plan.hip: make_plan
TUNING_GEOMETRIES = [(8, 1), (16, 1), (32, 1), (64, 1), (4, 4), (8, 4)]
MENU = [_lib.GAUSSIAN_ISO, _lib.EXPONENTIAL, _lib.ROSENBROCK, _lib.LOGNORMAL, _lib.MVNORMAL2]
SERVED = {(8, 2, 2)}                                                                                         # (L, K, ITER): C2's kernel
GENERIC, CREDIT, SHARE_BURNIN = 0, 1, 2                                                      # kmc_sampler.hpp: kVar*


@pytest.mark.parametrize("density", MENU)
def test_lookup_holds_one_entry_per_served_geometry(density):
    L = _lib.lib()
    for lanes, chunks in PLANNER_GEOMETRIES + TUNING_GEOMETRIES:
        for it in (1, 2, 4, 8, 16):
            share = L.kmc_debug_shared_draws(density, lanes, chunks, it)
            if (lanes, chunks, it) in SERVED and density != _lib.MVNORMAL2:          # (mvnormal2 rows are one lane wide: no unit)
                assert 2 <= share and share * it <= lanes, (density, lanes, chunks, it, share)       # SHARE <= L / ITER
            else:
                assert share == 0, (density, lanes, chunks, it)
    assert L.kmc_debug_shared_draws(99, 8, 2, 2) == 0


def _variant(monkeypatch, debug, nw=65536, nd=32, nburn=5000, g0=0, n=128, moments=1, chain=0, plan=None, density=None):
    monkeypatch.setenv("KMC_DEBUG", debug)
    if plan:
        monkeypatch.setenv("KMC_PLAN", plan)
    else:
        monkeypatch.delenv("KMC_PLAN", raising=False)
    return _lib.lib().kmc_debug_replay_variant(_lib.GAUSSIAN_ISO if density is None else density, nw, nd, nburn, g0, n, moments, chain)


def test_the_variant_follows_the_phase(monkeypatch):
    """C2: 65 536 x 32, nburnin 5 000 = 39 replays of 128 and 8 generations."""
    assert _variant(monkeypatch, "", g0=0) == SHARE_BURNIN and _variant(monkeypatch, "", g0=4864) == SHARE_BURNIN      # [4864, 4992): the last whole burn-in replay
    assert _variant(monkeypatch, "", g0=4992) == GENERIC                                                          # straddles nburnin
    assert _variant(monkeypatch, "", g0=4872) == SHARE_BURNIN and _variant(monkeypatch, "", g0=4873) == GENERIC    # ends exactly at / one past nburnin
    assert _variant(monkeypatch, "", g0=5000) == CREDIT and _variant(monkeypatch, "", g0=5120) == CREDIT                  # counted replays keep the Credit instance


def test_the_debug_switches_select_what_they_say(monkeypatch):
    for g0, shipped, share0 in ((0, SHARE_BURNIN, GENERIC), (5000, CREDIT, CREDIT)):
        assert _variant(monkeypatch, "", g0=g0) == shipped
        assert _variant(monkeypatch, "share=0", g0=g0) == share0
        assert _variant(monkeypatch, "fused=0,share=0", g0=g0) == share0
        assert _variant(monkeypatch, "spec=0", g0=g0) == GENERIC and _variant(monkeypatch, "share=1,spec=0", g0=g0) == GENERIC


def test_the_variant_follows_what_the_sampler_stores_and_its_grid(monkeypatch):
    for kw in (dict(moments=0), dict(chain=1)):                     # burn-in stores and credits nothing whatever comes later
        assert _variant(monkeypatch, "", g0=0, **kw) == SHARE_BURNIN and _variant(monkeypatch, "", g0=5000, **kw) == GENERIC
    share = _lib.lib().kmc_debug_shared_draws(_lib.GAUSSIAN_ISO, 8, 2, 2)
    full = 2 * 16 * share * 3                                       # three shared workgroups of 16-walker waves
    for g0, shipped in ((0, SHARE_BURNIN), (5000, CREDIT)):
        assert _variant(monkeypatch, "", nw=full, g0=g0, plan="8,2,2") == shipped
        assert _variant(monkeypatch, "", nw=full - 2 * 16, g0=g0, plan="8,2,2") == GENERIC               # one wave short: the sampler's own grid is not full either
        assert _variant(monkeypatch, "", nw=full + 2, g0=g0, plan="8,2,2") == GENERIC                     # a ragged last wave
    assert _variant(monkeypatch, "", nw=4096, nd=64, g0=5000) == CREDIT and _variant(monkeypatch, "", nw=4096, nd=64, g0=0) == GENERIC      # a geometry that is not served
    assert _variant(monkeypatch, "", nw=4096, nd=2, g0=5000, density=_lib.MVNORMAL2) == CREDIT


HOW = ("multi-launch (exact): half_step_vec L=8 K=2 ITER=2 exact-size, grid 1024 x 128, hipGraph replay of 128 generations with per-replay "
       "parameter updates (step preloaded) (measured per 64 generations: table graph 0.507 ms, updated graph 0.461 ms); phase-specialised kernel instance in counted replays")
CLAUSES = ["; workgroup-shared draws in burn-in replays (2 waves per workgroup)", "; no workgroup-shared draws (grid not full)", "; no workgroup-shared draws (KMC_DEBUG=share=0)"]


@pytest.mark.parametrize("clause", CLAUSES)
def test_the_appended_clause_changes_nothing_bench_reads(clause):
    from kissmcmc_jl_amd import GaussianIso
    for tail in ("", "; moments through a ring of 127 posted rows per wave"):
        how = HOW + clause + tail
        assert bench.kernel_geometry(how) == bench.kernel_geometry(HOW) == "half_step_vec L=8 K=2 ITER=2 exact-size, grid 1024 x 128"
        assert bench.launch_mode_of(how) == bench.launch_mode_of(HOW) == "updated_graph_128"
        assert bench.kernel_name(GaussianIso(), how) == bench.kernel_name(GaussianIso(), HOW)
        assert bench.launches_per_generation(how) == 2 and bench.moment_bytes(how) == bench.moment_bytes(HOW)
