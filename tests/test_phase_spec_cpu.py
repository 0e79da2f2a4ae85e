"""CPU: the phase-specialised half-step instance (kmc_kernels.hpp: Spec::Credit) as the host sees it -- the lookup holds one
for every geometry make_plan picks by itself with one or two walkers per group, and none beyond; and the clause kmc_sampler_describe appends for
it leaves what bench.py reads out of a describe string as it was."""
import pytest

import bench
from kissmcmc_jl_amd import _lib

PLANNER_GEOMETRIES = [(1, 1), (2, 1), (4, 1), (4, 2), (8, 2), (16, 2), (32, 2), (64, 2), (64, 4), (64, 8)]      # kmc_plan.hip: make_plan
MENU = [_lib.GAUSSIAN_ISO, _lib.EXPONENTIAL, _lib.ROSENBROCK, _lib.LOGNORMAL, _lib.MVNORMAL2]


@pytest.mark.parametrize("density", MENU)
def test_lookup_holds_an_instance_for_the_planner_geometries(density):
    L = _lib.lib()
    for lanes, chunks in PLANNER_GEOMETRIES:
        for it in (1, 2):
            want = 1 if it <= lanes and it * chunks <= 16 else 0          # (a group's walkers must fit its lanes: kmc_tables.hpp, vec_one)
            assert L.kmc_debug_phase_spec(density, lanes, chunks, it) == want, (density, lanes, chunks, it)
        for it in (4, 8, 16):                                             # large-ensemble geometries stay generic
            assert L.kmc_debug_phase_spec(density, lanes, chunks, it) == 0
    for lanes, chunks in [(8, 1), (16, 1), (32, 1), (64, 1), (4, 4), (8, 4)]:          # the tuning geometries (KMC_PLAN) too
        assert L.kmc_debug_phase_spec(density, lanes, chunks, 1) == 0
    assert L.kmc_debug_phase_spec(99, 8, 2, 2) == 0


HOW = ("multi-launch (exact): half_step_vec L=8 K=2 ITER=2 exact-size, grid 1024 x 128, hipGraph replay of 128 generations with per-replay "
       "parameter updates (step preloaded) (measured per 64 generations: table graph 0.507 ms, updated graph 0.461 ms)")
CLAUSES = ["; phase-specialised kernel instance in counted replays", "; generic kernel in every phase (chain on)", "; generic kernel in every phase (grid not full)"]


@pytest.mark.parametrize("clause", CLAUSES)
def test_the_appended_clause_changes_nothing_bench_reads(clause):
    from kissmcmc_jl_amd import GaussianIso
    for tail in ("", "; moments through a ring of 127 posted rows per wave"):
        how = HOW + clause + tail
        assert bench.kernel_geometry(how) == bench.kernel_geometry(HOW) == "half_step_vec L=8 K=2 ITER=2 exact-size, grid 1024 x 128"
        assert bench.launch_mode_of(how) == bench.launch_mode_of(HOW) == "updated_graph_128"
        assert bench.kernel_name(GaussianIso(), how) == bench.kernel_name(GaussianIso(), HOW)
        assert bench.launches_per_generation(how) == 2 and bench.moment_bytes(how) == bench.moment_bytes(HOW)
