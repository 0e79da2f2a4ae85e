"""GPU: the workgroup-shared-draws instance of the exact-size stretch half-step (kmc_shared_draws.hpp) against the kernels it stands in for, BIT
FOR BIT -- positions, log-pdfs, naccept, the moments msum, msumsq and n -- and, for the Gaussian, against the oracle with the parity tests' helpers
and tolerances (test_gpu_parity.py, test_gpu_phase_spec.py).

One wave of a workgroup (the leader) runs Philox, z and the two logarithms for every walker of the workgroup and hands them over through LDS behind
two barriers.  The instance serves L = 8, K = 2, ITER = 2 (32-dimensional rows, two walkers per group: W = 16 walkers per wave) on a grid that is
exactly full in workgroups of SHARE waves; the updated-graph launch mode runs it in replays that lie wholly in burn-in (kmc_updated.hip:
spec_of_chunk; the instance for counted replays was measured slower than the Credit instance and is not shipped).  Every case runs three times: as
shipped, with KMC_DEBUG=share=0 (the generic kernel in burn-in; the Credit instance in counted replays either way) and with KMC_DEBUG=spec=0 (the
generic kernel everywhere).  KMC_DEBUG=fused=0 keeps small states off the
one-launch-per-generation route, no-resident keeps tiny ones out of the LDS-resident kernel."""
import numpy as np
import pytest

from kissmcmc_jl_amd import _lib
from test_gpu_parity import _theta0
from test_gpu_phase_spec import _against_oracle, _oracle_run, _pdf, _same_bits

pytestmark = pytest.mark.gpu

ND, SEED, W = 32, 77, 16
NW, G = 4096, 600                       # test_gpu_phase_spec's shape: C2's kernel on a small full grid; its oracle runs are shared
GEOMETRY = "half_step_vec L=8 K=2 ITER=2 exact-size"
BOTH = "workgroup-shared draws in burn-in replays"


def _share():
    L = _lib.lib()
    share = L.kmc_debug_shared_draws(_lib.GAUSSIAN_ISO, 8, 2, 2)
    assert share >= 2 and share * 2 <= 8
    return share


def _job(kmc, oracle, monkeypatch, debug, name="gauss", nw=NW, nd=ND, g=G, nburn=200, pieces=None, plan="8,2,2", moments=True, store_chain=False, between=None):
    monkeypatch.setenv("KMC_DEBUG", "fused=0,no-resident" + debug)
    monkeypatch.setenv("KMC_LAUNCH", "updated")
    if plan:
        monkeypatch.setenv("KMC_PLAN", plan)
    else:
        monkeypatch.delenv("KMC_PLAN", raising=False)
    with kmc.Sampler(_pdf(kmc, oracle, name), nw, nd, g, nburn, 1, 2.0, SEED, store_chain=store_chain, moments=moments) as s:
        s.set_positions(_theta0(name, nw, nd, SEED))
        for i, n in enumerate(pieces or [g]):
            s.run(n)
            if between:
                between(s, i)
        s.sync()
        got = dict(final_pos=s.positions(), final_logp=s.logp(), naccept=s.naccept(), desc=s.describe())
        if moments:
            got["sum"], got["sumsq"], got["nmoment"] = s.moments()
        if store_chain:
            got["chain"], _ = s.chain(logp=False)
    return got


def _abc(kmc, oracle, monkeypatch, **kw):
    """As shipped, share=0 and spec=0: the same bits three times."""
    new, old, gen = (_job(kmc, oracle, monkeypatch, d, **kw) for d in ("", ",share=0", ",spec=0"))
    _same_bits(new, old)
    _same_bits(new, gen)
    assert "no workgroup-shared draws (KMC_DEBUG=share=0)" in old["desc"], old["desc"]
    assert "generic kernel in every phase (KMC_DEBUG=spec=0)" in gen["desc"] and "no workgroup-shared draws (KMC_DEBUG=spec=0)" in gen["desc"], gen["desc"]
    return new, old


@pytest.mark.parametrize("workgroups", [1, 2])
def test_one_and_two_workgroups(kmc, oracle, monkeypatch, workgroups):
    """The active half is exactly one (two) shared workgroup(s): leader and last sibling are both edge waves.  300 generations, nburnin 128: a
    burn-in replay (shared), a counted replay (Credit instance), and a remainder in the generic kernel."""
    nw = 2 * workgroups * _share() * W
    new, old = _abc(kmc, oracle, monkeypatch, nw=nw, g=300, nburn=128)
    assert GEOMETRY in new["desc"] and BOTH in new["desc"], new["desc"]
    assert "phase-specialised kernel instance in counted replays" in old["desc"], old["desc"]
    _against_oracle(_oracle_run(oracle, "gauss", nw, ND, 300, 128, 1, SEED), new)


@pytest.mark.parametrize("nburn", [200, 256])
def test_c2s_kernel_on_a_small_full_grid_across_the_phase_change(kmc, oracle, monkeypatch, nburn):
    """4 096 x 32 under KMC_PLAN=8,2,2, 600 generations = four replays of 128 and a remainder.  nburnin = 200: burn-in (shared) / straddling
    (generic) / counted (Credit instance) / counted; 256: the shared instance hands over to the Credit instance exactly between two replays."""
    new, _ = _abc(kmc, oracle, monkeypatch, nburn=nburn)
    assert GEOMETRY + ", grid 64 x 128" in new["desc"] and BOTH in new["desc"], new["desc"]
    _against_oracle(_oracle_run(oracle, "gauss", NW, ND, G, nburn, 1, SEED), new)


def test_a_grid_on_which_the_second_wave_leads(kmc, oracle, monkeypatch):
    """The leader of a workgroup is wave (blockIdx.x / 512) & 1 (kmc_shared_draws.hpp): every grid above has wave 0 leading.  768 shared workgroups
    (49 152 walkers) put wave 1 in the lead, wave 0 as its sibling, in the last 256 -- next to 512 workgroups of the other kind in the same
    launch.  160 generations, nburnin 128: one shared burn-in replay and a remainder in the generic kernel."""
    nw = 2 * 768 * _share() * W
    new, _ = _abc(kmc, oracle, monkeypatch, nw=nw, g=160, nburn=128)
    assert GEOMETRY + ", grid 768 x 128" in new["desc"] and BOTH in new["desc"], new["desc"]
    _against_oracle(_oracle_run(oracle, "gauss", nw, ND, 160, 128, 1, SEED), new)


def test_a_grid_that_is_not_full_in_shared_workgroups_is_refused(kmc, oracle, monkeypatch):
    """The active half is one wave short of two shared workgroups."""
    nw = 2 * (2 * _share() - 1) * W
    new, _ = _abc(kmc, oracle, monkeypatch, nw=nw, g=300, nburn=128)
    assert "generic kernel in every phase (grid not full)" in new["desc"] and "no workgroup-shared draws (grid not full)" in new["desc"], new["desc"]
    _against_oracle(_oracle_run(oracle, "gauss", nw, ND, 300, 128, 1, SEED), new)


def test_run_in_uneven_pieces_with_set_positions_between(kmc, oracle, monkeypatch):
    """Pieces of 130, 300 and 170 generations: replays start at generations that are no multiple of 128, the phase changes inside the second
    piece, and the ensemble is moved after the first.  (Compared with the other kernels only: the oracle runs one uninterrupted job.)"""
    th = _theta0("gauss", NW, ND, SEED + 1)
    new, _ = _abc(kmc, oracle, monkeypatch, pieces=[130, 300, 170], between=lambda s, i: s.set_positions(th) if i == 0 else None)
    assert BOTH in new["desc"], new["desc"]


def test_run_in_pieces_against_the_oracle(kmc, oracle, monkeypatch):
    new, _ = _abc(kmc, oracle, monkeypatch, pieces=[128, 200, 272])
    _against_oracle(_oracle_run(oracle, "gauss", NW, ND, G, 200, 1, SEED), new)


@pytest.mark.parametrize("kw,why", [(dict(moments=False), "moments off"), (dict(store_chain=True), "chain on")])
def test_samplers_that_store_or_credit_nothing_share_draws_in_burn_in_too(kmc, oracle, monkeypatch, kw, why):
    """(A burn-in generation stores and credits nothing, whatever the sampler does later: counted replays then run the generic kernel.)"""
    new, _ = _abc(kmc, oracle, monkeypatch, g=400, nburn=256, **kw)
    assert "generic kernel in every phase (" + why + ")" in new["desc"] and BOTH in new["desc"], new["desc"]


@pytest.mark.parametrize("name", ["expo", "rosen", "lognormal"])
def test_other_menu_densities_on_the_served_geometry(kmc, oracle, monkeypatch, name):
    new, _ = _abc(kmc, oracle, monkeypatch, name=name)
    assert GEOMETRY in new["desc"] and BOTH in new["desc"], new["desc"]
    assert 0.0 < new["naccept"].mean() / (G - 200) < 1.0


def test_mvnormal2_has_no_lanes_to_share(kmc, oracle, monkeypatch):
    """Two-dimensional rows: one lane per walker (L = 1), so there is no sibling a leader lane could draw for."""
    new, _ = _abc(kmc, oracle, monkeypatch, name="mvnormal2", nd=2, plan=None)
    assert "L=1 K=1 ITER=1" in new["desc"] and "no workgroup-shared draws (no instance for this move, row type or geometry)" in new["desc"], new["desc"]
