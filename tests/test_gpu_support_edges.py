"""GPU: the move and tempered kernels of every menu density, at the edge of its support.

The DE, snooker, mixture and tempered kernels are built once per menu density; the sibling modules run them for GaussianIso and
Rosenbrock only, which are finite everywhere.  Here they run for Exponential and LogNormal -- started so close to 0 that a good share
of the proposals leaves the support, so that the flag of a lane (an infinity through the lane reduction, `finish`, and then
beta * p1 - beta * p0 in accept_test_beta) decides walkers in every lane, chunk and clamped slot -- and for MvNormal2, whose move
kernels have never run.  tests/support_edges.py holds the matrix; `python tests/support_edges.py` and tests/test_support_edges_cpu.py
show that no case is vacuous.

1. forced geometries (KMC_PLAN): every (L, K, ITER) of tests/move_geometries.py, exact and ragged rows, plain and tempered;
2. short rows (L = 1, K = 1), rows too long for a vector kernel (the generic kernels), and the planner's own choice;
3. a function body the recogniser cannot map, which answers -inf below 0 and NaN above p[0].

Every case asserts on describe() that it ran the kernel it asked for, compares with the yardstick under DESIGN.md section 6's bar
(the assert_matches of the sibling modules, unchanged), and then checks the support on the device's own read-outs."""
import numpy as np
import pytest

import support_edges as se
from test_gpu_de_move import assert_matches as assert_matches_plain
from test_gpu_move_geometries import assert_moments_are_the_chains, assert_ran, library_move, run
from test_gpu_tempering import assert_matches as assert_matches_ladder

pytestmark = pytest.mark.gpu


def density(kmc, dens):
    if dens == se.MVN2:
        pdf = kmc.MvNormal2(se.MVN2_MEAN, se.MVN2_COV)
        assert pdf.params() == se.PARAMS[se.MVN2]                           # (the oracle is given the same digest)
        return pdf
    if dens == se.BODY:
        return kmc.CDensity(se.NONFINITE_BODY, params=se.PARAMS[se.BODY])
    return kmc.Exponential(*se.PARAMS[dens]) if dens == se.EXPO else kmc.LogNormal(*se.PARAMS[dens])


def check_job(kmc, monkeypatch, job):
    th = se.start(job)
    if job.plan is None:
        monkeypatch.delenv("KMC_PLAN", raising=False)
    else:
        monkeypatch.setenv("KMC_PLAN", job.plan)
    got = run(kmc, density(kmc, job.dens), th, job.G, se.NBURN, se.NTHIN, se.SEED, move=library_move(kmc, job.move), betas=job.betas)
    monkeypatch.delenv("KMC_PLAN", raising=False)
    assert_ran(got, job.words)                                              # (a fallback to another kernel comes without a word)
    want, counts = se.counted_yardstick(job)
    if job.tempered:
        assert_matches_ladder(got, want)
        assert_moments_are_the_chains(got)
    else:
        assert_matches_plain(got, want)
    # the support, on the device's own read-outs
    stored = [got["pos"], got["chain"]] + ([got["pos0"]] if job.tempered else [])
    logps = [got["logp"], got["chain_logp"]] + ([got["logp0"]] if job.tempered else [])
    for a in stored:
        assert np.all(se.in_support(job.dens, a)), (job.name, a[~se.in_support(job.dens, a)][:8])
    for a in logps:
        assert np.all(np.isfinite(a)), (job.name, a[~np.isfinite(a)][:8])
    np.testing.assert_array_equal(got["nacc"], want["nacc"])
    problems = se.cap_problems(job, got["nacc"], got.get("nswap"), counts)
    assert not problems, problems


# ---- 1. forced geometries against the yardsticks ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", se.cases(), ids=se.case_id)
def test_forced_geometry_at_the_edge_of_the_support(kmc, oracle, monkeypatch, c):
    check_job(kmc, monkeypatch, se.job_of(c))


# ---- 2. short rows, long rows, the planner's own choice --------------------------------------------------------------------------
@pytest.mark.parametrize("job", se.short_jobs(), ids=lambda j: j.name)
def test_short_rows_one_lane_per_walker(kmc, oracle, monkeypatch, job):
    """ndim 1 and 2: L = 1, K = 1 (Exponential and LogNormal half the time out of the support; MvNormal2's moves for the first time)."""
    assert any("L=1 K=1" in w for w in job.words)
    check_job(kmc, monkeypatch, job)


@pytest.mark.parametrize("job", se.long_jobs(), ids=lambda j: j.name)
def test_long_rows_in_the_generic_kernels(kmc, oracle, monkeypatch, job):
    assert job.move in ("de", "snooker", "mix") and "half_step_%s_generic" % job.move in job.words and ("half_step_temper_generic" in job.words) == job.tempered
    check_job(kmc, monkeypatch, job)


@pytest.mark.parametrize("job", se.planned_jobs(), ids=lambda j: j.name)
def test_the_planners_own_choice(kmc, oracle, monkeypatch, job):
    assert job.plan is None
    check_job(kmc, monkeypatch, job)


# ---- 3. -inf and NaN from a function body evaluated per walker ---------------------------------------------------------------------
@pytest.mark.parametrize("job", se.body_jobs(), ids=lambda j: j.name)
def test_a_body_that_answers_minus_infinity_and_nan(kmc, monkeypatch, job):
    """A NaN proposal is rejected like one outside the support: the stored values stay finite and inside [0, p[0]], the decisions are
    the yardstick's (check_job); the yardstick met both kinds."""
    _, counts = se.counted_yardstick(job)
    assert counts.nnan >= 1 and counts.ninf >= 1, (counts.nnan, counts.ninf)
    check_job(kmc, monkeypatch, job)
