"""CPU: the case matrix of tests/test_gpu_support_edges.py (tests/support_edges.py) meets its own cap with the numpy yardsticks
alone -- proposals do leave the support in every case with an edge, and not all of them -- and the yardsticks reject a proposal
whose log-pdf is -inf or NaN, as the kernels must.  No GPU."""
import math

import numpy as np

import snooker_yardstick as sy
import support_edges as se
import tempering_yardstick as ty


def test_the_matrix_covers_what_it_is_for():
    jobs = se.all_jobs()
    assert len({j.name for j in jobs}) == len(jobs)
    said = lambda j, *words: all(any(w in have for have in j.words) for w in words)
    for dens in (se.EXPO, se.LOGN):
        mine = [j for j in jobs if j.dens == dens]
        for move in ("de", "snooker", "mix"):
            for row in ("exact-size", "ragged"):
                assert any(said(j, row, "half_step_%s_vec" % move) and not j.tempered for j in mine), (dens, move, row)
                assert any(said(j, row, "half_step_%s_vec" % move, "half_step_temper_vec") for j in mine), (dens, move, row)
        for move in ("de", "snooker", "mix"):
            assert any(said(j, "half_step_%s_generic" % move) and not j.tempered for j in mine), (dens, move)
            assert any(said(j, "half_step_%s_generic" % move, "half_step_temper_generic") for j in mine), (dens, move)
        assert any(j.move == "stretch" and said(j, "half_step_temper_vec") for j in mine)
        assert any(said(j, "L=1 K=1") for j in mine)
    for move in ("de", "snooker", "mix"):
        mine = [j for j in jobs if j.dens == se.MVN2 and j.move == move]
        assert any(said(j, "half_step_%s_vec" % move) and not j.tempered for j in mine), move
        assert any(said(j, "half_step_%s_vec" % move, "half_step_temper_vec") for j in mine), move
    # every geometry of the Gaussian matrix, for both densities, with every move it lists, plain (but stretch) and tempered
    want = sum(len(moves) * 2 - ("stretch" in moves) for _, exact, ragged, moves in se.GEOMETRIES for nd in (exact, ragged) if nd is not None)
    assert len(se.cases()) == 2 * want
    assert all(j.nw <= 1104 and j.G <= 10 and j.nw >= j.nd + 2 and j.nw % 2 == 0 for j in jobs)


def test_every_case_meets_its_cap_with_the_yardstick_alone():
    """All of them (the yardsticks of the whole matrix take about half a minute): `python tests/support_edges.py` prints each."""
    missed = {}
    for job in se.all_jobs():
        want, counts = se.counted_yardstick(job)
        problems = se.cap_problems(job, want["nacc"], want.get("nswap"), counts)
        # what the device must reproduce is itself inside the support, with finite log-pdfs
        if not (np.all(se.in_support(job.dens, want["pos"])) and np.all(se.in_support(job.dens, want["chain"]))):
            problems.append("the yardstick left the support")
        if not (np.all(np.isfinite(want["logp"])) and np.all(np.isfinite(want["chain_logp"]))):
            problems.append("the yardstick stored a non-finite log-pdf")
        # the long DE rows' second start is there to send many times the first one's 2 to 4 % of the proposals across the edge
        if job.near == se.CLOSE and counts.outside < 0.1 * counts.proposals:
            problems.append("only %d of %d proposals out of the support from the close start" % (counts.outside, counts.proposals))
        if problems:
            missed[job.name] = problems
    assert not missed, missed


class Outside:
    """Finite at the start points (batches of nwalkers rows); -inf and NaN in turn for every proposal (batches of half as many)."""

    def __init__(self, nwalkers):
        self.nw, self.proposals = nwalkers, 0

    def __call__(self, X):
        X = np.asarray(X)
        if X.shape[0] == self.nw:
            return -0.5 * (X * X).sum(axis=1)
        self.proposals += X.shape[0]
        return np.where(np.arange(X.shape[0]) % 2 == 0, -np.inf, np.nan)


def test_the_yardsticks_reject_minus_infinity_and_nan():
    # the accept expressions as tempering_yardstick._half_step writes them
    lus = np.array([math.log(0.5 * 2.0 ** -52), -1.0, -1e-300])           # the smallest accept uniform, and up to (almost) 1
    p0s = np.array([-1e300, -3.7, 0.0, 12.5])
    t1s = np.array([-800.0, 0.0, 1099 * math.log(2.0)])                  # (N - 1) log z at the ends of the stretch move's z, N = 1100
    with np.errstate(invalid="ignore"):
        for beta in se.BETAS + se.LONG_BETAS:
            for p1 in (-np.inf, np.nan):
                for p0 in p0s:
                    assert not np.any((beta * p1 - beta * p0) >= lus), (beta, p1, p0)                              # DE
                    for t1 in t1s:
                        assert not np.any(((t1 + beta * p1) - beta * p0) >= lus), (beta, p1, p0, t1)               # stretch, snooker
            assert not np.any((beta * -np.inf - beta * -np.inf) >= lus)                                         # (-inf against -inf: NaN)
    # ... and the samplers themselves: nothing moves, nothing is counted
    nw, nd, gens = 12, 3, 4
    th = np.random.default_rng(1).standard_normal((nw, nd))
    for move in (sy.DE(), sy.Snooker(), [(sy.DE(), 0.5), (sy.Snooker(), 0.5)]):
        f = Outside(nw)
        got = sy.emcee_moves(f, th, gens, 0, 1, seed=3, move=move)
        assert f.proposals == gens * nw
        np.testing.assert_array_equal(got["pos"], th)
        assert not got["nacc"].any()
    for move in (None, sy.DE(), sy.Snooker()):
        f = Outside(nw)
        got = ty.emcee_tempered(f, th, se.BETAS, gens, 0, 1, seed=3, move=move, swap_every=0)
        assert f.proposals == len(se.BETAS) * gens * nw
        np.testing.assert_array_equal(got["pos"], np.broadcast_to(th, (len(se.BETAS), nw, nd)))
        assert not got["nacc"].any() and np.all(np.isfinite(got["logp"]))


def test_the_counting_wrapper_counts_proposals_only():
    f = se.Counting(lambda X: np.where(X[:, 0] < 0.0, -np.inf, np.where(X[:, 0] > 4.0, np.nan, -X[:, 0])), 8)
    f(np.full((8, 2), -1.0))                                             # start points: not counted
    f(np.array([[-1.0, 0.0], [1.0, 0.0], [5.0, 0.0], [2.0, 0.0]]))
    assert (f.proposals, f.ninf, f.nnan, f.outside) == (4, 1, 1, 2)
    x = np.array([[0.5, 1.0], [0.5, -1e-300], [4.5, 1.0], [0.0, 4.0]])
    np.testing.assert_array_equal(se.nonfinite_body_host(x, 4.0), np.array([-1.5, -np.inf, np.nan, -4.0]))
