"""The case matrix of tests/test_gpu_support_edges.py: the DE, snooker, mixture and tempered kernels of the menu densities the
sibling modules never give them -- Exponential and LogNormal, whose support ends at 0, and MvNormal2 -- started so close to the edge
that a good share of the proposals leaves the support (log-pdf -inf: the flag that travels through the lane reduction, `finish` and
accept_test_beta).  Built on tests/move_geometries.py (its geometries, sizes, plans, describe() words, ladder, seed and cap); the
yardsticks are snooker_yardstick.emcee_moves and tempering_yardstick.emcee_tempered over oracle.logpdf_batch.  No GPU is needed here:

    python tests/support_edges.py

runs the yardstick of every case and prints whether it alone meets the cap the GPU test asserts: that of move_geometries, and at
least 5 and at most 90 % of the yardstick's proposals out of the support -- so that no case can pass vacuously."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
import snooker_yardstick as sy
import tempering_yardstick as ty
from move_geometries import BETAS, G, GEOMETRIES, MIX, NBURN, NTHIN, SEED, Case, describe_words, plan_of, sizes, yardstick_move
from move_geometries import cap_problems as mg_cap_problems

EXPO, LOGN, MVN2 = oracle.EXPONENTIAL, oracle.LOGNORMAL, oracle.MVNORMAL2
BODY = -1                                            # (no menu density: the function body of section 3, restated below)
NAMES = {EXPO: "expo", LOGN: "lognormal", MVN2: "mvn2", BODY: "body"}
MVN2_MEAN, MVN2_COV = [0.5, -0.25], [[0.47, 0.2], [0.2, 7.0]]      # tests/test_gpu_fuzz.py's


def mvn2_params():
    """kmc.MvNormal2(MVN2_MEAN, MVN2_COV).params(), without the package."""
    P = np.linalg.inv(np.asarray(MVN2_COV, dtype=np.float64))
    return [MVN2_MEAN[0], MVN2_MEAN[1], float(P[0, 0]), float(0.5 * (P[0, 1] + P[1, 0])), float(P[1, 1])]


PARAMS = {EXPO: [1.0], LOGN: [0.0, 1.0], MVN2: mvn2_params(), BODY: [4.0]}
CENTRE = {EXPO: 2.0, LOGN: 1.0, BODY: 2.0}           # where the start points lie, but for one coordinate per walker
EDGED = (EXPO, LOGN, BODY)                           # the densities whose support ends
LONG_BETAS = [1.0, 0.3]
LONG_G = 6
NEAR = (0.05, 1e-3)                                  # the coordinate next to the edge: |0.05 N(0, 1)| + 1e-3
CLOSE = (0.002, 4e-5)                                # ... of the long DE rows' second start (long_jobs)

# ---- the function body the recogniser cannot map (section 3): -inf below 0, NaN above p[0] --------------------------------------
NONFINITE_BODY = ("double s = 0; for (int i = 0; i < n; ++i) { if (x[i] < 0.0) return -INFINITY; "
                  "if (x[i] > p[0]) return __builtin_nan(\"\"); s += x[i]; } return -s;")


def nonfinite_body_host(X, p0):
    def row(x):
        s = 0.0
        for v in x:
            if v < 0.0:
                return -np.inf
            if v > p0:
                return np.nan
            s += v
        return -s
    return np.array([row(x) for x in X])


class Job(namedtuple("Job", "name dens nw nd move betas G plan words near", defaults=(NEAR,))):
    """One sampler run.  `plan`: KMC_PLAN, or None for the planner's own choice; `words`: what describe() must say; `near`: (scale,
    floor) of the coordinate next to the edge."""
    __slots__ = ()

    @property
    def tempered(self):
        return self.betas is not None


# ---- 1. forced geometries: every row of move_geometries.GEOMETRIES, one size each ------------------------------------------
def cases():
    """mg.Case per density, geometry, raggedness, move and plain / tempered; the size is `tail` (one walker alone in the last wave)
    for exact rows and `min` (the smallest legal half) for ragged ones -- the Gaussian matrix sweeps the sizes."""
    out = []
    for dens in (EXPO, LOGN):
        for (L, K, ITER), nd_exact, nd_ragged, moves in GEOMETRIES:
            for nd, ragged, size in ((nd_exact, False, "tail"), (nd_ragged, True, "min")):
                if nd is None:
                    continue
                for move in moves:
                    for tempered in (False, True):
                        if move == "stretch" and not tempered:
                            continue
                        out.append(Case(L, K, ITER, nd, ragged, size, sizes(L, ITER, nd)[size], move, tempered, dens))
    return out


def case_id(c):
    return "%s-%d,%d,%d-nd%d-%s%d-%s%s" % (NAMES[c.dens], c.L, c.K, c.ITER, c.nd, c.size, c.nhalf, c.move, "-tempered" if c.tempered else "")


def job_of(c):
    return Job(case_id(c), c.dens, 2 * c.nhalf, c.nd, c.move, BETAS if c.tempered else None, G, plan_of(c), describe_words(c))


def move_words(move, tempered, vec):
    kind = "vec" if vec else "generic"
    words = [] if move == "stretch" else ["half_step_%s_%s" % (move, kind)]
    return words + (["half_step_temper_" + kind] if tempered else [])


def _job(dens, nw, nd, move, betas, geometry, g=G):
    """A job without a forced plan; `geometry`: what describe() says of the vector kernel's, or None for the generic kernels."""
    tempered = betas is not None
    name = "%s-%dx%d-%s%s" % (NAMES[dens], nw, nd, move, "-tempered" if tempered else "")
    return Job(name, dens, nw, nd, move, betas, g, None, ([geometry] if geometry else []) + move_words(move, tempered, geometry is not None))


# ---- 2. short rows, long rows, the planner's own choice ----------------------------------------------------------------------
def short_jobs():
    """L = 1, K = 1, ITER = 1 (move_geometries never gets there: ITER <= L)."""
    out = []
    for dens in (EXPO, LOGN):
        for nw in (4, 66, 130):
            for move, betas in (("de", None), ("de", BETAS), ("stretch", BETAS)):
                out.append(_job(dens, nw, 1, move, betas, "half_step_vec L=1 K=1 ITER=1 ragged"))
    for nw in (6, 66):
        for move in ("de", "snooker", "mix"):
            for betas in (None, BETAS):
                out.append(_job(MVN2, nw, 2, move, betas, "half_step_vec L=1 K=1 ITER=1 exact-size"))
        out.append(_job(MVN2, nw, 2, "stretch", BETAS, "half_step_vec L=1 K=1 ITER=1 exact-size"))
    return out


def long_jobs():
    """Rows too long for a vector kernel: the generic kernels, with every move.  A DE step of such a row is short (gamma0 = 2.38 /
    sqrt(2 ndim), about 0.007 per coordinate from this start), so under 4 % of DE's proposals cross an edge 0.05 away: the DE rows run
    a second time from CLOSE, where a quarter of them do and each crossing is one coordinate's alone -- every coordinate is the near
    one of some walker, so a flag lost for one coordinate of the one-walker-per-lane sum moves a walker for about three coordinates
    in four (tried with the yardstick over a log-pdf that drops it)."""
    out = [_job(dens, 1104, 1100, move, betas, None, LONG_G) for dens in (EXPO, LOGN) for move in ("de", "snooker", "mix")
           for betas in (None, LONG_BETAS)]
    close = [j._replace(name=j.name + "-close", near=CLOSE) for j in out if j.move == "de"]
    return out + close


def planned_jobs():
    out = []
    for dens in (EXPO, LOGN):
        for move in ("de", "snooker", "mix", "stretch"):
            out.append(_job(dens, 96, 5, move, BETAS, "half_step_vec L=4 K=1 ITER=1 ragged"))
            if move != "stretch":                   # (stretch runs tempered only, as in move_geometries)
                out.append(_job(dens, 256, 33, move, None, "half_step_vec L=16 K=2 ITER=1 ragged"))
    return out


# ---- 3. the function body: compiled for exactly one geometry (section 3 of tests/test_gpu_move_geometries.py) ---------------------
def body_jobs():
    out = []
    for (L, K, ITER), nd, move, tempered in (((16, 2, 4), 61, "de", False), ((8, 2, 2), 29, "mix", True), ((8, 2, 2), 29, "de", False)):
        c = Case(L, K, ITER, nd, True, "tail", sizes(L, ITER, nd)["tail"], move, tempered, BODY)
        out.append(job_of(c)._replace(words=describe_words(c) + ["runtime-compiled"]))
    return out


def all_jobs():
    return [job_of(c) for c in cases()] + short_jobs() + long_jobs() + planned_jobs() + body_jobs()


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def start(job):
    """Every walker about the density's centre (spread 0.1: DE and snooker steps scale with the ensemble's spread, and a stationary
    start loses every DE proposal of a long row to the edge), then ONE coordinate of each walker within about 0.05 of 0 (`job.near`) -- the first
    min(nw, nd) walkers take coordinates 0, 1, ..., the others a drawn one, so that the coordinate that leaves the support sits in
    every lane and chunk position over the ensemble.  The function body's walkers get a second coordinate as close below p[0]."""
    nw, nd = job.nw, job.nd
    rng = np.random.default_rng(1000 * nd + nw // 2)
    if job.dens == MVN2:                             # no edge: about the mean, with the marginals' spread
        return np.asarray(MVN2_MEAN) + rng.standard_normal((nw, nd)) * np.sqrt(np.diag(np.asarray(MVN2_COV)))
    if nd == 1:
        return np.abs(0.3 * rng.standard_normal((nw, 1))) + 1e-3
    th = CENTRE[job.dens] + 0.1 * rng.standard_normal((nw, nd))
    near = np.abs(job.near[0] * rng.standard_normal(nw)) + job.near[1]
    col = rng.integers(0, nd, nw)
    col[:min(nw, nd)] = np.arange(min(nw, nd))
    th[np.arange(nw), col] = near
    if job.dens == BODY:
        th[np.arange(nw), (col + 1 + rng.integers(0, nd - 1, nw)) % nd] = PARAMS[BODY][0] - (np.abs(0.05 * rng.standard_normal(nw)) + 1e-3)
    return th


def host_logpdf(dens):
    if dens == BODY:
        return lambda X: nonfinite_body_host(np.asarray(X), PARAMS[BODY][0])
    return lambda X: oracle.logpdf_batch(dens, PARAMS[dens], X)


class Counting:
    """`logpdf`, counting the proposals it is given and how many of them are -inf or NaN.  The yardsticks evaluate a half-step's
    proposals in one batch of nwalkers / 2 rows and the start points in batches of nwalkers rows: only the former count.  (That is
    how the yardsticks batch their calls today; tests/test_support_edges_cpu.py holds it -- its `Outside` density asserts the number
    of proposals of every yardstick and move -- so that a yardstick that came to evaluate rungs together fails there, by name, and not
    here with counts of zero.)"""

    def __init__(self, logpdf, nwalkers):
        self.logpdf, self.nhalf = logpdf, nwalkers // 2
        self.proposals = self.ninf = self.nnan = 0

    def __call__(self, X):
        v = np.asarray(self.logpdf(X), dtype=np.float64)
        if len(v) == self.nhalf:
            self.proposals += len(v)
            self.ninf += int(np.sum(np.isneginf(v)))
            self.nnan += int(np.sum(np.isnan(v)))
        return v

    @property
    def outside(self):
        return self.ninf + self.nnan


def yardstick(job, logpdf):
    mv = yardstick_move(job.move)
    if job.tempered:
        return ty.emcee_tempered(logpdf, start(job), job.betas, job.G, NBURN, NTHIN, seed=SEED, move=mv, swap_every=1)
    return sy.emcee_moves(logpdf, start(job), job.G, NBURN, NTHIN, seed=SEED, move=mv)


_DONE = {}


def counted_yardstick(job):
    """(the yardstick's result, the Counting it ran over): computed once per job and shared by the tests, which only read it (the
    long rows' are not kept: 30 MB each)."""
    if job.name in _DONE:
        return _DONE[job.name]
    f = Counting(host_logpdf(job.dens), job.nw)
    out = yardstick(job, f), f
    if job.nd <= 512:
        _DONE[job.name] = out
    return out


def cap_problems(job, nacc, nswap, counts):
    """move_geometries.cap_problems (some, not all, of the counted proposals accepted, on rung 0 and over the ladder; both members of
    a mixture drawn; every pair of rungs exchanged), the same bound at this job's own generation count, and of the yardstick's
    proposals (`counts`: its Counting) at least 5 and at most 90 % out of the support; the function body's of both kinds."""
    out = mg_cap_problems(job, nacc, nswap)
    nacc = np.atleast_2d(np.asarray(nacc))
    attempted = nacc.shape[1] * (job.G - NBURN)
    if not (nacc[0].sum() < attempted and nacc.sum() < nacc.shape[0] * attempted):
        out.append("every one of the %d x %d counted proposals was accepted" % (nacc.shape[0], attempted))
    if job.move == "mix":                            # (move_geometries looks at its own 2 G half-steps)
        drawn = set(sy.mix_choices(SEED, np.arange(2 * job.G), sy.mix_weights(list(MIX))[1]).tolist())
        if drawn != {0, 1}:
            out.append("the mixture drew only member(s) %s in %d half-steps" % (sorted(drawn), 2 * job.G))
    if job.dens in EDGED:
        if not 5 <= counts.outside <= 0.9 * counts.proposals:
            out.append("%d of %d proposals out of the support" % (counts.outside, counts.proposals))
        if job.dens == BODY and not (counts.ninf >= 1 and counts.nnan >= 1):
            out.append("%d -inf and %d NaN proposals" % (counts.ninf, counts.nnan))
    return out


def in_support(dens, x):
    """Element-wise: is the coordinate inside the density's support?"""
    x = np.asarray(x)
    return {EXPO: x >= 0.0, LOGN: x > 0.0, BODY: (x >= 0.0) & (x <= PARAMS[BODY][0]), MVN2: np.isfinite(x)}[dens]


if __name__ == "__main__":
    import time
    oracle.build()
    bad, t_all = 0, time.time()
    jobs = all_jobs()
    for job in jobs:
        t0 = time.time()
        want, counts = counted_yardstick(job)
        nacc = np.atleast_2d(want["nacc"])
        problems = cap_problems(job, nacc, want.get("nswap"), counts)
        bad += bool(problems)
        print("%-50s rung 0 %4d  ladder %5d  of %5d x %d  outside %5d (%4d NaN) of %6d  %5.2f s  %s"
              % (job.name, nacc[0].sum(), nacc.sum(), nacc.shape[1] * (job.G - NBURN), nacc.shape[0], counts.outside, counts.nnan,
                 counts.proposals, time.time() - t0, "; ".join(problems) or "ok"))
    print("%d cases, %d miss the cap, %.0f s" % (len(jobs), bad, time.time() - t_all))
    sys.exit(1 if bad else 0)
