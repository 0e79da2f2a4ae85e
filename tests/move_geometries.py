"""The case matrix of tests/test_gpu_move_geometries.py: every (L, K, ITER) with ITER > 1 that kmc_tables.hpp builds for the DE,
snooker, mixture and tempered kernels, at ensemble sizes that leave the last wave nearly empty, exactly one walker past a wave, or
whole workgroups; the start points and seeds of every case; and its numpy yardstick (snooker_yardstick.emcee_moves,
tempering_yardstick.emcee_tempered).  No GPU is needed here:

    python tests/move_geometries.py

runs the yardstick of every case and prints whether it alone meets the cap the GPU test asserts (0 < accepted < attempted on rung 0
and over the ladder; both members of a mixture drawn), so that no case can pass vacuously."""
import os
import sys
from collections import namedtuple

import numpy as np

import snooker_yardstick as sy
import tempering_yardstick as ty

GAUSS, ROSEN = 0, 2
PARAMS = {GAUSS: [0.3, 1.5], ROSEN: [1.0, 100.0, 20.0]}
BETAS = [1.0, 0.5, 0.2]
G, NBURN, NTHIN = 10, 3, 2          # the count and sample flags both change during the job, which is cut into two run() calls
SEED = 5
MIX = (0.8, 0.2)

ALL4 = ("de", "snooker", "mix", "stretch")
DE_ST = ("de", "stretch")
# (L, K, ITER), exact row length, ragged row length (or None), moves.  Stretch runs tempered only (its plain kernels have
# tests/test_gpu_parity.py and section 4 of the test module); snooker and the mixtures are built for ITER * K <= 4.
GEOMETRIES = [
    ((2, 1, 2), 4, 3, ALL4),
    ((4, 1, 4), 8, 7, ALL4),
    ((4, 2, 2), 16, 13, ALL4),
    ((8, 2, 2), 32, 29, ALL4),
    ((8, 2, 4), 32, 29, DE_ST),                 # workgroup moment fold
    ((8, 2, 8), 32, None, ("stretch",)),        # temper_iter builds 8 for exact rows only
    ((16, 2, 2), 64, 61, ALL4),
    ((16, 2, 4), 64, 61, DE_ST),
    ((32, 2, 2), 128, 100, ("snooker", "mix")),
    ((32, 2, 4), 128, 100, DE_ST),              # workgroup moment fold, four waves per workgroup
    ((64, 2, 2), 256, 200, ALL4),               # moment ring
    ((64, 2, 4), 256, 200, DE_ST),
    ((64, 4, 2), 512, 400, DE_ST),
]
ROSEN_ROWS = (29, 32, 61, 64)                   # ... of DE and the mixtures also run Rosenbrock: its frag_partial reads across chunk boundaries

Case = namedtuple("Case", "L K ITER nd ragged size nhalf move tempered dens")


def vec_tpb(L):
    """Threads per workgroup of the vector kernels (kmc_kernels.hpp)."""
    return 128 if L <= 8 else 64 if L == 16 else 256


def sizes(L, ITER, nd):
    """Active-half sizes.  W walkers per wave, NW waves per workgroup; `min`: the smallest legal half (nwalkers >= ndim + 2, even, and
    >= 6 for snooker); `tail`: the smallest k W + 1 >= min, k >= 1 -- one walker alone in the last wave; `full`: the smallest
    multiple of W NW >= min -- whole workgroups."""
    W = (64 // L) * ITER
    NW = vec_tpb(L) // 64
    lo = max(3, (nd + 2 + 1) // 2)
    k = max(1, -(-(lo - 1) // W))
    full = -(-lo // (W * NW)) * (W * NW)
    return {"min": lo, "tail": k * W + 1, "full": full}


def cases():
    out = []
    for (L, K, ITER), nd_exact, nd_ragged, moves in GEOMETRIES:
        for nd, ragged, names in ((nd_exact, False, ("tail", "full")), (nd_ragged, True, ("min", "tail"))):
            if nd is None:
                continue
            assert (2 * L * K == nd) == (not ragged) and 2 * L * K >= nd > L * K
            sz = sizes(L, ITER, nd)
            seen = set()
            for name in names:
                if sz[name] in seen:                # (long rows: min is already one walker past a wave)
                    continue
                seen.add(sz[name])
                for move in moves:
                    for dens in (GAUSS, ROSEN) if (move in ("de", "mix") and nd in ROSEN_ROWS) else (GAUSS,):
                        for tempered in (False, True):
                            if move == "stretch" and not tempered:
                                continue
                            out.append(Case(L, K, ITER, nd, ragged, name, sz[name], move, tempered, dens))
    return out


def case_id(c):
    return "%d,%d,%d-nd%d-%s%d-%s%s%s" % (c.L, c.K, c.ITER, c.nd, c.size, c.nhalf, c.move, "-rosen" if c.dens == ROSEN else "",
                                         "-tempered" if c.tempered else "")


def plan_of(c):
    return "%d,%d,%d" % (c.L, c.K, c.ITER)


def describe_words(c):
    """What describe() must say for the case to have run what it asked for."""
    words = ["half_step_vec L=%d K=%d ITER=%d %s" % (c.L, c.K, c.ITER, "ragged" if c.ragged else "exact-size")]
    if c.move != "stretch":
        words.append({"de": "half_step_de_vec", "snooker": "half_step_snooker_vec", "mix": "half_step_mix_vec"}[c.move])
    if c.tempered:
        words.append("half_step_temper_vec")
    return words


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def start(c):
    """Start points about the density's centre with the spread the sibling tests use (0.5)."""
    centre = 1.0 if c.dens == ROSEN else PARAMS[GAUSS][0]
    return centre + 0.5 * np.random.default_rng(1000 * c.nd + c.nhalf).standard_normal((2 * c.nhalf, c.nd))


def yardstick_move(name):
    return {"stretch": None, "de": sy.DE(), "snooker": sy.Snooker(), "mix": [(sy.DE(), MIX[0]), (sy.Snooker(), MIX[1])]}[name]


def members():
    """The member index of every half-step of a mixture's job (a function of seed and step alone)."""
    _, cum = sy.mix_weights(list(MIX))
    return sy.mix_choices(SEED, np.arange(2 * G), cum)


def yardstick(c, logpdf, th):
    if c.tempered:
        return ty.emcee_tempered(logpdf, th, BETAS, G, NBURN, NTHIN, seed=SEED, move=yardstick_move(c.move), swap_every=1)
    return sy.emcee_moves(logpdf, th, G, NBURN, NTHIN, seed=SEED, move=yardstick_move(c.move))


def cap_problems(c, nacc, nswap=None):
    """The cap of every case: some, not all, of the counted proposals were accepted -- on rung 0 and summed over the rungs; a mixture
    drew both of its members; rows of a ladder changed rung.  `nacc`: [nwalkers], or [ntemps, nwalkers] of a ladder, with its `nswap`.
    Returns what is wrong (nothing: [])."""
    out = []
    nacc = np.atleast_2d(np.asarray(nacc))
    attempted = nacc.shape[1] * (G - NBURN)
    if not 0 < nacc[0].sum() < attempted:
        out.append("rung 0 accepted %d of %d" % (nacc[0].sum(), attempted))
    if not 0 < nacc.sum() < nacc.shape[0] * attempted:
        out.append("the ladder accepted %d of %d" % (nacc.sum(), nacc.shape[0] * attempted))
    if c.move == "mix" and set(members().tolist()) != {0, 1}:
        out.append("the mixture drew only member(s) %s" % sorted(set(members().tolist())))
    if c.tempered and not np.all(np.asarray(nswap) > 0):
        out.append("a pair of rungs exchanged no walker: %s" % (nswap,))
    return out


if __name__ == "__main__":
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle
    oracle.build()
    bad, t_all = 0, time.time()
    cs = cases()
    for c in cs:
        t0 = time.time()
        want = yardstick(c, lambda X: oracle.logpdf_batch(c.dens, PARAMS[c.dens], X), start(c))
        nacc = np.atleast_2d(want["nacc"])
        problems = cap_problems(c, nacc, want.get("nswap"))
        bad += bool(problems)
        print("%-46s rung 0 %4d  ladder %5d  of %5d x %d  %5.2f s  %s" % (case_id(c), nacc[0].sum(), nacc.sum(), nacc.shape[1] * (G - NBURN),
                                                                       nacc.shape[0], time.time() - t0, "; ".join(problems) or "ok"))
    print("%d cases, %d miss the cap, %.0f s" % (len(cs), bad, time.time() - t_all))
    sys.exit(1 if bad else 0)
