"""The inputs of the relative-efficiency tests (tests/test_gpu_relative_eff.py, tests/test_relative_eff_cpu.py), hand-built and computed
once, and the measurement of the yardsticks' own error on them.  Needs no device.

Inputs: psis_cases.TERM over thetas built from convergence_yardstick.ar1, ``th = [0.5 a0, 1 + 0.1 a1]``, so that the rows are
autocorrelated and the term is + - * only (the device's l equals numpy's bit for bit).

``python tests/relative_eff_cases.py`` prints
* per input A, B, C: the range of the yardstick's r_eff_j, of the tail lengths and their distinct values, the smallest pair margin of the
  truncation rule, the smallest distance of ``3 sqrt(n / r_eff_j)`` from an integer and the columns truncated;
* the float64-to-longdouble distance of tests/psis_yardstick.py per output with a tail length per observation: on psis_cases.case(J,
  457) under SPREAD (r_eff_j spread over [0.3, 4]) and on input C under the yardstick's own r_eff_j -- the figures DIST of
  tests/test_gpu_relative_eff.py holds;
* whether the over-long input OVER (n = 25 000) asks for more than 4 096 draws by the yardstick's r_eff.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import convergence_yardstick as cy
import psis_cases as pc
import psis_yardstick as Y

# name: (walkers, samples, J, phi)
INPUTS = {"A": (4, 25, 65, 0.5),       # an odd n / nsel (the middle sample is left out); two groups, one live column in the second
          "B": (3, 150, 130, 0.8),     # more than one lag block
          "C": (4, 500, 130, 0.8)}     # the tail lengths really differ
OVER = (4, 6250, 3, 0.995)             # n = 25 000, strongly autocorrelated: 3 sqrt(n / r_eff_j) > 4096 asks for r_eff_j < 0.0134
SPREAD_JS = (65, 130)


def build(nw, ns, J, phi, seed):
    rng = np.random.default_rng(seed)
    a = cy.ar1(rng, phi, ns, nw, 2)                                                # [sample][walker][2]
    th = np.ascontiguousarray(np.stack([0.5 * a[:, :, 0], 1.0 + 0.1 * a[:, :, 1]], axis=2).transpose(1, 0, 2))
    D = rng.standard_normal((J, 1))
    l = pc.matrix(pc.rows_of(th), D)
    for x in (th, D, l):
        x.setflags(write=False)
    return th, D, l


@functools.lru_cache(maxsize=None)
def case(name):
    """``thetas[walker][sample][2]``, data ``[J][1]`` and the matrix ``l[n][J]`` (rows sample by sample, walkers ascending)."""
    nw, ns, J, phi = INPUTS[name]
    return build(nw, ns, J, phi, 7000 + ord(name))


@functools.lru_cache(maxsize=None)
def over_case():
    return build(*OVER, 7100)


def weights(l):
    """The series in float64, as the definition writes it: exp of the rounded difference."""
    with np.errstate(invalid="ignore"):
        return np.exp(l - l.max(axis=0))


def yardstick_reff(v, nw, split=True, max_lag=None):
    """(r_eff_j, the yardstick's stats, its raw arrays) of a series ``v[n][J]`` read as ``nw`` chains."""
    n, J = v.shape
    want, r = cy.convergence(v.reshape(n // nw, nw, J), split=split, max_lag=max_lag)
    return want["ess"] / (r["m"] * r["h"]), want, r


def tail_lengths(n, r_eff_j):
    return np.array([Y.tail_length(n, r if np.isfinite(r) and r > 0 else 1.0) for r in r_eff_j], dtype=np.int64)


def smallest_margin(want, r):
    out = math.inf
    max_lag = r["lagsum"].shape[1]
    for c in range(want["T"].size):
        upto = min(int(want["T"][c]) + 2, max_lag)
        if upto >= 3:
            out = min(out, float(cy.pair_margins(r["m"], r["h"], want["var_plus"][c:c + 1], r["lagsum"][c:c + 1], upto).min()))
    return out


def integer_distance(n, r_eff_j):
    x = 3.0 * np.sqrt(n / r_eff_j)
    x = x[x < 0.2 * n]                                                             # (where 0.2 n is the smaller the root does not decide)
    return float(np.min(np.abs(x - np.rint(x)))) if x.size else math.inf


def spread(J):
    """r_eff_j spread over [0.3, 4], in an order that is not monotone."""
    return np.random.default_rng(900 + J).permutation(np.geomspace(0.3, 4.0, J))


def loo_per_observation(l, Mj, longdouble=False, dropped=None):
    """tests/psis_yardstick.py's loo with the tail length ``Mj[j]`` for observation ``j``: dict ``pareto_k, elpd_loo_j``."""
    ft = np.longdouble if longdouble else np.float64
    cols = [Y.loo_column(l[:, j], int(Mj[j]), ft, dropped) for j in range(l.shape[1])]
    return {"pareto_k": np.array([c["k"] for c in cols], dtype=ft), "elpd_loo_j": np.array([c["elpd"] for c in cols], dtype=ft), "cols": cols}


def yardstick_distance(l, Mj):
    d64, d80 = [], []
    a, b = loo_per_observation(l, Mj, dropped=d64), loo_per_observation(l, Mj, True, dropped=d80)
    same = len(d64) == len(d80) and all((p == q).all() for p, q in zip(d64, d80))
    return {k: pc.rel(a[k], b[k]) for k in ("pareto_k", "elpd_loo_j")}, same


if __name__ == "__main__":
    for name, (nw, ns, J, phi) in INPUTS.items():
        l = case(name)[2]
        n = l.shape[0]
        r, want, raw = yardstick_reff(weights(l), nw)
        M = tail_lengths(n, r)
        print(f"{name}: r_eff_j {r.min():.3f} .. {r.max():.3f}, tail lengths {M.min()} .. {M.max()} ({np.unique(M).size} distinct; r_eff = 1 gives "
              f"{Y.tail_length(n)}), smallest pair margin {smallest_margin(want, raw):.2e}, 3 sqrt(n / r) from an integer {integer_distance(n, r):.2e}, "
              f"truncated {int(((want['flags'] & cy.TRUNCATED) != 0).sum())} of {J}, lag {want['T'].min()} .. {want['T'].max()}")
    for J in SPREAD_JS:
        l = pc.case(J, 457)[2]
        dist, same = yardstick_distance(l, tail_lengths(457, spread(J)))
        print(f'    ("spread", {J}): dict(' + ", ".join(f"{k}={v:.2e}" for k, v in dist.items()) + f"),    # same weights dropped: {same}")
    l = case("C")[2]
    r = yardstick_reff(weights(l), INPUTS["C"][0])[0]
    dist, same = yardstick_distance(l, tail_lengths(l.shape[0], r))
    print('    ("chain", "C"): dict(' + ", ".join(f"{k}={v:.2e}" for k, v in dist.items()) + f"),    # same weights dropped: {same}")
    l = over_case()[2]
    r = yardstick_reff(weights(l), OVER[0])[0]
    print(f"OVER: r_eff_j {r}, tail lengths {tail_lengths(l.shape[0], r)} (the limit is 4096)")
