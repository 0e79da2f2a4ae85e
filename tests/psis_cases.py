"""The inputs of the PSIS-LOO tests, hand-built and computed once, and the measurement of the yardstick's own error on them.

``python tests/psis_cases.py`` prints, per row count ``n`` of :data:`NS` and per output, the largest distance of the float64 yardstick
(tests/psis_yardstick.py) from its ``longdouble`` mode over the observation counts :data:`JS`, relative to ``max(1, |value|)``; it also
checks that the two modes drop the same weights at the ``10 eps`` threshold (an input where they disagree is not a test input) and
reports whether any are dropped.  tests/test_gpu_psis_loo.py holds the printed figures as named constants.  Needs no device.
"""
from __future__ import annotations

import functools

import numpy as np

import psis_yardstick as Y

# a normal log-density without its constant, + - * only: the device's terms equal numpy's bit for bit
TERM = "double z = (d[0] - x[0]) * x[1]; return -0.5 * z * z;"
INJECT_TERM = "return x[(int)d[0]];"              # data d_j = [j], ndim <= 32: l[r][j] = theta_r[j], any matrix the test writes
NS = [5, 24, 25, 30, 457, 7300]
JS = [1, 31, 63, 64, 65, 130]
OUTPUTS = ("pareto_k", "elpd_loo_j", "p_loo_j", "elpd_loo", "se", "p_loo")


def shape_of(n):
    """(walkers, samples) with walkers * samples == n, more than one walker where n allows."""
    for nw in (4, 3, 2):
        if n % nw == 0:
            return nw, n // nw
    return 1, n


def rows_of(th):
    """The rows of ``thetas[walker][sample][dim]`` in the library's order: sample by sample, walkers ascending."""
    return np.ascontiguousarray(th.transpose(1, 0, 2)).reshape(-1, th.shape[2])


def matrix(rows, D):
    z = (D[None, :, 0] - rows[:, None, 0]) * rows[:, None, 1]
    return -0.5 * z * z


@functools.lru_cache(maxsize=None)
def case(J, n):
    """``thetas[walker][sample][2]``, data ``[J][1]`` and the matrix ``l[n][J]`` for one shape; never written to."""
    rng = np.random.default_rng(100003 * J + n)
    nw, ns = shape_of(n)
    th = np.stack([0.5 * rng.standard_normal((nw, ns)), 1.0 + 0.1 * rng.standard_normal((nw, ns))], axis=2)
    D = rng.standard_normal((J, 1))
    l = matrix(rows_of(th), D)
    for a in (th, D, l):
        a.setflags(write=False)
    return th, D, l


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    scale = np.maximum(1.0, np.abs(b))
    both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    with np.errstate(invalid="ignore"):
        d = np.where(both_inf | (np.isnan(a) & np.isnan(b)), 0.0, np.abs(a - b) / scale)
    return float(np.max(d)) if d.size else 0.0


def yardstick_distance(l, r_eff=1.0):
    """Per output, the distance of the float64 yardstick from its longdouble mode on ``l``; and whether the two modes dropped the same
    weights, and whether any were dropped."""
    d64, d80 = [], []
    a, b = Y.loo(l, r_eff, dropped=d64), Y.loo(l, r_eff, longdouble=True, dropped=d80)
    same = len(d64) == len(d80) and all((p == q).all() for p, q in zip(d64, d80))
    return {k: rel(a[k], b[k]) for k in OUTPUTS}, same, any(p.any() for p in d64)


if __name__ == "__main__":
    for n in NS:
        worst, same_all, any_dropped = dict.fromkeys(OUTPUTS, 0.0), True, False
        for J in JS:
            dist, same, dropped = yardstick_distance(case(J, n)[2])
            worst = {k: max(worst[k], dist[k]) for k in OUTPUTS}
            same_all, any_dropped = same_all and same, any_dropped or dropped
        print(f"    {n}: dict(" + ", ".join(f"{k}={worst[k]:.2e}" for k in OUTPUTS) + f"),    # same weights dropped: {same_all}; any dropped: {any_dropped}")
