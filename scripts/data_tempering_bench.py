"""Likelihood tempering of a data density: the ladder's period per half-step against `ntemps` plain DataDensity samplers run one
after the other (what the library offered before), at S1 (100 x 3 over 10^3 observations) and S2 (4 096 x 8 over 10^5), 8 rungs; the
sweep node's period.  Writes profiles/data_tempering.json.

    python scripts/data_tempering_bench.py [--parent-root DIR] [--out profiles/data_tempering.json]
    python scripts/data_tempering_bench.py --one ladder|plain|sweep|adapt --shape S1|S2|W1|W2   (one figure as a JSON line: the child mode)
    python scripts/data_tempering_bench.py --adapt [--parent-root DIR] [--out profiles/adaptive_ladder.json]

--adapt: the adaptive ladder's price (README "Adaptive ladder").  Per shape -- S1, S2 in the likelihood mode and W1 (100 x 3), W2 (4 096 x 8)
in whole mode on GaussianIso, 8 rungs, a sweep after every generation -- the period with the ladder fixed (`off`) and adapting all the way
(`on`: nburnin = ngenerations), and with --parent-root `off` on the parent commit's build too: each a median of three child processes of
the same session, with its spread (max - min).

--parent-root: a checkout of the parent commit with its library built; the plain samplers are then ALSO timed there, in child
processes of the same session, three repetitions (their spread is the run-to-run spread the comparison is read against).  Kernel
shares come from a run of their own:  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/data_tempering_bench.py --one ladder --shape S1
Periods are HIP-event times of whole run() calls over the half-steps in them (launch gaps included), after a warm-up run."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"S1": dict(nw=100, nd=3, ndata=1000, G=400), "S2": dict(nw=4096, nd=8, ndata=100000, G=40)}
WHOLE = {"W1": dict(nw=100, nd=3, G=1024), "W2": dict(nw=4096, nd=8, G=1024)}      # --adapt only: whole mode, GaussianIso
NTEMPS = 8
TERM = "double mu = x[0]; for (int k = 1; k < n; ++k) mu += x[k] * d[k - 1]; double r = d[n - 1] - mu; return -0.5 * p[0] * r * r;"
PRIOR = "double s = 0.0; for (int k = 0; k < n; ++k) s += x[k] * x[k]; return -0.5 * s;"


def problem(kmc, sh):
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((sh["ndata"], sh["nd"] - 1))
    beta = np.linspace(0.5, -0.5, sh["nd"])
    y = beta[0] + Z @ beta[1:] + 0.5 * rng.standard_normal(sh["ndata"])
    dd = kmc.DataDensity(TERM, np.column_stack([Z, y]), prior=PRIOR, params=[4.0])
    return dd, beta + 0.05 * rng.standard_normal((sh["nw"], sh["nd"]))


def timed(s, th, G):
    s.set_positions(th)
    s.run(G)
    s.sync()                                                   # warm-up: modules loaded, clocks up
    s.run(G)
    s.sync()
    return s.last_run_ms() * 1e3 / (2 * G)                    # us per half-step


def one(kind, shape):
    sys.path.insert(0, ROOT)
    import kissmcmc_jl_amd as kmc
    kw = dict(adapt=True) if kind == "adapt" else {}          # (the parent commit's package is only asked for the other kinds)
    if shape in WHOLE:
        sh = WHOLE[shape]
        G, th = sh["G"], np.random.default_rng(0).standard_normal((sh["nw"], sh["nd"]))
        with kmc.Sampler(kmc.GaussianIso(), sh["nw"], sh["nd"], 3 * G, 3 * G, 1, 2.0, 5, betas=kmc.geometric_betas(NTEMPS, 0.05), swap_every=1, **kw) as s:
            return dict(kind=kind, shape=shape, us_per_half_step=timed(s, th, G), describe=s.describe())
    sh = SHAPES[shape]
    dd, th = problem(kmc, sh)
    G = sh["G"]
    if kind == "plain":                                        # ntemps samplers, one after the other: the sum of their periods
        us = 0.0
        for t in range(NTEMPS):
            with kmc.Sampler(dd, sh["nw"], sh["nd"], 3 * G, 0, 1, 2.0, 5 + t) as s:
                us += timed(s, th, G)
        return dict(kind=kind, shape=shape, us_per_half_step=us, one_sampler_us=us / NTEMPS)
    betas = kmc.geometric_betas(NTEMPS, 1e-3)
    # swap_every 0 and no stored samples: no sweep node; "sweep": a sweep after every generation, the difference is the node's period
    with kmc.Sampler(dd, sh["nw"], sh["nd"], 3 * G, 3 * G, 1, 2.0, 5, betas=betas, swap_every=1 if kind in ("sweep", "adapt") else 0, temper="likelihood", **kw) as s:
        us = timed(s, th, G)
        return dict(kind=kind, shape=shape, us_per_half_step=us, describe=s.describe())


def child(root, kind, shape):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, "--shape", shape, "--root", root],
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    global ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--shape", default="S1")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root")
    ap.add_argument("--adapt", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_tempering.json"))
    a = ap.parse_args()
    if a.one:
        ROOT = os.path.abspath(a.root)                         # (the package under test: this checkout, or the parent's)
        print(json.dumps(one(a.one, a.shape)))
        return
    if a.adapt:
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "adaptive_ladder.json")
        rec = dict(device="MI355X", ntemps=NTEMPS, shapes={**SHAPES, **WHOLE}, swap_every=1,
                   unit="us per half-step (HIP events over run(), launch gaps included); median of three child processes, spread = max - min", results={})
        stat = lambda v: dict(median=float(np.median(v)), spread=float(max(v) - min(v)), runs=v)
        for shape in list(WHOLE) + list(SHAPES):
            r = dict(off=stat([child(ROOT, "sweep", shape)["us_per_half_step"] for _ in range(3)]),
                     on=stat([child(ROOT, "adapt", shape)["us_per_half_step"] for _ in range(3)]))
            if a.parent_root:
                r["off_parent"] = stat([child(a.parent_root, "sweep", shape)["us_per_half_step"] for _ in range(3)])
                r["off_minus_parent"] = r["off"]["median"] - r["off_parent"]["median"]
            r["on_minus_off_us_per_generation"] = 2.0 * (r["on"]["median"] - r["off"]["median"])
            rec["results"][shape] = r
            print(shape, json.dumps(r), flush=True)
        if not a.parent_root:
            rec["not_measured"] = ["off on the parent commit's build (--parent-root)"]
        json.dump(rec, open(out, "w"), indent=1)
        return
    rec = dict(ntemps=NTEMPS, shapes=SHAPES, unit="us per half-step (HIP events over run(), launch gaps included)", results={})
    for shape in SHAPES:
        r = dict(ladder=child(ROOT, "ladder", shape), ladder_with_sweep=child(ROOT, "sweep", shape), plain_x8_head=[child(ROOT, "plain", shape)["us_per_half_step"] for _ in range(3)])
        r["sweep_node_us_per_generation"] = 2.0 * (r["ladder_with_sweep"]["us_per_half_step"] - r["ladder"]["us_per_half_step"])
        if a.parent_root:
            r["plain_x8_parent"] = [child(a.parent_root, "plain", shape)["us_per_half_step"] for _ in range(3)]
        base = r.get("plain_x8_parent", r["plain_x8_head"])
        r["plain_x8_spread"] = (max(base) - min(base)) / float(np.median(base))
        r["ladder_over_plain_x8"] = r["ladder"]["us_per_half_step"] / float(np.median(base))
        r["ladder_over_one_sampler"] = r["ladder"]["us_per_half_step"] / (float(np.median(base)) / NTEMPS)
        rec["results"][shape] = r
        print(shape, json.dumps({k: v for k, v in r.items() if k not in ("ladder", "ladder_with_sweep")}), flush=True)
    rec["not_measured"] = ["kernel shares (rocprofv3 --kernel-trace --stats), unless a kernel_shares entry was added by hand from such a run",
                           "graph capture of the data route", "ladders of other lengths than 8"]
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
