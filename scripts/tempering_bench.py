"""Parallel tempering (kmc.Sampler(..., betas=...)) on one MI355X, in one process: the cost of the tempered launch against what it
replaces, and mixing on a two-mode target.

    python scripts/tempering_bench.py --out profiles/tempering.json

Per shape ntemps x nwalkers x ndim (8 x 512 x 8, 16 x 1 024 x 16, 8 x 8 192 x 32), unit Gaussian, stretch and DE, no chain: us per
half-step of the tempered launch (the sampler's own events over a run, best of three after a warm-up; the sweep node's share is the
difference between swap_every = 1 and swap_every = 0, per generation; with moments=True as well, where the sweep credits the
walkers that leave rung 0 with atomic adds) against
  (a) the untempered sampler at ntemps * nwalkers walkers x ndim forced onto the two-launch kernels (KMC_DEBUG=fused=0,no-resident),
      measured TWICE -- the same algorithmic bytes per launch, and kernels that are the parent commit's byte for byte
      (profiles/tempering_isa.txt); the spread of the two measurements is the noise the ratio is read against;
  (b) ntemps untempered samplers of nwalkers, run one after the other in their default mode: what a user does today.  One device
      event pair cannot span several samplers' streams, so (b) is timed with the HOST clock around run + sync, and its ratio is taken
      against the tempered run timed with the same host clock (host_us_per_half_step), not against the event time.
In the table graph the sweep is a node of every generation and leaves at once when it has no work: tempered_noswap (no chain, no
sweeps) carries 64 such empty nodes per replay, so tempered_over_flat includes them; their cost alone is not isolated.
Mixing: tau_int of rung 0's chain (kmc.int_acorr; parity unpinned: the reference's analysis.jl is commented out), the first
coordinate being the one the modes differ in, on the two-mode target of tests/test_gpu_tempering.py with and without
the ladder, and effective samples per second counting the whole ladder's cost.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 512, 8), (16, 1024, 16), (8, 8192, 32)]
TWO_MODES = ("double a = 0.0, b = 0.0; for (int i = 0; i < n; ++i) { const double m = (i == 0) ? p[0] : 0.0; a += (x[i] - m) * (x[i] - m); "
             "b += (x[i] + m) * (x[i] + m); } a = -0.5 * a; b = -0.5 * b; const double mx = a > b ? a : b; return mx + log(exp(a - mx) + exp(b - mx));")


def timed(kmc, nw, nd, move, gens, warm, **kw):
    import time
    th = np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, warm + 3 * gens, 0, 1, 2.0, 1, move=move, **kw) as s:
        s.set_positions(th)
        s.run(warm)
        s.sync()
        ms, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            s.run(gens)
            s.sync()
            host.append(time.perf_counter() - t0)
            ms.append(s.last_run_ms())
        desc = s.describe()
    return dict(us_per_half_step=min(ms) * 1e3 / (2 * gens), host_us_per_half_step=min(host) * 1e6 / (2 * gens), runs_ms=ms, describe=desc)


def separate(kmc, T, nw, nd, move, gens, warm):
    """T untempered samplers of nw walkers, one after the other, default mode: wall time of the T runs (host clock around run + sync)."""
    import time
    th = np.random.default_rng(0).standard_normal((nw, nd))
    ss = [kmc.Sampler(kmc.GaussianIso(), nw, nd, warm + 3 * gens, 0, 1, 2.0, 1 + t, move=move) for t in range(T)]
    try:
        for s in ss:
            s.set_positions(th)
            s.run(warm)
            s.sync()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            for s in ss:
                s.run(gens)
            for s in ss:
                s.sync()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        desc = ss[0].describe()
    finally:
        for s in ss:
            s.close()
    return dict(host_us_per_ladder_half_step=best * 1e6 / (2 * gens), clock="host (perf_counter around run + sync of all samplers)", describe=desc)


def two_mode_mixing(kmc, betas, gens, nburn, nw=256, d=10.0):
    r = np.random.default_rng(0)
    th = r.standard_normal((nw, 4))
    sign = np.where(np.arange(nw) < int(0.9 * nw), 1.0, -1.0)
    r.shuffle(sign)
    th[:, 0] += sign * d / 2
    kw = {} if betas is None else dict(betas=betas, swap_every=1)
    with kmc.Sampler(kmc.CDensity(TWO_MODES, params=[d / 2]), nw, 4, gens, nburn, 1, 2.0, 1000, store_chain=True, **kw) as s:
        s.set_positions(th)
        s.run(gens)
        s.sync()
        ms = s.last_run_ms()
        tau, _ = s.int_acorr()
        ch, _ = s.chain(logp=False)
    share = float(np.mean(ch[:, :, 0] > 0))
    return dict(tau_first_coordinate=float(tau[0]), tau_median=float(np.median(tau)), share_first_mode=share, run_ms=ms,
                ess_per_s_first_coordinate=nw * (gens - nburn) / float(tau[0]) / (ms * 1e-3 * (gens - nburn) / gens))


def adapt_figures(kmc, gens, shapes=((100, 3), (4096, 8)), T=8):
    """--adapt: HIP-event time per half-step of run() with 8 rungs, a sweep after every generation, the ladder fixed (`off`) and adapting
    all the way (`on`: nburnin = ngenerations, lag and time at their defaults): each a median of three runs with its spread.  The price of
    the counters and the ticket is on - off; `off` against the same figure of the parent commit's build says what the feature costs unused."""
    rows = []
    for nw, nd in shapes:
        row = dict(ntemps=T, nwalkers=nw, ndim=nd)
        for name, kw in (("off", {}), ("on", dict(adapt=True))):
            th = np.random.default_rng(0).standard_normal((nw, nd))
            G = gens // 4 + 3 * gens
            with kmc.Sampler(kmc.GaussianIso(), nw, nd, G, G, 1, 2.0, 1, betas=kmc.geometric_betas(T, 0.05), swap_every=1, **kw) as s:
                s.set_positions(th)
                s.run(gens // 4)
                s.sync()
                us = []
                for _ in range(3):
                    s.run(gens)
                    s.sync()
                    us.append(s.last_run_ms() * 1e3 / (2 * gens))
                row[name] = dict(us_per_half_step_median=float(np.median(us)), spread=float(max(us) - min(us)), runs=us, describe=s.describe())
        row["on_minus_off_us_per_generation"] = 2 * (row["on"]["us_per_half_step_median"] - row["off"]["us_per_half_step_median"])
        rows.append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "describe"}) for k, v in row.items()}), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adapt", action="store_true", help="only the adaptive ladder's figures (README \"Adaptive ladder\"); --out profiles/adaptive_ladder.json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempering.json"))
    ap.add_argument("--gens", type=int, default=1024)
    ap.add_argument("--mix-gens", type=int, default=20000)
    a = ap.parse_args()
    import kissmcmc_jl_amd as kmc
    if a.adapt:
        rec = dict(device="MI355X", density="GaussianIso(0, 1)", ladder="geometric_betas(8, 0.05), swap_every=1", whole_mode=adapt_figures(kmc, a.gens))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print("wrote", a.out)
        return
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", ladder="geometric_betas(ntemps, 0.05)", shapes=[])
    for T, nw, nd in SHAPES:
        betas = kmc.geometric_betas(T, 0.05)
        row = dict(ntemps=T, nwalkers=nw, ndim=nd)
        for name, mv in (("stretch", None), ("de", kmc.DEMove())):
            r = {}
            r["tempered_noswap"] = timed(kmc, nw, nd, mv, a.gens, a.gens // 4, betas=betas, swap_every=0)
            r["tempered_swap1"] = timed(kmc, nw, nd, mv, a.gens, a.gens // 4, betas=betas, swap_every=1)
            r["sweep_node_us_per_generation"] = 2 * (r["tempered_swap1"]["us_per_half_step"] - r["tempered_noswap"]["us_per_half_step"])
            r["tempered_swap1_moments"] = timed(kmc, nw, nd, mv, a.gens, a.gens // 4, betas=betas, swap_every=1, moments=True)
            r["tempered_noswap_moments"] = timed(kmc, nw, nd, mv, a.gens, a.gens // 4, betas=betas, swap_every=0, moments=True)
            r["sweep_node_us_per_generation_moments"] = 2 * (r["tempered_swap1_moments"]["us_per_half_step"] - r["tempered_noswap_moments"]["us_per_half_step"])
            os.environ["KMC_DEBUG"] = "fused=0,no-resident"
            r["flat_two_launch_a"] = timed(kmc, T * nw, nd, mv, a.gens, a.gens // 4)
            r["flat_two_launch_b"] = timed(kmc, T * nw, nd, mv, a.gens, a.gens // 4)
            del os.environ["KMC_DEBUG"]
            flat = [r["flat_two_launch_a"]["us_per_half_step"], r["flat_two_launch_b"]["us_per_half_step"]]
            r["flat_spread"] = abs(flat[0] - flat[1]) / min(flat)
            r["tempered_over_flat"] = r["tempered_noswap"]["us_per_half_step"] / min(flat)
            r["separate_samplers"] = separate(kmc, T, nw, nd, mv, a.gens, a.gens // 4)
            r["separate_over_tempered_host_clock"] = r["separate_samplers"]["host_us_per_ladder_half_step"] / r["tempered_noswap"]["host_us_per_half_step"]
            row[name] = r
            print(json.dumps({"shape": [T, nw, nd], "move": name, **{k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "describe"}) for k, v in r.items()}}), flush=True)
        rec["shapes"].append(row)
    rec["two_modes"] = dict(target="two unit Gaussians in 4-D, 10 apart; 256 walkers, 90 / 10 start; stretch move", generations=a.mix_gens,
                            tau="kmc.int_acorr (parity unpinned)",
                            plain=two_mode_mixing(kmc, None, a.mix_gens, a.mix_gens // 2),
                            ladder=two_mode_mixing(kmc, kmc.geometric_betas(6, 0.05), a.mix_gens, a.mix_gens // 2))
    print(json.dumps(rec["two_modes"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
