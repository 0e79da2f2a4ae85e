"""The differential-evolution move (kmc.DEMove, KMC_MOVE_DE) against the stretch move, in one process on one MI355X: cost per
half-step, and mixing per second.

    python scripts/de_move_bench.py --out profiles/de_move.json

Per shape (65 536 x 32 = C2, 16 384 x 64, 4 096 x 8, the README's 100 x 1), unit Gaussian, no chain: us per half-step and walker-steps/s
of both moves, timed by the sampler's own events over `--gens` generations after a warm-up.  Algorithmic bytes of a DE walker-step:
the own row and two partner rows read (3 x 8 ndim), the log-pdf read (8), naccept / klast (8), the accepted row and its log-pdf and
counter written (acc x (8 ndim + 12)); the roofline fraction prices the C2 half-step against the 8 TB/s HBM spec.  Mixing on the 32-D
unit Gaussian: the median integrated autocorrelation time (in generations) of the stored chain of a `--mix-walkers` ensemble
(kmc_sampler_int_acorr; its FFT plan for all 65 536 x 32 series of a C2 chain does not fit the device), and at C2's size
ESS/s = 65 536 x generations/s / tau -- tau is a property of the move and the dimension once nwalkers >> ndim.
With hipcc at hand, the VGPRs and scratch of the DE vector kernel at C2's geometry from `--save-temps`.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BPS = 8.0e12      # MI355X HBM3E spec (MI355X_MICROARCH.md)
SHAPES = [(65536, 32), (16384, 64), (4096, 8), (100, 1)]


def timed(kmc, nw, nd, move, gens, warm, seed=1):
    th = np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, warm + 3 * gens, 0, 1, 2.0, seed, move=move) as s:
        s.set_positions(th)
        s.run(warm)
        s.sync()
        ms = []
        for _ in range(3):
            s.run(gens)
            s.sync()
            ms.append(s.last_run_ms())
        acc = float(s.naccept().sum()) / (nw * (warm + 3 * gens))
        desc = s.describe()
    best = min(ms)
    return dict(us_per_half_step=best * 1e3 / (2 * gens), walker_steps_per_s=nw * gens / (best * 1e-3), runs_ms=ms, accept=acc, describe=desc)


def mixing(kmc, nw, nd, move, gens, nburn, seed=7):
    th = np.random.default_rng(3).standard_normal((nw, nd))      # the target itself: stationary from the start
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, gens, nburn, 1, 2.0, seed, store_chain=True, move=move) as s:
        s.set_positions(th)
        s.run(gens)
        s.sync()
        tau, conv = s.int_acorr()
    return dict(tau_median=float(np.median(tau)), tau_max=float(np.max(tau)), nsamples=gens - nburn, converged_min=float(np.min(conv)))


def isa_stats():
    """VGPRs / scratch of half_step_de_vec<GaussianIso, 8, 2, ITER, exact> (C2's geometry) from hipcc --save-temps."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    sys.path.insert(0, os.path.join(ROOT, "kissmcmc.jl_amd"))
    import build as kb
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call([hipcc, *kb.FLAGS, *kb.PRELOAD, "--save-temps", "-c", os.path.join(kb.CSRC, "kmc_inst_gaussian_iso_de.hip"), "-o",
                               os.path.join(d, "de.o")], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = open(os.path.join(d, "kmc_inst_gaussian_iso_de-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    out = {}
    for blk in s.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN3kmc16half_step_de_vecINS_11GaussianIsoELi8ELi2ELi(\d+)ELb0E", name)
        if m:
            out[f"L8_K2_ITER{m.group(1)}"] = dict(vgpr=int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                                                scratch_bytes=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "de_move.json"))
    ap.add_argument("--gens", type=int, default=400)
    ap.add_argument("--mix-gens", type=int, default=4000)
    ap.add_argument("--mix-burn", type=int, default=1000)
    ap.add_argument("--mix-walkers", type=int, default=4096)
    ap.add_argument("--no-isa", action="store_true")
    a = ap.parse_args()
    import kissmcmc_jl_amd as kmc
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", de=dict(gamma0="2.38/sqrt(2 ndim)", sigma=1e-5), shapes=[])
    for nw, nd in SHAPES:
        gens = a.gens if nw * nd >= 65536 else 4 * a.gens
        row = dict(nwalkers=nw, ndim=nd)
        for name, mv in (("stretch", None), ("de", kmc.DEMove())):
            row[name] = timed(kmc, nw, nd, mv, gens, warm=gens // 4)
        row["de_over_stretch_per_half_step"] = row["de"]["us_per_half_step"] / row["stretch"]["us_per_half_step"]
        acc = row["de"]["accept"]
        row["de_bytes_per_walker_step"] = 24 * nd + 16 + acc * (8 * nd + 12)
        row["de_roofline_fraction"] = row["de_bytes_per_walker_step"] * row["de"]["walker_steps_per_s"] / HBM_PEAK_BPS
        rec["shapes"].append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "describe"}) for k, v in row.items()}), flush=True)
    nw, nd = 65536, 32
    c2 = rec["shapes"][0]
    mix = dict(nwalkers=nw, ndim=nd, tau_measured_with_nwalkers=a.mix_walkers, generations=a.mix_gens, nburnin=a.mix_burn)
    for name, mv in (("stretch", None), ("de", kmc.DEMove())):
        m = mixing(kmc, a.mix_walkers, nd, mv, a.mix_gens, a.mix_burn)
        gens_per_s = 1.0 / (2 * c2[name]["us_per_half_step"] * 1e-6)
        m["ess_per_s"] = nw * gens_per_s / m["tau_median"]
        mix[name] = m
    mix["de_over_stretch_ess_per_s"] = mix["de"]["ess_per_s"] / mix["stretch"]["ess_per_s"]
    rec["mixing_c2"] = mix
    print(json.dumps(mix), flush=True)
    if not a.no_isa:
        rec["de_vec_isa_c2_geometry"] = isa_stats()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
