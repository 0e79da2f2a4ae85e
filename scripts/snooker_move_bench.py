"""The snooker move (kmc.DESnookerMove, KMC_MOVE_SNOOKER) and the 0.8 / 0.2 DE / snooker mixture (KMC_MOVE_MIX) against the stretch and
DE moves, in one process on one MI355X: cost per half-step, and mixing on the 32-D unit Gaussian.

    python scripts/snooker_move_bench.py --out profiles/snooker_move.json

Per shape (65 536 x 32 = C2, 16 384 x 64, 4 096 x 8), unit Gaussian, no chain: us per half-step of the four moves, timed as
scripts/de_move_bench.py times them (the sampler's own events, best of three runs after a warm-up), and the ratios against DE in
the same process -- the DE kernels' assembly is the parent commit's, byte for byte (profiles/snooker_isa.txt), so that IS the
parent's DE.  Derived bytes: one more partner row than DE, 8 ndim on DE's 24 ndim + 16 + acc (8 ndim + 12) per walker-step.
tau_int: the median integrated autocorrelation time of a `--mix-walkers` ensemble's chain, as de_move_bench.py measures it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from de_move_bench import mixing, timed  # noqa: E402

SHAPES = [(65536, 32), (16384, 64), (4096, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snooker_move.json"))
    ap.add_argument("--gens", type=int, default=400)
    ap.add_argument("--mix-gens", type=int, default=4000)
    ap.add_argument("--mix-burn", type=int, default=1000)
    ap.add_argument("--mix-walkers", type=int, default=4096)
    a = ap.parse_args()
    import kissmcmc_jl_amd as kmc
    moves = lambda: (("stretch", None), ("de", kmc.DEMove()), ("snooker", kmc.DESnookerMove()),
                     ("mixture", [(kmc.DEMove(), 0.8), (kmc.DESnookerMove(), 0.2)]))
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", de=dict(gamma0="2.38/sqrt(2 ndim)", sigma=1e-5), snooker=dict(gamma=1.7),
               mixture="0.8 DE + 0.2 snooker", shapes=[])
    for nw, nd in SHAPES:
        row = dict(nwalkers=nw, ndim=nd)
        for name, mv in moves():
            row[name] = timed(kmc, nw, nd, mv, a.gens, warm=a.gens // 4)
        for name in ("snooker", "mixture"):
            row[name + "_over_de_per_half_step"] = row[name]["us_per_half_step"] / row["de"]["us_per_half_step"]
        de_bytes = 24 * nd + 16 + row["de"]["accept"] * (8 * nd + 12)
        row["snooker_over_de_bytes_derived"] = (32 * nd + 16 + row["snooker"]["accept"] * (8 * nd + 12)) / de_bytes
        rec["shapes"].append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "describe"}) for k, v in row.items()}), flush=True)
    c2 = rec["shapes"][0]
    mix = dict(nwalkers=65536, ndim=32, tau_measured_with_nwalkers=a.mix_walkers, generations=a.mix_gens, nburnin=a.mix_burn)
    for name, mv in moves():
        m = mixing(kmc, a.mix_walkers, 32, mv, a.mix_gens, a.mix_burn)
        m["ess_per_s"] = 65536 * (1.0 / (2 * c2[name]["us_per_half_step"] * 1e-6)) / m["tau_median"]
        mix[name] = m
    rec["mixing_c2"] = mix
    print(json.dumps(mix), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
