#!/usr/bin/env python
"""Marginal histograms on the device against the route a user had before them: profiles/corner.json.

Per shape (a menu Gaussian, chain stored on the device), in each of three child processes:
  device   Sampler.corner(bins=32) over the selected dimensions -- the default range, so the call holds one select of every column's
           minimum and maximum, the 1-D kernel and the 2-D kernel -- the same with the edges given (the two histogram kernels alone),
           and Sampler.histogram(bins=64) over every dimension; each after one untimed call;
  host     s.chain() followed by np.histogram per column and np.histogram2d per pair -- the yardstick: what the same tables cost
           without these calls, timed in the same process.
All are blocking calls; each is bracketed by HIP events (recorded on an otherwise idle stream, so their distance is the time the call
took, host work included) and by the host clock.  Reported: the median over the three processes with min / max, the bytes the two
histogram kernels read ((1 + pair groups) x padded chain: hist1d reads it once, hist2d once per group of pairs) and that byte count
per second, over the time of the call with the edges given, against the 6.29 TB/s a plain copy reaches on this card (README
"Measured").  The middle shape is run once more with every walker started at the same point: the chain is then one value repeated and
every element lands on one counter -- the contention case.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BPS = 6.29e12
B2, B1 = 32, 64
# (name, walkers, ndim, stored samples, selected dimensions of the corner (None: all), all walkers at one point)
CASES = [("65536x32x50", 65536, 32, 50, [0, 4, 9, 13, 18, 22, 27, 31], False), ("4096x8x2000", 4096, 8, 2000, None, False),
         ("100x3x10000", 100, 3, 10000, None, False), ("4096x8x2000-all-equal", 4096, 8, 2000, None, True)]


def bracket(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), (t1 - t0) * 1e3


def pair_groups(ndims, nbins):
    from kissmcmc_jl_amd import _lib
    ppg, ng, lds = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().kmc_hist_pair_plan(ndims, nbins, C.byref(ppg), C.byref(ng), C.byref(lds)))
    return ppg.value, ng.value, lds.value


def child(idx):
    import kissmcmc_jl_amd as kmc
    name, nw, nd, ns, dims, equal = CASES[idx]
    nburn = 20
    th = np.zeros((nw, nd)) if equal else np.random.default_rng(0).standard_normal((nw, nd))
    sel = list(range(nd)) if dims is None else dims
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        run_ms = s.last_run_ms()
        edges = s.corner(bins=B2, dims=dims)["edges"]
        s.corner(bins=edges, dims=dims)
        s.histogram(bins=B1)
        cd, c_ev, c_wall = bracket(lambda: s.corner(bins=B2, dims=dims))
        ce, ce_ev, ce_wall = bracket(lambda: s.corner(bins=edges, dims=dims))
        (h1, e1, o1), h_ev, h_wall = bracket(lambda: s.histogram(bins=B1))

        def host_corner():
            ch = s.chain(logp=False)[0].reshape(-1, nd)
            one = [np.histogram(ch[:, d], bins=B2) for d in sel]
            two = [np.histogram2d(ch[:, sel[a]], ch[:, sel[b]], bins=[one[a][1], one[b][1]])[0]
                   for a in range(len(sel)) for b in range(a + 1, len(sel))]
            return one, two

        (one, two), hc_ev, hc_wall = bracket(host_corner)

        def host_hist():
            ch = s.chain(logp=False)[0].reshape(-1, nd)
            return [np.histogram(ch[:, d], bins=B1) for d in range(nd)]

        hh, hh_ev, hh_wall = bracket(host_hist)
    agree = bool(all(np.array_equal(cd["hist1d"][i], one[i][0]) and np.array_equal(cd["edges"][i], one[i][1]) for i in range(len(sel))) and
                 all(np.array_equal(cd["hist2d"][k], two[k]) for k in range(len(two))) and np.array_equal(ce["hist2d"], cd["hist2d"]) and
                 all(np.array_equal(h1[d], hh[d][0]) and np.array_equal(e1[d], hh[d][1]) for d in range(nd)))
    print("RESULT " + json.dumps(dict(case=name, sampling_ms=run_ms, device_corner_ms=c_ev, device_corner_wall_ms=c_wall,
                                      device_corner_given_edges_ms=ce_ev, device_corner_given_edges_wall_ms=ce_wall, device_histogram_ms=h_ev,
                                      device_histogram_wall_ms=h_wall, host_corner_ms=hc_ev, host_corner_wall_ms=hc_wall, host_histogram_ms=hh_ev,
                                      host_histogram_wall_ms=hh_wall, device_equals_host=agree)), flush=True)


def spread(vals):
    return dict(median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corner.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child)
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", corner_bins=B2, histogram_bins=B1, copy_bytes_per_s=COPY_BPS,
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max)" % a.repeats,
               yardstick="s.chain() + np.histogram per column / np.histogram2d per pair on the host, same process", cases=[])
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, ns, dims, equal = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(idx)], stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:                     # a fault: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        nsel = nd if dims is None else len(dims)
        ppg, ngroups, lds = pair_groups(nsel, B2)
        chain_bytes = ns * nw * (nd + nd % 2) * 8                         # what one read of the selection moves: padded rows
        row = dict(case=name, nwalkers=nw, ndim=nd, nsamples=ns, corner_dims=nsel, pairs=nsel * (nsel - 1) // 2, pairs_per_group=ppg,
                   pair_groups=ngroups, lds_budget=lds, all_equal=equal, chain_bytes=chain_bytes, corner_bytes=(1 + ngroups) * chain_bytes,
                   device_equals_host=all(r["device_equals_host"] for r in runs))
        for k in runs[0]:
            if k.endswith("_ms"):
                row[k] = spread([r[k] for r in runs])
        row["corner_bytes_per_s"] = row["corner_bytes"] / (row["device_corner_given_edges_ms"]["median"] * 1e-3)
        row["corner_fraction_of_copy_rate"] = row["corner_bytes_per_s"] / COPY_BPS
        row["histogram_bytes_per_s"] = chain_bytes / (row["device_histogram_ms"]["median"] * 1e-3)     # (its range select not counted in the bytes)
        row["host_over_device_corner"] = row["host_corner_ms"]["median"] / row["device_corner_ms"]["median"]
        row["host_over_device_histogram"] = row["host_histogram_ms"]["median"] / row["device_histogram_ms"]["median"]
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
