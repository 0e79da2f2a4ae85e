#!/usr/bin/env python
"""Highest-density intervals on the device against the routes there were before: profiles/hdi.json.

Per shape (a menu Gaussian, chain stored on the device; the three shapes of the rank-convergence table), in each of three child
processes, every call blocking and bracketed by HIP events after one untimed call:
  device   Sampler.hdi(0.94) and Sampler.hdi(sixteen probabilities): gather, one segmented radix sort, the scan and its fold;
  host     s.chain(), then np.sort and the window minimum per column in numpy -- the route there was before;
  torch    torch.sort along the column axis of the same [ncols, N] double tensor on the device, plus the window minimum in torch.
Reported: the median over the processes with min / max; the library's own stage times (gather, sort, scan + fold) of both calls; the
bytes the scan loads as the library counts them, per second of the scan stage, against the 6.29 TB/s plain-copy rate.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from convergence_bench import CASES, bracket, spread                               # noqa: E402

COPY_RATE = 6.29e12
PROBS16 = [0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.68, 0.7, 0.8, 0.89, 0.9, 0.94, 0.95, 0.99, 0.999]


def host_route(chain, p):
    """lo, hi [ncols] from a chain [sample][walker][dim] in host memory, in numpy."""
    ns, nw, nd = chain.shape
    n = ns * nw
    k = int(np.floor(p * n))
    lo, hi = np.empty(nd), np.empty(nd)
    for c in range(nd):
        xs = np.sort(chain[:, :, c].ravel() + 0.0)
        i = int(np.argmin(xs[k:] - xs[:n - k]))
        lo[c], hi[c] = xs[i], xs[i + k]
    return lo, hi


def child(idx, with_host=True):
    import torch

    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd.summary import _SamplerProvider, hdi_from
    name, nw, nd, ns = CASES[idx]
    nburn = 20
    th = np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        s.hdi(0.94)
        one, one_ev, one_wall = bracket(lambda: s.hdi(0.94))
        s.hdi(PROBS16)
        many, many_ev, _ = bracket(lambda: s.hdi(PROBS16))
        info1 = hdi_from(_SamplerProvider(s), 0.94, with_info=True)["info"]
        info16 = hdi_from(_SamplerProvider(s), PROBS16, with_info=True)["info"]
        chain = s.chain(logp=False)[0]
        if with_host:
            (hlo, hhi), h_ev, h_wall = bracket(lambda: host_route(s.chain(logp=False)[0], 0.94))
    n, k = one["n"], one["k"]
    cols = torch.from_numpy(np.ascontiguousarray(chain.reshape(-1, nd).T)).cuda()

    def torch_route():
        xs = torch.sort(cols, dim=1).values
        i = torch.argmin(xs[:, k:] - xs[:, :n - k], dim=1)
        r = torch.arange(nd, device=cols.device)
        out = xs[r, i].cpu(), xs[r, i + k].cpu()
        torch.cuda.synchronize()
        return out
    torch_route()
    (tlo, thi), t_ev, _ = bracket(torch_route)
    _, ts_ev, _ = bracket(lambda: (torch.sort(cols, dim=1), torch.cuda.synchronize()))
    agree_torch = bool(np.array_equal(tlo.numpy(), one["lo"]) and np.array_equal(thi.numpy(), one["hi"]))
    agree_host = bool(np.array_equal(hlo, one["lo"]) and np.array_equal(hhi, one["hi"])) if with_host else None
    agree_16 = bool(np.array_equal(many["lo"][PROBS16.index(0.94)], one["lo"]))
    print("RESULT " + json.dumps(dict(
        case=name, device_ms=one_ev, device_wall_ms=one_wall, device16_ms=many_ev, host_ms=h_ev if with_host else None,
        host_wall_ms=h_wall if with_host else None, torch_ms=t_ev, torch_sort_ms=ts_ev,
        gather_ms=info1[3] * 1e-6, sort_ms=info1[4] * 1e-6, scan_ms=info1[5] * 1e-6,
        gather16_ms=info16[3] * 1e-6, sort16_ms=info16[4] * 1e-6, scan16_ms=info16[5] * 1e-6,
        n=int(n), k=int(k), tiles=int(info1[1]), scan_bytes=int(info1[2]), scan16_bytes=int(info16[2]),
        device_equals_host=agree_host, device_equals_torch=agree_torch, sixteen_equals_one=agree_16)), flush=True)


def derive(row):
    row["scan_bytes_per_s"] = row["scan_bytes"] / (row["scan_ms"]["median"] * 1e-3)
    row["scan_of_copy_rate"] = row["scan_bytes_per_s"] / COPY_RATE
    row["scan16_bytes_per_s"] = row["scan16_bytes"] / (row["scan16_ms"]["median"] * 1e-3)
    row["scan16_of_copy_rate"] = row["scan16_bytes_per_s"] / COPY_RATE
    dev = row["device_ms"]["median"]
    row["sort_share_of_call"] = row["sort_ms"]["median"] / dev
    row["host_over_device"] = None if row["host_ms"] is None else row["host_ms"]["median"] / dev
    row["torch_over_device"] = row["torch_ms"]["median"] / dev
    row["sort_over_torch_sort"] = row["sort_ms"]["median"] / row["torch_sort_ms"]["median"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdi.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--skip-host", action="store_true", help="leave the numpy route out: its columns are then null")
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child, not a.skip_host)
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", call="Sampler.hdi(0.94) and Sampler.hdi(sixteen probabilities), every stored draw",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max); "
                      "stage times: the library's own events (info of kmc_sampler_hdi)" % a.repeats,
               yardsticks="host: s.chain() + np.sort + the window minimum per column; torch: torch.sort(dim=1) of the [ncols, N] doubles + the window minimum in torch",
               probs16=PROBS16, copy_rate=COPY_RATE, cases=[])
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, ns = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", str(idx)] +
                               (["--skip-host"] if a.skip_host else []), stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:                     # a fault or a time limit: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print(f"{name}: process {len(runs)} of {a.repeats} done", flush=True)
        r0 = runs[0]
        row = dict(case=name, nwalkers=nw, ndim=nd, nsamples=ns)
        for key in ("n", "k", "tiles", "scan_bytes", "scan16_bytes"):
            row[key] = r0[key]
        for key in ("device_equals_host", "device_equals_torch", "sixteen_equals_one"):
            row[key] = None if r0[key] is None else all(r[key] for r in runs)
        for key in r0:
            if key.endswith("_ms"):
                row[key] = None if r0[key] is None else spread([r[key] for r in runs])
        derive(row)
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
