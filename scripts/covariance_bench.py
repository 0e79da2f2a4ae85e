#!/usr/bin/env python
"""The posterior covariance on the device against the routes there were before it: profiles/covariance.json.

Per shape (a menu Gaussian, chain stored on the device), in each of three child processes:
  device   Sampler.covariance(): the column sums, the centred cross products on the matrix instruction, the two folds, the host stage;
           after one untimed call;
  host     s.chain() followed by np.cov on the host -- the route a user had: what the same matrix cost without this call;
  torch    torch.cov on the same doubles already on the device (the upload is not timed; one untimed call first): what a general
           library's matrix product makes of the same sum.
All are blocking calls; each is bracketed by HIP events (recorded on an otherwise idle stream, so their distance is the time the call
took, host work included) and by the host clock.  Reported: the median over the three processes with min / max; the rows walked, the
partial sums per entry, the strips and the bytes of the chain the kernels loaded (counted by the library from the shapes: selected rows
x the columns of every tile a stage reads x element size), and that byte count per second of the whole call against the device's copy
rate on record.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, walkers, ndim, stored samples); the last needs several strips
CASES = [("65536x32x50", 65536, 32, 50), ("4096x8x2000", 4096, 8, 2000), ("100x3x10000", 100, 3, 10000), ("4096x128x100", 4096, 128, 100)]
COPY_RATE = 6.29e12            # bytes per second: the device-to-device copy rate on record
CHILD_TIMEOUT = 420            # seconds


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


def child(idx):
    import torch
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import chain_covariance, summary
    name, nw, nd, ns = CASES[idx]
    nburn = 20
    th = np.random.default_rng(0).standard_normal((nw, nd))
    with kmc.Sampler(kmc.GaussianIso(), nw, nd, nburn + ns, nburn, 1, 2.0, 3, store_chain=True) as s:
        s.set_positions(th)
        s.run(nburn + ns)
        s.sync()
        run_ms = s.last_run_ms()
        s.covariance()
        dev, d_ev, d_wall = bracket(lambda: s.covariance())
        info = chain_covariance.covariance_raw_from(summary._SamplerProvider(s))["info"]
        ref, h_ev, h_wall = bracket(lambda: np.cov(s.chain(logp=False)[0].reshape(-1, nd), rowvar=False))
        x = torch.from_numpy(s.chain(logp=False)[0].reshape(-1, nd)).cuda()

    def torch_cov():
        c = torch.cov(x.T)
        torch.cuda.synchronize()
        return c

    torch_cov()
    tc, t_ev, t_wall = bracket(torch_cov)
    ref = ref.reshape(nd, nd)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    err = float(np.max(np.abs(dev["cov"] - ref) / scale))
    err_torch = float(np.max(np.abs(tc.cpu().numpy().reshape(nd, nd) - ref) / scale))
    print("RESULT " + json.dumps(dict(case=name, sampling_ms=run_ms, device_ms=d_ev, device_wall_ms=d_wall, host_ms=h_ev, host_wall_ms=h_wall,
                                      torch_ms=t_ev, torch_wall_ms=t_wall, rows=int(info[0]), partials=int(info[1]), strips=int(info[2]),
                                      bytes_loaded=int(info[3]), n=int(dev["n"]), max_err_vs_numpy=err, torch_max_err_vs_numpy=err_torch)), flush=True)


def spread(vals):
    return dict(median=float(np.median(vals)), min=float(min(vals)), max=float(max(vals)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance.json"))
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(str(i) for i in range(len(CASES))))
    a = ap.parse_args()
    if a.child >= 0:
        return child(a.child)
    rec = dict(device="MI355X", density="GaussianIso(0, 1)", call="Sampler.covariance(): every stored sample of every walker, the dimensions only",
               timing="HIP events around each blocking call, one untimed call first; median of %d child processes (min, max)" % a.repeats,
               yardsticks="host: s.chain() + np.cov, same process; torch: torch.cov of the same doubles on the device, upload not timed",
               form="the matrix-instruction form (v_mfma_f64_16x16x4_f64); a plain-FMA form was not built, so there is no second number",
               copy_rate_bytes_per_s=COPY_RATE, cases=[])
    if os.path.exists(a.out) and a.cases != ",".join(str(i) for i in range(len(CASES))):      # a run over some of the cases adds to the file
        with open(a.out) as f:
            old = json.load(f)
        rec["cases"] = [c for c in old.get("cases", []) if c["case"] not in {CASES[int(v)][0] for v in a.cases.split(",")}]
    for idx in (int(v) for v in a.cases.split(",")):
        name, nw, nd, ns = CASES[idx]
        runs = []
        for _ in range(a.repeats):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(idx)], stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT)
            if p.returncode != 0:                     # a fault: nothing more is started on the device
                raise SystemExit(f"child for {name} ended with status {p.returncode}")
            runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        r0 = runs[0]
        row = dict(case=name, nwalkers=nw, ndim=nd, nsamples=ns, chain_bytes=ns * nw * (nd + nd % 2) * 8)
        for k in ("n", "rows", "partials", "strips", "bytes_loaded"):
            row[k] = r0[k]
        for k in r0:
            if k.endswith("_ms"):
                row[k] = spread([r[k] for r in runs])
        row["max_err_vs_numpy"] = max(r["max_err_vs_numpy"] for r in runs)
        row["torch_max_err_vs_numpy"] = max(r["torch_max_err_vs_numpy"] for r in runs)
        row["bytes_per_s"] = row["bytes_loaded"] / (row["device_ms"]["median"] * 1e-3)
        row["share_of_copy_rate"] = row["bytes_per_s"] / COPY_RATE
        row["host_over_device"] = row["host_ms"]["median"] / row["device_ms"]["median"]
        row["torch_over_device"] = row["torch_ms"]["median"] / row["device_ms"]["median"]
        rec["cases"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
