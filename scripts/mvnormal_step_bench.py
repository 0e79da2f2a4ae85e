"""What the covariance-shaped Metropolis proposal costs and what it buys (README: Covariance-shaped proposal).

    python scripts/mvnormal_step_bench.py [--parent-root DIR] [--shapes A,B] [--out profiles/mvnormal_step.json]

cost      per shape, `device_ms` (HIP events around the sampling kernels) of one run after one untimed run, in a child process each:
          GaussianStep on this build, GaussianStep on the parent commit's build (--parent-root: a checkout of the parent commit with
          its library built) and MVNormalStep with a dense L, by turns, three times; medians and spreads (max - min).
gain      MvNormal2 at correlation 0.95 and 0.999: tau_int (kmc.int_acorr, in steps) and effective samples per second of device time
          for the best isotropic GaussianStep of a five-point grid, MVNormalStep with the true covariance and TunedStep.
boundary  the cost of one tuning boundary (covariance kernels, copy, host Cholesky, upload): tune_ms / rounds of a TunedStep run.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"1048576x2": (1 << 20, 2, 2000), "65536x8": (65536, 8, 2000), "65536x32": (65536, 32, 1000), "4096x64": (4096, 64, 1000),
          "1x2": (1, 2, 100000), "64x8": (64, 8, 20000)}                     # (nchains, ndim, niter)
RHOS = (0.95, 0.999)
GRID = (1.0, 2.0, 4.0, 8.0, 16.0)                                           # x the narrow direction's standard deviation sqrt(1 - rho)


def factor(nd):
    rng = np.random.default_rng(nd)
    L = np.tril(rng.standard_normal((nd, nd)), -1) * (0.3 / nd)
    L[np.diag_indices(nd)] = 0.5 / np.sqrt(nd)
    return L


def one(mode, shape):
    sys.path.insert(0, ROOT)
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd.metropolis import run_chains
    nc, nd, niter = SHAPES[shape]
    th = np.random.default_rng(0).standard_normal((nc, nd))
    if mode == "gauss":
        step = kmc.GaussianStep(0.5 / np.sqrt(nd))
    elif mode == "mv":
        step = kmc.MVNormalStep(chol=factor(nd))
    else:
        step = kmc.TunedStep(kmc.GaussianStep(0.5 / np.sqrt(nd)), rounds=4)
    kw = dict(store_chain=False, store_logp=False)
    run_chains(kmc.GaussianIso(), step, th, niter, niter // 2, 1, 1, **kw)                   # untimed
    r = run_chains(kmc.GaussianIso(), step, th, niter, niter // 2, 1, 1, **kw)
    return dict(device_ms=r["device_ms"], tune_ms=r.get("tune_ms", 0.0), steps_per_s=nc * niter / (r["device_ms"] * 1e-3),
                accept=float(r["accept_ratio"].mean()))


def gain(rho):
    sys.path.insert(0, ROOT)
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd.metropolis import run_chains
    cov = np.array([[1.0, rho], [rho, 1.0]])
    pdf = kmc.MvNormal2([0.0, 0.0], cov)
    nc, niter, nburn, nthin = 1024, 42000, 2000, 20
    th = np.random.default_rng(1).multivariate_normal([0.0, 0.0], cov, nc)                  # started in the target: burn-in only tunes
    out = {}

    def measure(step):
        run_chains(pdf, step, th, 200, 100, 1, 5, store_logp=False)
        r = run_chains(pdf, step, th, niter, nburn, nthin, 5, store_logp=False, by_chain=True)
        tau, conv = kmc.int_acorr(r["chain"], warn=False)
        tau_steps = float(np.max(tau)) * nthin
        return dict(tau_int_steps=tau_steps, resolved=bool(np.min(conv) > 50), accept=float(r["accept_ratio"].mean()), device_ms=r["device_ms"],
                    ess_per_s=nc * (niter - nburn) / tau_steps / (r["device_ms"] * 1e-3))
    narrow = np.sqrt(1.0 - rho)
    grid = {f"{g}": measure(kmc.GaussianStep(g * narrow)) for g in GRID}
    best = min(grid, key=lambda k: grid[k]["tau_int_steps"])
    out["gaussian_grid"] = grid
    out["gaussian_best"] = dict(grid[best], scale_over_narrow_sd=float(best))
    out["mvnormal_true_cov"] = measure(kmc.MVNormalStep(cov=cov))
    out["tuned"] = measure(kmc.TunedStep(kmc.GaussianStep(narrow), rounds=4))
    return out


def child(root, *args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--one", *args], capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    global ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root")
    ap.add_argument("--shapes", help="comma-separated subset of the shapes (a repeat session)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvnormal_step.json"))
    a = ap.parse_args()
    if a.one:
        ROOT = os.path.abspath(a.root)                         # (the package under test: this checkout, or the parent's)
        print(json.dumps(gain(float(a.one[1])) if a.one[0] == "gain" else one(*a.one)))
        return
    stat = lambda v: dict(median=float(np.median(v)), spread=float(max(v) - min(v)), runs=v)
    rec = dict(device="MI355X", unit="device_ms: HIP events around the sampling kernels of one kmc_metropolis_run after one untimed run; "
               "median of three child processes, spread = max - min; the three configurations by turns",
               shapes={k: dict(nchains=v[0], ndim=v[1], niter=v[2]) for k, v in SHAPES.items()}, cost={}, boundary={}, gain={})
    only = a.shapes.split(",") if a.shapes else list(SHAPES)
    for shape, (nc, nd, niter) in SHAPES.items():
        if shape not in only:
            continue
        runs = dict(gauss=[], mv=[], gauss_parent=[])
        for _ in range(3):
            runs["gauss"].append(child(ROOT, "gauss", shape)["device_ms"])
            if a.parent_root:
                runs["gauss_parent"].append(child(a.parent_root, "gauss", shape)["device_ms"])
            runs["mv"].append(child(ROOT, "mv", shape)["device_ms"])
        r = {k: stat(v) for k, v in runs.items() if v}
        r["mv_over_gauss"] = r["mv"]["median"] / r["gauss"]["median"]
        # what the ratio should follow: ndim (ndim + 1) / 2 multiplies and adds on top of ceil((ndim + 2) / 4) Philox blocks and ndim / 2 Box-Muller pairs
        r["counts"] = dict(mul_add_pairs=nd * (nd + 1) // 2, philox_blocks=-(-(nd + 2) // 4), box_muller_pairs=(nd + 1) // 2)
        if a.parent_root:
            p = r["gauss_parent"]
            r["gauss_inside_parent_spread"] = bool(min(p["runs"]) <= r["gauss"]["median"] <= max(p["runs"]))
            r["gauss_minus_parent_ms"] = r["gauss"]["median"] - p["median"]
        rec["cost"][shape] = r
        print(shape, json.dumps(r), flush=True)
    for shape in ("65536x8", "65536x32"):
        if shape not in only:
            continue
        v = [child(ROOT, "tuned", shape) for _ in range(3)]
        rec["boundary"][shape] = dict(ms_per_boundary=stat([x["tune_ms"] / 4 for x in v]), run_device_ms=stat([x["device_ms"] for x in v]))
        print("boundary", shape, json.dumps(rec["boundary"][shape]), flush=True)
    for rho in RHOS:
        rec["gain"][str(rho)] = child(ROOT, "gain", str(rho))
        print("gain", rho, json.dumps({k: v for k, v in rec["gain"][str(rho)].items() if k != "gaussian_grid"}), flush=True)
    rec["not_measured"] = ["hardware counters", "a kernel trace", "ndim between 64 and 128", "runtime-compiled densities (ExprDensity, CDensity)",
                           "the host-density route"] + ([] if a.parent_root else ["GaussianStep on the parent commit's build (--parent-root)"])
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
