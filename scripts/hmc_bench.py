"""What the HMC step of the many-chain Metropolis sampler costs and what it buys (README: Hamiltonian Monte Carlo step).

    python scripts/hmc_bench.py [--parent-root DIR] [--only cost,gain,price] [--out profiles/hmc_step.json]

cost   GaussianIso at 65 536 x 8 and 65 536 x 32: `device_ms` (HIP events around the sampling kernels) of one run after one untimed run, in a
       child process each, for GaussianStep and for HMCStep with nleap in {1, 4, 16}, by turns, three times; medians and spreads
       (max - min); time per iteration and chain, per gradient evaluation (nleap + 1 of them an iteration: kmc_hmc.hpp computes the
       gradient at the current state anew) and per leapfrog step.
gain   a 32-D GaussianIso(0, 1) and the 2-D Rosenbrock(1, 100, 20): tau_int (kmc.int_acorr, in iterations) and effective samples per
       second of device time for a hand-picked HMCStep and for the best GaussianStep of a five-point grid of scales; three child
       processes (the same seeds: the chains are the same, the device times are not), medians and spreads.
price  what the feature costs the existing kernels: GaussianStep and MVNormalStep at the six shapes of the README's MVNormalStep table,
       this build against the parent commit's (--parent-root: a checkout of the parent commit with its library built), by turns,
       three times; whether this build's median lies inside the parent's own run-to-run spread.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COST_SHAPES = {"65536x8": (65536, 8, 400), "65536x32": (65536, 32, 200)}    # (nchains, ndim, niter)
NLEAPS = (1, 4, 16)
PRICE_SHAPES = {"1048576x2": (1 << 20, 2, 2000), "65536x8": (65536, 8, 2000), "65536x32": (65536, 32, 1000), "4096x64": (4096, 64, 1000),
                "1x2": (1, 2, 100000), "64x8": (64, 8, 20000)}
GAIN = {"gaussian32": dict(ndim=32, nchains=256, hmc=dict(eps=0.4, nleap=4, jitter=0.3), grid=(0.21, 0.3, 0.42, 0.6, 0.85),
                           rw=dict(niter=42000, nburnin=2000, nthin=20), hm=dict(niter=4000, nburnin=1000, nthin=1)),
        "rosenbrock2": dict(ndim=2, nchains=1024, hmc=dict(eps=0.1, nleap=16, jitter=0.3), grid=(0.25, 0.5, 1.0, 2.0, 4.0),
                            rw=dict(niter=82000, nburnin=2000, nthin=40), hm=dict(niter=8000, nburnin=2000, nthin=3))}


def factor(nd):
    rng = np.random.default_rng(nd)
    L = np.tril(rng.standard_normal((nd, nd)), -1) * (0.3 / nd)
    L[np.diag_indices(nd)] = 0.5 / np.sqrt(nd)
    return L


def one(mode, shape):
    sys.path.insert(0, ROOT)
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd.metropolis import run_chains
    nc, nd, niter = (COST_SHAPES if mode.startswith("hmc") or mode == "gauss-cost" else PRICE_SHAPES)[shape]
    th = np.random.default_rng(0).standard_normal((nc, nd))
    if mode.startswith("hmc"):
        step = kmc.HMCStep(0.5 / nd ** 0.25, nleap=int(mode[3:]), jitter=0.2)
    elif mode == "mv":
        step = kmc.MVNormalStep(chol=factor(nd))
    else:
        step = kmc.GaussianStep(0.5 / np.sqrt(nd))
    kw = dict(store_chain=False, store_logp=False)
    run_chains(kmc.GaussianIso(), step, th, niter, niter // 2, 1, 1, **kw)                   # untimed
    r = run_chains(kmc.GaussianIso(), step, th, niter, niter // 2, 1, 1, **kw)
    return dict(device_ms=r["device_ms"], accept=float(r["accept_ratio"].mean()))


def gain(name):
    sys.path.insert(0, ROOT)
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd.metropolis import run_chains
    g = GAIN[name]
    nc, nd = g["nchains"], g["ndim"]
    rng = np.random.default_rng(1)
    if name == "gaussian32":
        pdf, th = kmc.GaussianIso(0.0, 1.0), rng.standard_normal((nc, nd))
    else:
        pdf, th = kmc.Rosenbrock(1.0, 100.0, 20.0), np.array([1.0, 1.0]) + 0.1 * rng.standard_normal((nc, nd))

    def measure(step, niter, nburnin, nthin):
        run_chains(pdf, step, th, 200, 100, 1, 5, store_logp=False)
        r = run_chains(pdf, step, th, niter, nburnin, nthin, 5, store_logp=False, by_chain=True)
        tau, conv = kmc.int_acorr(r["chain"], warn=False)
        tau_it = float(np.max(tau)) * nthin
        return dict(tau_int_iterations=tau_it, resolved=bool(np.min(conv) > 50), accept=float(r["accept_ratio"].mean()), device_ms=r["device_ms"],
                    niter=niter, nthin=nthin, ess_per_s=nc * (niter - nburnin) / tau_it / (r["device_ms"] * 1e-3))
    grid = {f"{s}": measure(kmc.GaussianStep(s), **g["rw"]) for s in g["grid"]}
    best = max(grid, key=lambda k: grid[k]["ess_per_s"])
    hmc = measure(kmc.HMCStep(**g["hmc"]), **g["hm"])
    hmc["gradients_per_independent_draw"] = hmc["tau_int_iterations"] * (g["hmc"]["nleap"] + 1)
    return dict(gaussian_grid=grid, gaussian_best=dict(grid[best], scale=float(best)), hmc=dict(hmc, **g["hmc"]),
                ess_per_s_hmc_over_gaussian=hmc["ess_per_s"] / grid[best]["ess_per_s"])


def child(root, *args):
    env = dict(os.environ, KMC_DEBUG="no-torch-preload")             # (nothing here uses torch; its import is most of a child's start)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--one", *args], capture_output=True, text=True, env=env)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    global ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root")
    ap.add_argument("--only", default="cost,gain,price")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmc_step.json"))
    a = ap.parse_args()
    if a.one:
        ROOT = os.path.abspath(a.root)                         # (the package under test: this checkout, or the parent's)
        print(json.dumps(gain(a.one[1]) if a.one[0] == "gain" else one(*a.one)))
        return
    only = a.only.split(",")
    stat = lambda v: dict(median=float(np.median(v)), spread=float(max(v) - min(v)), runs=v)
    rec = dict(device="MI355X", unit="device_ms: HIP events around the sampling kernels of one kmc_metropolis_run after one untimed run; "
               "median of three child processes, spread = max - min; the configurations of a shape by turns", cost={}, gain={}, price={})
    if os.path.exists(a.out):                                    # (a repeat session of one part keeps the others)
        old = json.load(open(a.out))
        rec.update({k: old[k] for k in ("cost", "gain", "price") if k in old and k not in only})
    if "cost" in only:
        for shape, (nc, nd, niter) in COST_SHAPES.items():
            modes = ["gauss-cost"] + [f"hmc{n}" for n in NLEAPS]
            runs = {m: [] for m in modes}
            acc = {}
            for _ in range(3):
                for m in modes:
                    c = child(ROOT, m, shape)
                    runs[m].append(c["device_ms"])
                    acc[m] = c["accept"]
            r = dict(nchains=nc, ndim=nd, niter=niter)
            ns = lambda ms: ms * 1e6 / (nc * niter)              # ns per chain and iteration
            r["gaussian_step"] = dict(stat(runs["gauss-cost"]), ns_per_step=ns(float(np.median(runs["gauss-cost"]))), accept=acc["gauss-cost"])
            for n in NLEAPS:
                med = float(np.median(runs[f"hmc{n}"]))
                r[f"nleap{n}"] = dict(stat(runs[f"hmc{n}"]), ns_per_iteration=ns(med), ns_per_gradient=ns(med) / (n + 1), ns_per_leapfrog=ns(med) / n,
                                      accept=acc[f"hmc{n}"])
            # the cost of one more leapfrog step, from the two longest trajectories: what a trajectory costs beyond its draws
            r["ns_per_added_leapfrog"] = (r["nleap16"]["ns_per_iteration"] - r["nleap4"]["ns_per_iteration"]) / 12.0
            rec["cost"][shape] = r
            print("cost", shape, json.dumps(r), flush=True)
    if "gain" in only:
        for name in GAIN:                                        # three child processes; every figure: median and spread over them
            runs = [child(ROOT, "gain", name) for _ in range(3)]
            fold = lambda pick: {k: stat([pick(r)[k] for r in runs]) for k in ("tau_int_iterations", "accept", "device_ms", "ess_per_s")}
            g = runs[1]
            rec["gain"][name] = dict(runs=runs, hmc=dict(fold(lambda r: r["hmc"]), resolved=[r["hmc"]["resolved"] for r in runs], **GAIN[name]["hmc"]),
                                     gaussian_grid={k: dict(fold(lambda r, k=k: r["gaussian_grid"][k]), resolved=[r["gaussian_grid"][k]["resolved"] for r in runs])
                                                    for k in g["gaussian_grid"]},
                                     gaussian_best_scale=[r["gaussian_best"]["scale"] for r in runs],
                                     ess_per_s_hmc_over_gaussian=stat([r["ess_per_s_hmc_over_gaussian"] for r in runs]))
            print("gain", name, json.dumps({k: v for k, v in rec["gain"][name].items() if k != "runs"}), flush=True)
    if "price" in only:
        for shape in PRICE_SHAPES:
            runs = dict(gauss=[], gauss_parent=[], mv=[], mv_parent=[])
            for _ in range(3):
                for m in ("gauss", "mv"):
                    runs[m].append(child(ROOT, m, shape)["device_ms"])
                    if a.parent_root:
                        runs[m + "_parent"].append(child(a.parent_root, m, shape)["device_ms"])
            r = {k: stat(v) for k, v in runs.items() if v}
            for m in ("gauss", "mv"):
                if a.parent_root:
                    p = r[m + "_parent"]
                    r[m + "_inside_parent_spread"] = bool(min(p["runs"]) <= r[m]["median"] <= max(p["runs"]))
                    r[m + "_minus_parent_ms"] = r[m]["median"] - p["median"]
            rec["price"][shape] = r
            print("price", shape, json.dumps(r), flush=True)
    rec["not_measured"] = ["hardware counters", "a kernel trace", "runtime-compiled densities with a gradient (CDensity(grad=))",
                           "densities other than GaussianIso in the cost table", "nleap above 16"] + \
                          ([] if a.parent_root or "price" not in only else ["the parent commit's build (--parent-root)"])
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
