"""Writes tests/golden/pointwise/routes.npz: the chain tests/test_gpu_pointwise_routes.py runs on and what the kmc_chain_* calls of
tests/pointwise_route_cases.py return on it -- every output array (the larger ones as the SHA-256 of their bytes), n_out and the
info slots that are not times.  Data only.  Needs a GPU.

The committed fixture was recorded ONCE, from the library built at commit e67fa0f ("Split kmc_validate and kmc_sampler_describe into
per-feature parts"), the last one whose pointwise and PSIS-LOO host code was the single file kmc_pointwise.hip; the test holds every
later arrangement of that code to the same bits.  Do not regenerate it from a later library to make the test pass: a difference is a
change of behaviour to be found.  The chain is an input of the fixture, so the sampler that drew it takes no part in the comparison."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pointwise_route_cases as rc  # noqa: E402

PATH = os.path.join(HERE, "pointwise", "routes.npz")


def main():
    import kissmcmc_jl_amd as kmc
    if os.path.exists(PATH):
        sys.exit(f"{PATH} exists: it is recorded once (see this file's docstring)")
    out = {}
    for case in rc.CASES:
        pdf = rc.density(kmc, case)
        with rc.sample_chain(kmc, pdf) as s:
            chain = s.chain(logp=False)[0]
        out[f"{case}/chain"] = chain
        route = rc.ChainRoute(kmc, pdf, chain)
        for family in rc.FAMILIES:
            out.update({k: rc.digest(a) for k, a in rc.flatten(rc.run_family(route, case, family), f"{case}/{family}").items()})
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else PATH, **out)
    print(f"{len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes")


if __name__ == "__main__":
    main()
