"""The seven pointwise / PSIS-LOO entry pairs by their two routes -- kmc_sampler_* on the chain a sampler holds, kmc_chain_* on that
chain copied to the host -- with the calls of tests/pointwise_route_cases.py: every output array, n_out and the info slots that are not
times agree bit for bit.  Both routes fill one request and run one body, and a swapped argument in either wrapper shows here: every
element of the selection (first_sample = 4, thin = 3, five walkers masked out), of the held-out data and of the ranges is non-default.

And against the past: the kmc_chain_* calls on the chain stored in tests/golden/pointwise/routes.npz return the bits recorded there from
the library whose pointwise host code was still one file (tests/golden/make_pointwise_routes.py)."""
import functools
import os

import numpy as np
import pytest

import pointwise_route_cases as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "pointwise", "routes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def samplers(kmc):
    """Per case: the density, the sampler with its stored chain, and that chain on the host."""
    out = {}
    for case in rc.CASES:
        pdf = rc.density(kmc, case)
        s = rc.sample_chain(kmc, pdf)
        out[case] = (pdf, s, s.chain(logp=False)[0])
    yield out
    for _, s, _ in out.values():
        s.close()


@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("case", list(rc.CASES))
def test_the_two_routes_agree_bit_for_bit(kmc, samplers, case, family):
    pdf, s, chain = samplers[case]
    by_sampler = rc.flatten(rc.run_family(rc.SamplerRoute(s), case, family), f"{case}/{family}")
    by_chain = rc.flatten(rc.run_family(rc.ChainRoute(kmc, pdf, chain), case, family), f"{case}/{family}")
    assert list(by_sampler) == list(by_chain) and len(by_chain) >= 4
    for k in by_chain:
        assert same_bits(by_sampler[k], by_chain[k]), k
        if k.endswith("/n"):
            assert by_chain[k][0] == rc.N, k
    # workspace = 1: one group of 64 observations per block and per batch, so J70's range [3, 68) runs two of each
    groups = {"J70": 2, "J10": 1}[case]
    if family == "relative_eff":
        assert by_chain[f"{case}/{family}/max_lag=5/workspace=1/info"][1] == groups
    elif family == "psis_loo":
        assert by_chain[f"{case}/{family}/r_eff=0.7/workspace=1/info"][2] == groups
    elif family == "psis_loo_reff":
        info = by_chain[f"{case}/{family}/computed/split=0/max_lag=5/workspace=1/info"]
        assert info[2] == groups and info[7] == groups                              # (of the kept slots: blocks, groups)


@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("case", list(rc.CASES))
def test_the_chain_route_returns_the_recorded_bits(kmc, case, family):
    want = {k: v for k, v in golden().items() if k.startswith(f"{case}/{family}/")}
    got = rc.flatten(rc.run_family(rc.ChainRoute(kmc, rc.density(kmc, case), golden()[f"{case}/chain"]), case, family), f"{case}/{family}")
    assert list(got) == list(want) and want
    for k in want:
        assert same_bits(rc.digest(got[k]), want[k]), k
