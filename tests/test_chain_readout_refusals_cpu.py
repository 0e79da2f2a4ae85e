"""The convergence / rank / quantile / HDI read-outs against their recorded refusals (tests/golden/chain_readout_refusals.json, written
once by tests/golden/make_chain_readout_refusals.py from the library in which each of the seven read-outs still spelt out its own
preamble): the same status, the same kmc_last_error() text, byte for byte, and the same m_out, h_out and n_out left behind, for every
call of tests/chain_readout_refusal_cases.py -- the seven kmc_chain_* calls with one, two and three faults at once, where the ORDER of
the checks decides which refusal is given, the kmc_sampler_* forms with a null sampler, and the stages that touch no device, whose
accepted calls return the recorded bits.  No device is touched."""
import hashlib
import json
import os

import pytest

import chain_readout_refusal_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def rows(kmc):
    return cases.run_cases(kmc)


@pytest.fixture(scope="module")
def recorded(rows):
    """{case id: [status, message, sizes out, outputs or None]}: the fixture holds the outcomes in the order of the case list, whose ids
    it pins by their count and SHA-256."""
    with open(os.path.join(HERE, "golden", "chain_readout_refusals.json")) as f:
        d = json.load(f)
    ids = [r[0] for r in rows]
    assert len(ids) == d["count"] == len(d["cases"]) and hashlib.sha256("\n".join(ids).encode()).hexdigest() == d["ids_sha256"], \
        "the case list and the fixture differ: new cases are ADDED at the end of the list and of the fixture (make_chain_readout_refusals.py --add)"
    return {cid: d["outcomes"][i] for cid, i in zip(ids, d["cases"])}


def test_every_recorded_case_gets_the_recorded_answer(recorded, rows):
    for cid, st, msg, _, sizes, rec in rows:
        assert [st, msg, sizes, rec] == recorded[cid], f"first differing case: {cid}: recorded {recorded[cid]}, got {[st, msg, sizes, rec]}"


def test_a_refused_call_writes_nothing_but_its_sizes_out(rows):
    for cid, st, _, untouched, _, _ in rows:
        assert st == 0 or untouched, cid


def test_the_list_needs_no_device_and_covers_the_family(kmc, recorded):
    from kissmcmc_jl_amd import _lib
    for cid, (st, msg, sizes, rec) in recorded.items():
        assert st != _lib.ERR_NO_DEVICE and (st != 0) == (rec is None) and (st == 0) == (msg == ""), cid
    for fn in cases.CHAIN_CALLS:
        assert sum(cid.startswith(fn + "/") and cid.count("+") == 1 for cid in recorded) >= 25, fn
        assert any(cid.startswith(fn + "/") and cid.count("+") == 2 for cid in recorded), fn
        assert recorded[f"{fn}/null_chain"][:2] == [_lib.ERR_BAD_ARG, "null argument"]
        assert recorded[f"null_sampler/{fn}"] == [_lib.ERR_BAD_ARG, "null sampler", [-7, -7, None] if fn != "hdi" else [None, None, -7], None]
    for fn in ("convergence_stats", "rank_normal_scores", "hdi_span", "beta_quantile", "quantile_mcse_ranks", "indicator_moments"):
        got = [v for cid, v in recorded.items() if cid.startswith(fn + "/")]
        assert any(v[0] == 0 for v in got) and any(v[0] != 0 for v in got), fn
    for plan in ("convergence_plan", "rank_plan", "indicator_plan"):
        assert recorded[plan][0] == 0
    assert recorded["hdi/prob*N<1"][2] == [None, None, 120]                              # kmc_chain_hdi has written n_out by then
    assert recorded["hdi/prob=0"][2] == [None, None, -7]                                 # ... and not yet here
    assert recorded["convergence/max_lag=2"][2] == [-7, -7, None]                        # m_out and h_out go out after every check
    assert len({(v[0], v[1]) for v in recorded.values()}) >= 40
