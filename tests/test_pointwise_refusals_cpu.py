"""The pointwise / PSIS-LOO calls against their recorded refusals (tests/golden/pointwise_refusals.json, written once by
tests/golden/make_pointwise_refusals.py from the library whose pointwise host code was still the single file kmc_pointwise.hip): the same
status and the same kmc_last_error() text, byte for byte, for every call of tests/pointwise_refusal_cases.py -- the seven kmc_chain_*
calls with one, two and three faults at once, where the ORDER of the checks decides which refusal is given, the kmc_sampler_* forms with
a null sampler, and the plans and host stages, whose accepted calls return the recorded bits.  No device is touched."""
import hashlib
import json
import os

import pytest

import pointwise_refusal_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def rows(kmc):
    return cases.run_cases(kmc)


@pytest.fixture(scope="module")
def recorded(rows):
    """{case id: [status, message, outputs or None]}: the fixture holds the outcomes in the order of the case list, whose ids it pins by
    their count and SHA-256."""
    with open(os.path.join(HERE, "golden", "pointwise_refusals.json")) as f:
        d = json.load(f)
    ids = [r[0] for r in rows]
    assert len(ids) == d["count"] == len(d["cases"]) and hashlib.sha256("\n".join(ids).encode()).hexdigest() == d["ids_sha256"], \
        "the case list and the fixture differ: new cases are ADDED at the end of the list and of the fixture (make_pointwise_refusals.py --add)"
    return {cid: d["outcomes"][i] for cid, i in zip(ids, d["cases"])}


def test_every_recorded_case_gets_the_recorded_answer(recorded, rows):
    for cid, st, msg, _, rec in rows:
        assert [st, msg, rec] == recorded[cid], f"first differing case: {cid}: recorded {recorded[cid]}, got {[st, msg, rec]}"


def test_a_refused_call_leaves_its_outputs_untouched(rows):
    for cid, st, _, untouched, _ in rows:
        assert st == 0 or untouched, cid


def test_the_list_needs_no_device_and_covers_the_family(kmc, recorded):
    from kissmcmc_jl_amd import _lib
    for cid, (st, msg, rec) in recorded.items():
        assert st != _lib.ERR_NO_DEVICE and (st != 0) == (rec is None) and (st == 0) == (msg == ""), cid
    for fn in cases.CHAIN_CALLS:
        assert sum(cid.startswith(fn + "/") and cid.count("+") == 1 for cid in recorded) >= 100, fn
        assert recorded[f"{fn}/non_data"][1].startswith("the pointwise log-likelihood needs a data density")
        assert recorded[f"null_sampler/{fn}"] == [_lib.ERR_BAD_ARG, "null sampler", None]
    for fn in ("pointwise_plan", "psis_plan", "waic_stats", "loo_stats", "psis_smooth_host"):
        got = [v for cid, v in recorded.items() if cid.startswith(fn + "/")]
        assert any(st == 0 for st, _, _ in got) and any(st != 0 for st, _, _ in got), fn
    assert recorded["psis_loo/non_data+null_lppd"][1] == "null argument"                # the chain route checks lppd_j before the density
    assert recorded["null_sampler/psis_loo/null_lppd"][1] == "null sampler"             # the sampler route, the sampler before lppd_j
    assert len({(st, msg) for st, msg, _ in recorded.values()}) >= 60
