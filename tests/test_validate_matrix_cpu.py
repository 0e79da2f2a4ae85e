"""kmc_validate against its recorded refusal matrix (tests/golden/validate_matrix.json, written once by
tests/golden/make_validate_matrix.py from the library whose kmc_validate was still one function): the same status and the same
kmc_last_error() text, byte for byte, for every configuration of tests/validate_cases.py -- the cross product of the features, where a
configuration breaks several rules at once and the ORDER of the checks decides which refusal it gets, and every refusal over an
argument's value one fault at a time.  No device is touched."""
import json
import os

import validate_cases

HERE = os.path.dirname(os.path.abspath(__file__))


def _recorded():
    with open(os.path.join(HERE, "golden", "validate_matrix.json")) as f:
        d = json.load(f)
    return {cid: tuple(d["outcomes"][i]) for cid, i in d["cases"].items()}, [tuple(o) for o in d["outcomes"]]


def test_every_recorded_case_gets_the_recorded_refusal(kmc):
    want, _ = _recorded()
    got = validate_cases.run_cases(validate_cases.Densities(kmc))
    assert [cid for cid, _, _ in got] == list(want), "the case list and the fixture differ: new cases are ADDED to the fixture (make_validate_matrix.py --add)"
    for cid, st, msg in got:
        assert (st, msg) == want[cid], f"first differing case: {cid}: recorded {want[cid]}, got {(st, msg)}"


def test_the_list_covers_the_product_and_has_accepted_cases(kmc):
    want, outcomes = _recorded()
    product = [cid for cid in want if cid.startswith("x/")]
    assert len(product) == 5 * 6 * 2 * 2 * 2 * 4 * 2 * 2
    assert sum(st == 0 for st, _ in want.values()) >= 42 and len(outcomes) >= 34
    assert want["base"] == (0, "") and want["null_config"][1] == "null config"

