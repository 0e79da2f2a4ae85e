"""Writes tests/golden/chain_readout_refusals.json: status, kmc_last_error() and the sizes out (m_out, h_out, n_out as the call left
them) of every call of tests/chain_readout_refusal_cases.py, and the outputs of the accepted calls of the stages that touch no device.
Data only: status codes, the library's messages and numbers.  The file holds the distinct outcomes, then per case, in the order of the
case list, the index of its outcome; the case ids themselves are the list's (run_cases) and are pinned by their count and the SHA-256
of their lines.

The committed fixture was recorded ONCE, from the library built at commit d91ebad ("Add the ESS and MCSE of quantiles, from bit-packed
indicator chains") -- the last one in which each of the seven read-outs spelt out its own preamble -- and pins what those seven bodies
answered, so that tests/test_chain_readout_refusals_cpu.py holds every later arrangement of the checks to the same refusal, word for
word, also where a call breaks several rules at once.  Do not regenerate it from a later library to make that test pass; a new check
adds cases at the END of the list, recorded with
    python tests/golden/make_chain_readout_refusals.py --add
which keeps every recorded case as it is and refuses to go on when the list no longer begins with the recorded cases or the loaded
library answers one of them differently.
Needs no device: every case is refused before one is touched, or is a call that touches none."""
import json
import os
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import chain_readout_refusal_cases  # noqa: E402
from make_pointwise_refusals import ids_digest  # noqa: E402

PATH = os.path.join(HERE, "chain_readout_refusals.json")


def outcome(row):
    _, st, msg, _, sizes, rec = row
    return [st, msg, sizes, rec]


def dump(rows, path=PATH):
    outcomes, index, cases = [], {}, []
    for row in rows:
        key = json.dumps(outcome(row))
        if key not in index:
            index[key] = len(outcomes)
            outcomes.append(key)
        cases.append(index[key])
    with open(path, "w") as f:
        f.write('{"outcomes": [\n' + ",\n".join(outcomes) + '\n],\n')
        f.write(f'"count": {len(rows)}, "ids_sha256": "{ids_digest([r[0] for r in rows])}",\n"cases": [\n')
        f.write(textwrap.fill(", ".join(str(i) for i in cases), 160) + "\n]}\n")
    return outcomes


def load(ids, path=PATH):
    """{case id: [status, message, sizes out, outputs or None]} of the recorded cases, which must be the first of `ids`."""
    with open(path) as f:
        d = json.load(f)
    n = d["count"]
    if len(d["cases"]) != n or len(ids) < n or ids_digest(ids[:n]) != d["ids_sha256"]:
        raise ValueError("the case list does not begin with the recorded cases: new cases are ADDED at its end")
    return {cid: d["outcomes"][i] for cid, i in zip(ids, d["cases"])}


def main():
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import _lib
    rows = chain_readout_refusal_cases.run_cases(kmc)
    for row in rows:
        cid, st, _, untouched, _, rec = row
        if st == _lib.ERR_NO_DEVICE or (st == 0 and rec is None):
            sys.exit(f"{cid}: not refused from its arguments alone (status {st}): it does not belong in this list")
        if st and not untouched:
            sys.exit(f"{cid}: refused, but an output array other than the sizes out was written")
    if "--add" in sys.argv[1:]:
        old = load([r[0] for r in rows])
        for row in rows:
            if row[0] in old and old[row[0]] != outcome(row):
                sys.exit(f"{row[0]}: recorded {old[row[0]]}, the loaded library answers {outcome(row)}")
    elif os.path.exists(PATH):
        sys.exit(f"{PATH} exists: it is recorded once (see this file's docstring); --add records new cases next to it")
    outcomes = dump(rows)
    print(f"{len(rows)} cases, {sum(r[1] == 0 for r in rows)} accepted, {len(outcomes)} distinct outcomes")


if __name__ == "__main__":
    main()
