"""Writes tests/golden/pointwise_refusals.json: (status, kmc_last_error()) of every call of tests/pointwise_refusal_cases.py, and the
outputs of the accepted calls of the plans and the host stages.  Data only: status codes, the library's messages and numbers.  The file
holds the distinct outcomes, then per case, in the order of the case list, the index of its outcome; the case ids themselves are the
list's (run_cases) and are pinned by their count and the SHA-256 of their lines.

The committed fixture was recorded ONCE, from the library built at commit e67fa0f ("Split kmc_validate and kmc_sampler_describe into
per-feature parts") -- the last one whose pointwise and PSIS-LOO host code was the single file kmc_pointwise.hip -- and pins what that
file answered, so that tests/test_pointwise_refusals_cpu.py holds every later arrangement of the checks to the same refusal, word for
word, also where a call breaks several rules at once.  Do not regenerate it from a later library to make that test pass; a new check
adds cases at the END of the list, recorded with
    python tests/golden/make_pointwise_refusals.py --add
which keeps every recorded case as it is and refuses to go on when the list no longer begins with the recorded cases or the loaded
library answers one of them differently.
Needs no device: every case is refused before one is touched, or is a call that touches none."""
import hashlib
import json
import os
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pointwise_refusal_cases  # noqa: E402

PATH = os.path.join(HERE, "pointwise_refusals.json")


def ids_digest(ids):
    return hashlib.sha256("\n".join(ids).encode()).hexdigest()


def dump(rows, path=PATH):
    outcomes, index, cases = [], {}, []
    for _, st, msg, _, rec in rows:
        key = json.dumps([st, msg, rec])
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
    """{case id: [status, message, outputs or None]} of the recorded cases, which must be the first of `ids`."""
    with open(path) as f:
        d = json.load(f)
    n = d["count"]
    if len(d["cases"]) != n or len(ids) < n or ids_digest(ids[:n]) != d["ids_sha256"]:
        raise ValueError("the case list does not begin with the recorded cases: new cases are ADDED at its end")
    return {cid: d["outcomes"][i] for cid, i in zip(ids, d["cases"])}


def main():
    import kissmcmc_jl_amd as kmc
    from kissmcmc_jl_amd import _lib
    rows = pointwise_refusal_cases.run_cases(kmc)
    for cid, st, msg, untouched, rec in rows:
        if st == _lib.ERR_NO_DEVICE or (st == 0 and rec is None):
            sys.exit(f"{cid}: not refused from its arguments alone (status {st}): it does not belong in this list")
        if st and not untouched:
            sys.exit(f"{cid}: refused, but an output array was written")
    if "--add" in sys.argv[1:]:
        old = load([r[0] for r in rows])
        for cid, st, msg, _, rec in rows:
            if cid in old and old[cid] != [st, msg, rec]:
                sys.exit(f"{cid}: recorded {old[cid]}, the loaded library answers {[st, msg, rec]}")
    elif os.path.exists(PATH):
        sys.exit(f"{PATH} exists: it is recorded once (see this file's docstring); --add records new cases next to it")
    outcomes = dump(rows)
    print(f"{len(rows)} cases, {sum(r[1] == 0 for r in rows)} accepted, {len(outcomes)} distinct outcomes")


if __name__ == "__main__":
    main()
