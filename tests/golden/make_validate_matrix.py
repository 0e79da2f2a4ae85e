"""Writes tests/golden/validate_matrix.json: (status, kmc_last_error()) of kmc_validate for every configuration of
tests/validate_cases.py.  Data only: case ids, status codes and the library's messages.

The committed fixture was recorded ONCE, from the library built at commit a65929b ("Share one draw pass per workgroup in C2's
burn-in half-steps") -- the last one whose kmc_validate was a single function in kmc_sampler.hip -- and pins what that function
answered, so that tests/test_validate_matrix_cpu.py holds every later arrangement of the checks to the same refusal, word for
word, also where a configuration breaks several rules at once.  Do not regenerate it from a later library to make that test pass;
a new check adds cases, recorded with
    python tests/golden/make_validate_matrix.py --add
which keeps every recorded case as it is and refuses to go on when the loaded library answers one of them differently.
Needs no device (kmc_validate touches none)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import validate_cases  # noqa: E402

PATH = os.path.join(HERE, "validate_matrix.json")


def dump(rows, path=PATH):
    outcomes, index, cases = [], {}, []
    for cid, st, msg in rows:
        if (st, msg) not in index:
            index[(st, msg)] = len(outcomes)
            outcomes.append([st, msg])
        cases.append((cid, index[(st, msg)]))
    with open(path, "w") as f:
        f.write('{"outcomes": [\n' + ",\n".join(json.dumps(o) for o in outcomes) + '\n],\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(cid)}: {i}" for cid, i in cases) + "\n}}\n")
    return outcomes


def load(path=PATH):
    """{case id: (status, message)}"""
    with open(path) as f:
        d = json.load(f)
    return {cid: tuple(d["outcomes"][i]) for cid, i in d["cases"].items()}


def main():
    import kissmcmc_jl_amd as kmc
    rows = validate_cases.run_cases(validate_cases.Densities(kmc))
    if "--add" in sys.argv[1:]:
        old = load()
        for cid, st, msg in rows:
            if cid in old and old[cid] != (st, msg):
                sys.exit(f"{cid}: recorded {old[cid]}, the loaded library answers {(st, msg)}")
    elif os.path.exists(PATH):
        sys.exit(f"{PATH} exists: it is recorded once (see this file's docstring); --add records new cases next to it")
    outcomes = dump(rows)
    print(f"{len(rows)} cases, {sum(st == 0 for _, st, _ in rows)} accepted, {len(outcomes)} distinct outcomes, "
          f"{len({m for _, m in outcomes if m})} distinct messages")


if __name__ == "__main__":
    main()
