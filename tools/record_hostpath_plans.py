"""Record what the twelve module-loop entries and the five finish functions of the built _hostpath extension do on the sweep of
tests/_hostpath_plan_cases.py into tests/hostpath_plans.json (batch keys, table rows with pointers as symbols, `rest`, job tuples, the modules' entries after
the finish), or with --check compare the built extension against that record.  CPU only.  Record on the commit whose behaviour is the yardstick, BEFORE
changing csrc/host/ct_hostpath.cpp; tests/test_hostpath_plans.py replays the file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _hostpath_plan_cases as C  # noqa: E402
import compressed_tensors_amd as cta  # noqa: E402
from compressed_tensors_amd import _lib  # noqa: E402

RECORD = os.path.join(ROOT, "tests", "hostpath_plans.json")


def main():
    hp = _lib.hostpath()
    assert hp is not None, "the host extension was not built (python -c 'import __graft_entry__ as g; g.build()')"
    try:
        got = {case["id"]: C.run_case(cta, hp, case) for case in C.cases()}
    finally:
        C.restore()
    if "--check" in sys.argv:
        want = C.unpack(json.load(open(RECORD)))
        bad = sorted(k for k in set(got) | set(want) if json.loads(json.dumps(got.get(k))) != want.get(k))
        print(f"{len(got)} cases, {len(bad)} differ" + "".join("\n  " + b for b in bad))
        return 1 if bad else 0
    doc = C.pack(got)
    with open(RECORD, "w") as f:  # one state, one call per line
        f.write('{"states":[\n' + ",\n".join(json.dumps(s) for s in doc["states"]) + '\n],"cases":{\n')
        f.write(",\n".join(json.dumps(k) + ":[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in g) + "]" for k, g in doc["cases"].items()) + "\n}}\n")
    print(f"{len(got)} cases, {sum(len(g) for g in got.values())} calls, {len(doc['states'])} states -> {RECORD} ({os.path.getsize(RECORD)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
