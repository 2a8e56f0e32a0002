"""Writes tests/golden/entry_refusals.json: what the built library answers, with a null context, to the faults of
tests/entry_faults.py -- the record tests/test_entry_refusals.py replays.  Run from a checkout with the libraries built:

    python tests/golden/make_entry_refusals.py

For each entry point: every fault alone; then peel chains -- one fault of every group applied at once (chain k takes the k-th
alternative of a group where it has one, at most three chains), the answer recorded, the fault the text names removed, and again
until the call reaches the entry point's last refusal ("null context"; "bad argument" for rtk_debug_*).  The order of the
refusals is in the chains: two checks swapped change a chain's texts.

A record is {entry, faults applied, rc, text}.  The file holds them per entry point, the text without its "<entry>: ":
"alone" lists [fault or null for the good call, rc, text]; a chain is the "faults" it starts from and its "peel", one
[rc, text, the fault removed before the next call] per call, so that a call's faults are the chain's less those removed so far.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import raytracingoneweekendapplication_amd as rt  # noqa: E402
from tests import entry_faults as ef  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "entry_refusals.json")
MAX_CHAINS = 3


def chains(entry):
    """The fault lists the peel chains start from."""
    groups = {}
    for f in entry.faults:
        if not f.solo:
            groups.setdefault(f.group, []).append(f)
    for k in range(min(MAX_CHAINS, max(len(g) for g in groups.values()))):
        yield [g[min(k, len(g) - 1)] for g in groups.values()]


def transcript(entry, lib, b):
    """(the "alone" records, the chains) of one entry point."""
    names = [f.name for f in entry.faults]
    assert len(set(names)) == len(names), (entry.name, names)
    prefix = entry.name + ": "

    def answer(faults):
        rc, text = ef.call(entry, lib, rt, b, faults)
        assert rc != 0 and text.startswith(prefix), (entry.name, [f.name for f in faults], rc, text)
        return rc, text[len(prefix):]

    alone = [[None, *answer([])]] + [[f.name, *answer([f])] for f in entry.faults]
    peeled = []
    for applied in chains(entry):
        chain = {"faults": [f.name for f in applied], "peel": []}
        while True:
            rc, text = answer(applied)
            if text.endswith(entry.terminal):
                chain["peel"].append([rc, text, None])
                break
            named = [f for f in applied if f.names in " " + text]     # (a name such as " n must be" begins with the blank after "<entry>:")
            assert named, "%s: no applied fault is named by %r (%s)" % (entry.name, text, [f.name for f in applied])
            chain["peel"].append([rc, text, named[0].name])
            applied = [f for f in applied if f is not named[0]]
        peeled.append(chain)
    return alone, peeled


def main():
    lib, b = rt.hip_lib(), ef.Buffers(rt)
    dump = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    rows = lambda records: "[\n" + ",\n".join(dump(r) for r in records) + "\n]"  # noqa: E731
    blocks, total = [], 0
    for entry in ef.ENTRIES.values():
        alone, peeled = transcript(entry, lib, b)
        total += len(alone) + sum(len(c["peel"]) for c in peeled)
        chains_text = ",\n".join('{"faults":%s,\n"peel":%s}' % (dump(c["faults"]), rows(c["peel"])) for c in peeled)
        blocks.append('%s:{"alone":%s,\n"chains":[\n%s\n]}' % (dump(entry.name), rows(alone), chains_text))
    assert b.untouched()
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(blocks) + "\n}\n")
    print("%d records of %d entry points -> %s" % (total, len(ef.ENTRIES), OUT))


if __name__ == "__main__":
    main()
