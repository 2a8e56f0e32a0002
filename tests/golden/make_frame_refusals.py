"""Writes tests/golden/frame_refusals.json: what the built library answers to the faults of tests/frame_faults.py, for each of
its three contexts (none, one without a scene, one with three_spheres) -- the record tests/test_frame_refusals.py replays.  Run
on an MI355X from a checkout with the libraries built; the file is written to the path given, or in place:

    python tests/golden/make_frame_refusals.py [out.json]

The records and their layout are tests/golden/make_entry_refusals.py's -- every fault alone, then up to three peel chains per
entry point -- made by its transcript(), once per context: {context: {entry point: {"alone": ..., "chains": ...}}}.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import raytracingoneweekendapplication_amd as rt  # noqa: E402
from tests import frame_faults as ff  # noqa: E402
from tests.golden.make_entry_refusals import transcript  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "frame_refusals.json")


def main(out):
    lib, b = ff.Answers(rt.hip_lib()), ff.Buffers(True)
    dump = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    rows = lambda records: "[\n" + ",\n".join(dump(r) for r in records) + "\n]"  # noqa: E731
    columns, total = [], 0
    for kind in ff.KINDS:
        blocks = []
        for entry in ff.entries(ff.Context(rt, kind)).values():
            alone, peeled = transcript(entry, lib, b)
            total += len(alone) + sum(len(c["peel"]) for c in peeled)
            chains_text = ",\n".join('{"faults":%s,\n"peel":%s}' % (dump(c["faults"]), rows(c["peel"])) for c in peeled)
            blocks.append('%s:{"alone":%s,\n"chains":[\n%s\n]}' % (dump(entry.name), rows(alone), chains_text))
        columns.append("%s:{\n%s\n}" % (dump(kind), ",\n".join(blocks)))
    assert b.untouched()
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(columns) + "\n}\n")
    print("%d records of 12 entry points in %d contexts -> %s" % (total, len(ff.KINDS), out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
