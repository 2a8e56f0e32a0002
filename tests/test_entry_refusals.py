"""The refusals of the 30 lane-per-ray entry points, replayed against a transcript (tests/golden/entry_refusals.json, written by
tests/golden/make_entry_refusals.py from the faults of tests/entry_faults.py).  Every record -- a set of faults applied to an
entry point's good null-context call -- must give the recorded return code and the recorded text of rtk_last_error, exactly.  The
records include peel chains (many faults at once, then the one the text names removed, and again), so the order of the checks
is held, not only their presence.  No device is needed and nothing is written."""
import json
import os

from tests import entry_faults as ef
from tests.conftest import GOLDEN

TRANSCRIPT = os.path.join(GOLDEN, "entry_refusals.json")


def records_of(name, block):
    """(faults applied, rc, text) of every record the transcript holds for one entry point (the layout is described in
    tests/golden/make_entry_refusals.py)."""
    for fault, rc, text in block["alone"]:
        yield ([] if fault is None else [fault]), rc, name + ": " + text
    for chain in block["chains"]:
        applied = list(chain["faults"])
        for k, (rc, text, removed) in enumerate(chain["peel"]):
            yield list(applied), rc, name + ": " + text
            if k + 1 < len(chain["peel"]):
                assert removed in applied, "%s: a chain removes %r, which is not applied (%s)" % (name, removed, applied)
                applied.remove(removed)


def test_every_recorded_refusal_is_given_again(rt):
    lib, b = rt.hip_lib(), ef.Buffers(rt)
    with open(TRANSCRIPT) as f:
        transcript = json.load(f)
    replayed, wrong, n_records = {}, [], 0
    for name, block in transcript.items():
        assert name in ef.ENTRIES, "the transcript holds an entry point the table does not: %s" % name
        entry = ef.ENTRIES[name]
        table = {f.name: f for f in entry.faults}
        for faults, rc, text in records_of(name, block):
            unknown = [n for n in faults if n not in table]
            assert not unknown, "%s: the transcript holds faults the table does not: %s" % (name, unknown)
            got = ef.call(entry, lib, rt, b, [table[n] for n in faults])
            if got != (rc, text):
                wrong.append((faults, (rc, text), got))
            replayed.setdefault(name, set()).update(faults)
            n_records += 1
        assert block["chains"] and all(len(c["faults"]) > 1 for c in block["chains"]), name
    assert not wrong, "%d of %d records differ; the first: %s" % (len(wrong), n_records, wrong[:3])
    assert len(ef.ENTRIES) == 30 and sorted(replayed) == sorted(ef.ENTRIES), sorted(set(ef.ENTRIES) - set(replayed))
    for name, entry in ef.ENTRIES.items():                        # ... and no fault of the table is missing from it
        missing = {f.name for f in entry.faults} - replayed[name]
        assert not missing, (name, sorted(missing))
    assert b.untouched()
