"""The refusals of the 12 frame entry points, replayed against a transcript (tests/golden/frame_refusals.json, written by
tests/golden/make_frame_refusals.py from the faults of tests/frame_faults.py): against no context, a context without a scene and
one with three_spheres, every record -- a set of faults applied to an entry point's good call of an 8x8 frame -- must give the
recorded return code and the recorded text of rtk_last_error, exactly; an accepted call is recorded as such.  The records include
peel chains, so the order of the checks is held.  Where a HIP call itself failed (RTK_ERR_HIP: rtk_render_host asked for an image
of a negative size) the text names the call that failed, which is the implementation's to choose: the code is compared.

The column that needs no context is replayed without a device as well."""
import json
import os

import pytest

from tests import frame_faults as ff
from tests.conftest import GOLDEN
from tests.test_entry_refusals import records_of

TRANSCRIPT = os.path.join(GOLDEN, "frame_refusals.json")


def replay(rt, kinds, device):
    lib, b = ff.Answers(rt.hip_lib()), ff.Buffers(device)
    with open(TRANSCRIPT) as f:
        transcript = json.load(f)
    assert sorted(transcript) == sorted(ff.KINDS)
    wrong, n_records = [], 0
    for kind in kinds:
        table = ff.entries(ff.Context(rt, kind))
        assert sorted(transcript[kind]) == sorted(table), kind
        for name, block in transcript[kind].items():
            entry, replayed = table[name], set()
            faults_of = {f.name: f for f in entry.faults}
            for faults, rc, text in records_of(name, block):
                if rc == ff.ACCEPTED and entry.good["writes"]:     # what it writes is put back: the refused calls before it are held to account here
                    assert b.untouched(), (kind, name, faults)
                got = ff.call(entry, lib, rt, b, [faults_of[n] for n in faults])
                if got != (rc, text) and not (rc == ff.RTK_ERR_HIP and got[0] == rc):
                    wrong.append((kind, faults, (rc, text), got))
                replayed.update(faults)
                n_records += 1
            assert block["chains"] and all(len(c["faults"]) > 1 for c in block["chains"]), (kind, name)
            missing = set(faults_of) - replayed                    # no fault of the table is missing from the record
            assert not missing, (kind, name, sorted(missing))
    assert not wrong, "%d of %d records differ; the first: %s" % (len(wrong), n_records, wrong[:3])
    assert b.untouched()                                           # accepted calls aside (frame_faults restores after them), nothing was written
    return n_records


@pytest.mark.gpu
def test_every_recorded_frame_refusal_is_given_again(rt):
    assert replay(rt, ff.KINDS, True) > 1000


def test_the_refusals_that_need_no_context_are_given_again(rt):
    assert replay(rt, ("null",), False) > 300
