"""The CPU side of the stream-order tests (tests/stream_common.py, tests/test_gpu_streams.py): every stream-taking entry of
include/nerftex.h has a case off the null stream, the table of entries that wait on purpose is the documented one, and the batches the traps
swap are fair."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import stream_common as sc


def test_every_stream_taking_entry_has_a_case():
    """A prototype with an `ntx_stream` parameter is in `COVERED` (an id of tests/test_gpu_streams.py runs it on a side stream) or, for an
    entry that waits on purpose, in `SYNCHRONISING`: a new stream-taking entry without a case fails here."""
    entries = sc.stream_entries()
    assert len(entries) >= 25 and "ntx_render_rays" in entries and "ntx_train_backward" in entries and "ntx_create" not in entries, entries
    missing = [e for e in entries if e not in sc.COVERED and e not in sc.SYNCHRONISING]
    assert not missing, f"stream-taking entries without a case in tests/test_gpu_streams.py: {missing}"
    unknown = [e for e in sc.COVERED if e not in entries]
    assert not unknown, f"COVERED names entries that take no stream (or do not exist): {unknown}"
    declared = set(re.findall(r"\b(ntx_\w+)\s*\(", open(sc.HEADER).read()))
    assert not [e for e in sc.SYNCHRONISING if e not in declared], "SYNCHRONISING names entries the header does not declare"
    for e, (scope, why) in sc.SYNCHRONISING.items():
        assert scope in ("device", "stream", "setup") and why and "\n" not in why, e


def test_the_table_and_the_collected_ids_agree():
    """Every test `COVERED` names exists in tests/test_gpu_streams.py, by collected id (and every case id is collected under both traps)."""
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_streams.py")], capture_output=True,
                         text=True, cwd=sc.ROOT, timeout=300)
    ids = {line.split("::", 1)[1] for line in out.stdout.splitlines() if "::" in line}
    assert ids, (out.stdout[-2000:], out.stderr[-2000:])
    assert not [t for t in sc.COVERED.values() if t not in ids], [t for t in sc.COVERED.values() if t not in ids]
    assert not [(c, t) for c, t in sc.trap_ids() if f"test_trap[{c}-{t}]" not in ids]


@pytest.mark.parametrize("path", [sc.HEADER, sc.INTEGRATION], ids=["nerftex.h", "INTEGRATION_details.md"])
def test_the_documented_table_is_the_tested_one(path):
    """The synchronisation table of the header's conventions and of the integration notes equals `SYNCHRONISING`, entry by entry."""
    assert sc.documented_table(path) == {e: scope for e, (scope, _) in sc.SYNCHRONISING.items()}


def case_batches():
    """(id, inputs(seed), fairness check or None) of every kind of batch the cases take, without a device."""
    rows = [("camera", lambda s: sc.camera_batch(s, 7), sc.camera_fair), ("instancer", sc.instancer_batch, None),
            ("instanced", lambda s: sc.instanced_batch(s, (1, 6), 23, 70), sc.instanced_fair)]
    rows += [(f"train_{k}", lambda s, k=k: sc.trainer_batch(k, s), sc.train_fair) for k in sc.TRAIN_BATCH]
    return rows


@pytest.mark.parametrize("name,inputs,fair", case_batches(), ids=[r[0] for r in case_batches()])
def test_the_three_batches_differ_in_every_array_and_are_all_fair(name, inputs, fair):
    """A late copy, or a kernel that ran on the other batch, can only be seen if the batches differ in every input; and the other batch is as
    valid as the real one (no NaN, no index out of range, the same mix of hits and misses), so that a mis-ordered kernel computes a wrong number
    instead of faulting."""
    real, history, poison = (inputs(s) for s in (sc.REAL, sc.HISTORY, sc.POISON))
    sc.differ_everywhere(real, poison)
    sc.differ_everywhere(real, history)
    sc.differ_everywhere(history, poison)
    for b in (real, history, poison):
        for k, v in b.items():
            if v.dtype.kind == "f" and k not in ("t",):
                assert not np.isnan(v).any(), k
        if fair is not None:
            fair(b)


def test_a_step_without_live_samples_is_swapped_for_one_with():
    real, poison = sc.instanced_batch(sc.REAL, (1, 6), 23, 70, "none"), sc.instanced_batch(sc.POISON, (1, 6), 23, 70)
    sc.instanced_fair(real, "none")
    sc.instanced_fair(poison, "some")
    assert real["hit"].all() and (real["dists"] <= 0).all()


def test_delays_follow_the_reference_run():
    assert sc.delay_ms(0.0) == sc.MIN_DELAY_MS == 20.0 and sc.delay_ms(0.5) == 5000.0 and sc.DELAY_FACTOR == 10.0
    assert sorted(set(sc.CASE_IDS)) == sorted(sc.CASE_IDS) and len(sc.trap_ids()) == 2 * len(sc.CASE_IDS)
