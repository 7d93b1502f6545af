"""What ``Imagen.sample()`` does on the host, pinned: for the fixed matrix of calls of tools/dump_sample_trace.py (one per keyword family, one
repeated) the launches issued through ``_lib.check``, every engine's workspace keys, and per workspace the sampler-state keys and the graph
keys each state holds must be, word for word, what tests/golden/sample_trace.json.gz recorded before the call plumbing was refactored."""
import gzip
import json
import os

import pytest

from tools import dump_sample_trace as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_trace.json.gz")


@pytest.mark.emu
def test_sample_trace_matches_the_recorded_one():
    with gzip.open(GOLDEN, "rt") as f:
        want = json.load(f)
    got = json.loads(D.text(D.trace("emu")))                # (through JSON: tuples and lists compare alike)
    assert [c["call"] for c in got] == [c["call"] for c in want]
    for g, w in zip(got, want):
        assert g["launches"] == w["launches"], g["call"]
        assert g["workspaces"] == w["workspaces"], g["call"]
