"""The striped scan's results bit for bit (gpu).

tests/golden/striped_scan_bits.json holds every field of every state of Size plus the six C2 analyzers per column,
recorded by tools/scan_bits_golden.py from the library before the r08 instruction cuts in the 8-byte tile loop. The
cuts leave the per-lane arithmetic, the lane -> row mapping and the fold order alone, so at a fixed grid the states
must not move by a bit. Inputs: tests/striped_bits_cases.py.
"""
import json

import pytest

import striped_bits_cases as C
from test_gpu_scan import assert_state_parity

pytestmark = pytest.mark.gpu

_TABLES = {}


@pytest.fixture(scope="module")
def golden():
    with open(C.GOLDEN) as f:
        return json.load(f)["cases"]


def _table(key, build):
    if key not in _TABLES:
        _TABLES[key] = build().to_device()
    return _TABLES[key]


def _assert_bits(golden, key, grid, table, analyzers, states):
    exp = golden["%s/grid=%d" % (key, grid)]
    assert len(exp) == len(analyzers)
    for an, st in zip(analyzers, states):
        assert C.encode(st) == exp[repr(an)], (key, grid, an, st)


# ---- (a) bit identity with the recorded build ----------------------------------------------------------------
@pytest.mark.parametrize("grid", C.GRIDS)
@pytest.mark.parametrize("kind", ["c2", "crafted"])
def test_states_match_recorded_bits(monkeypatch, golden, kind, grid):
    monkeypatch.setenv("DQ_SCAN_GRID", str(grid))
    for key, build in C.cases():
        if not key.startswith(kind + "/"):
            continue
        table = _table(key, build)
        analyzers = C.analyzers_of(table)
        _assert_bits(golden, key, grid, table, analyzers, C.run_states(table, analyzers))


# ---- (b) lanes whose first kept batch comes late, or never -----------------------------------------------------
def test_late_first_batch(monkeypatch, golden):
    monkeypatch.setenv("DQ_SCAN_GRID", "2")
    key = "late/n=%d" % C.LATE_ROWS
    table = _table(key, C.late_first_batch_table)
    analyzers = C.analyzers_of(table)
    states = C.run_states(table, analyzers)
    for an, st in zip(analyzers, states):
        assert_state_parity(table, an, st)
    _assert_bits(golden, key, 2, table, analyzers, states)
