"""bench.py --dump-outputs: the folded states of the last timed step are written as finite float64 arrays, one row per
op (the state's fields in dq_state order, zero-padded), each op's metric value, and a mask of the ops that have a
state. CPU only: the states are built by hand."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import deequ_amd.native as N  # noqa: E402
from deequ_amd.states import state_from_native  # noqa: E402


def _state(kind, present=1):
    s = N.DqState()
    s.kind, s.present = kind, present
    return s


def test_dump_outputs_layout(tmp_path):
    size = _state(N.OP_SIZE)
    size.u.num_matches.num_matches = 7
    comp = _state(N.OP_COMPLETENESS)
    comp.u.num_matches_and_count.num_matches, comp.u.num_matches_and_count.count = 3, 4
    mean = _state(N.OP_MEAN)
    mean.u.mean.sum, mean.u.mean.count = 10.5, 3
    mx = _state(N.OP_MAXIMUM)
    mx.u.dbl.value = -4.25
    sd = _state(N.OP_STANDARD_DEVIATION)
    sd.u.stddev.n, sd.u.stddev.avg, sd.u.stddev.m2 = 3.0, 2.0, 6.0
    absent = _state(N.OP_MINIMUM, present=0)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), N, [size, comp, mean, mx, sd, absent], state_from_native)
    assert sorted(os.listdir(out)) == ["metrics.npy", "present.npy", "states.npy"]
    states, metrics, present = (np.load(out / f) for f in ("states.npy", "metrics.npy", "present.npy"))
    for a in (states, metrics, present):
        assert a.dtype == np.float64 and np.isfinite(a).all()
    np.testing.assert_array_equal(states, np.array([[7, 0, 0], [3, 4, 0], [10.5, 3, 0], [-4.25, 0, 0], [3, 2, 6],
                                                    [0, 0, 0]], dtype=np.float64))
    np.testing.assert_array_equal(metrics, np.array([7.0, 0.75, 3.5, -4.25, np.sqrt(2.0), 0.0]))
    np.testing.assert_array_equal(present, np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0]))
