"""Inputs and state encoding shared by tests/test_gpu_scan_striped_bits.py and tools/scan_bits_golden.py.

The striped scan's per-lane arithmetic, lane -> row mapping and fold order are fixed, so for a given table, row count
and grid (DQ_SCAN_GRID) every field of every state is reproducible to the bit. The golden file records those bits as
produced by the library before the r08 instruction cuts; the test holds every later build to them.
"""
import os
import struct

import numpy as np

import deequ_amd as D
from deequ_amd.table import Table, Column, pack_validity, NUMPY_OF, spark_type_of
import oracle as O

TILE = 2048
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "striped_scan_bits.json")
GRIDS = (1, 2, 3)
SIZES = (1, TILE, 2 * TILE + 2047, 5 * TILE + 1, 7 * TILE + 2047)
SEED = 0x5EED0000
C2_KINDS = (1, 1, 2, 3, 4, 4, 4, 4)  # the benchmark's C2 columns: 4 double, 4 long, 10 per mille NULL


def _columns(specs):
    cols = []
    for name, t, v, valid in specs:
        st = spark_type_of(t)
        cols.append(Column(name, st, np.ascontiguousarray(v.astype(NUMPY_OF[st])),
                           None if valid is None else pack_validity(valid)))
    return Table(cols)


def c2_table(n):
    specs = []
    for c, kind in enumerate(C2_KINDS):
        v = O.synth_column(kind, SEED + c, 0, n)
        valid = O.synth_validity(SEED + 0x100 + c, 0, n, 10)
        specs.append(("c%d" % c, "long" if kind == 4 else "double", v, valid))
    return _columns(specs)


def crafted_table(n):
    """d / l: double / long with 30 % NULL; valid NaN, +-inf and -0.0 rows in d (tiles 1, 2, 4, 5); |x| >= 2^53 in some
    8-row batches of l, mixed with small values; tile 3 all NULL in d and l; g / k: no validity bitmap, g with -0.0 and
    (tile 4) an infinity."""
    rng = np.random.default_rng(n + 8)
    rows = np.arange(n)
    d = rng.normal(50.0, 20.0, n)
    g = rng.normal(-3.0, 1.0, n)
    l = rng.integers(-10 ** 6, 10 ** 6, n, dtype=np.int64)
    k = rng.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)
    vd = rng.random(n) >= 0.3
    vl = rng.random(n) >= 0.3
    for tile in (1, 2, 4, 5):
        for i, sp in enumerate((np.nan, np.inf, -np.inf, -0.0)):
            r = tile * TILE + 41 + 523 * i + tile  # spread over the four loads of a tile and over lanes
            if r < n:
                d[r] = sp
                vd[r] = True
                if sp == 0.0 or (tile == 4 and sp == np.inf):
                    g[r] = sp
    big = rows[(rows // 8) % 5 == 0][::3]
    l[big] = rng.choice(np.array([2 ** 53, -(2 ** 53), 2 ** 62 + 12345, -(2 ** 62) - 1], dtype=np.int64), big.size)
    in3 = (rows >= 3 * TILE) & (rows < 4 * TILE)
    vd[in3] = False
    vl[in3] = False
    if n == 1:
        vd[:] = True
        vl[:] = True
    return _columns([("d", "double", d, vd), ("g", "double", g, None), ("l", "long", l, vl), ("k", "long", k, None)])


LATE_ROWS = 6 * TILE + 1500  # 7 tiles, the last one partial: at grid 2 workgroup 0 folds tiles 0, 2, 4 and 6


def _lane_rows(tile, tid, nrows):
    """Rows of lane `tid` in tile `tile` (P = 2: load j, element e -> tile * 2048 + j * 512 + 2 * tid + e)."""
    r = [tile * TILE + j * 512 + 2 * tid + e for j in range(4) for e in range(2)]
    return [x for x in r if x < nrows]


def late_first_batch_table():
    """A long and a double column at grid 2 over 7 tiles whose lanes meet their first kept batch at different times:
    every row of wave 1's lanes is NULL in each workgroup's first three tiles (tiles 0-5: all the full ones) and valid
    afterwards (the partial tile 6, workgroup 0; in workgroup 1 the wave stays empty); lane 7 of wave 0 is NULL
    throughout; lane 0 of wave 2 is valid only in the partial last tile; wave 3's lanes are NULL in each workgroup's
    first tile only, so their first batch is the second fold of the loop. Elsewhere about 5 % NULL."""
    n = LATE_ROWS
    rng = np.random.default_rng(2024)
    l = rng.integers(-10 ** 9, 10 ** 9, n, dtype=np.int64)
    d = rng.normal(1.0e6, 3.0, n)
    valid = {"l": rng.random(n) >= 0.05, "d": rng.random(n) >= 0.05}
    for v in valid.values():
        for tile in range(7):
            for tid in range(64, 128):
                v[_lane_rows(tile, tid, n)] = tile == 6
            v[_lane_rows(tile, 7, n)] = False
            v[_lane_rows(tile, 128, n)] = tile == 6
            if tile < 2:
                for tid in range(192, 256):
                    v[_lane_rows(tile, tid, n)] = False
    return _columns([("l", "long", l, valid["l"]), ("d", "double", d, valid["d"])])


def analyzers_of(table):
    out = [D.Size()]
    for c in table.columns:
        out += [D.Completeness(c), D.Mean(c), D.Sum(c), D.Minimum(c), D.Maximum(c), D.StandardDeviation(c)]
    return out


def run_states(table, analyzers):
    batch = D.ScanBatch(table)
    offsets = [a.addOps(batch) for a in analyzers]
    res = batch.run()
    return [a.fromAggregationResult(res, ops) for a, ops in zip(analyzers, offsets)]


def encode(state):
    """Every field of a state as text: doubles as the hex of their 8 bytes, everything else by repr."""
    if state is None:
        return None
    return {k: struct.pack("<d", v).hex() if isinstance(v, float) else repr(v) for k, v in sorted(vars(state).items())}


def cases():
    """(key, table builder) of every golden case; the grid is the last part of the key."""
    out = []
    for n in SIZES:
        out.append(("c2/n=%d" % n, lambda n=n: c2_table(n)))
        out.append(("crafted/n=%d" % n, lambda n=n: crafted_table(n)))
    out.append(("late/n=%d" % LATE_ROWS, late_first_batch_table))
    return out
