"""The striped scan's tile loop at small sizes (gpu).

DQ_SCAN_GRID caps every scan group's grid, so a handful of tiles gives each workgroup the loop's first tile, its
steady state (a prefetched tile folded while the next one loads), its last tile with an odd or an even number of
full tiles, and the partial last tile. Without the cap only inputs of millions of rows give a workgroup a second
tile. All results are held to the exact oracle through test_gpu_scan.assert_state_parity (1e-12 / exact rules).
"""
import math
import struct

import numpy as np
import pytest

import deequ_amd as D
from deequ_amd.table import Table, Column, pack_validity, NUMPY_OF, spark_type_of
import oracle as O
from test_gpu_scan import random_table, all_analyzers, assert_state_parity

pytestmark = pytest.mark.gpu

TILE = 2048
SIZES = [T * TILE + r for T in range(8) for r in (0, 1, 2047)]
WHERE = "k < 25"


@pytest.fixture(autouse=True)
def _oracle_once(monkeypatch):
    """The oracle's answers for one table are computed once and shared by every analyzer and grid held to them
    (the cache keeps the table alive, so its id stays its own)."""
    def once(fn):
        def cached(table, *args, **kw):
            key = (fn.__name__, id(table), repr(args), repr(sorted(kw.items())))
            if key not in _ORACLE:
                _ORACLE[key] = (table, fn(table, *args, **kw))
            return _ORACLE[key][1]
        return cached

    for name in ("expected_state", "column_stats", "predicate_masks"):
        monkeypatch.setattr(O, name, once(getattr(O, name)))


_ORACLE = {}
_TABLES = {}


def _random(n):
    if n not in _TABLES:
        _TABLES[n] = random_table(np.random.default_rng(n + 101), n, with_nan=(n % 2 == 1)).to_device()
    return _TABLES[n]


def _states(table, analyzers):
    batch = D.ScanBatch(table)
    offsets = [a.addOps(batch) for a in analyzers]
    res = batch.run()
    return [a.fromAggregationResult(res, ops) for a, ops in zip(analyzers, offsets)]


def _check(table, analyzers):
    for a, got in zip(analyzers, _states(table, analyzers)):
        assert_state_parity(table, a, got)


# ---- 1. every pipeline stage at small sizes ---------------------------------------------------------
@pytest.mark.parametrize("where", [None, WHERE])
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_every_stage_small_sizes(monkeypatch, grid, where):
    monkeypatch.setenv("DQ_SCAN_GRID", str(grid))
    for n in SIZES:
        t = _random(n)
        _check(t, all_analyzers(t, where))


# ---- 2. crafted 8-byte columns at grid 2 ------------------------------------------------------------
def _crafted(n):
    """d: double with NaN, +-inf and -0.0 in tiles 2-5 (the second and third tile of both workgroups at grid 2);
    l: long with |x| >= 2^53 in some batches; g / k: no validity bitmap; tile 3 all NULL in d and l; the first batch
    of lane 5 (tile 0, workgroup 0) and of lane 9 (tile 1, workgroup 1) all NULL; about 30 % NULL elsewhere."""
    rng = np.random.default_rng(n + 7)
    rows = np.arange(n)
    d = rng.normal(50.0, 20.0, n)
    g = rng.normal(-3.0, 1.0, n)
    l = rng.integers(-10 ** 6, 10 ** 6, n, dtype=np.int64)
    k = rng.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)
    vd = rng.random(n) >= 0.3
    vl = rng.random(n) >= 0.3
    specials = [np.nan, np.inf, -np.inf, -0.0]
    for tile in (2, 3, 4, 5):
        for i, sp in enumerate(specials):
            r = tile * TILE + 37 + 523 * i + tile  # spread over the four loads of a tile and over lanes
            if r < n:
                d[r] = sp
                vd[r] = tile != 3
                g[r] = -0.0 if sp == 0.0 else (sp if tile == 4 else g[r])
    big = rows[(rows // 8) % 5 == 0][::3]  # a few rows of every fifth 8-row group: mixed with small values
    l[big] = rng.choice(np.array([2 ** 53, -(2 ** 53), 2 ** 62 + 12345, -(2 ** 62) - 1], dtype=np.int64), big.size)
    in3 = (rows >= 3 * TILE) & (rows < 4 * TILE)
    vd[in3] = False
    vl[in3] = False
    for tile, lane in ((0, 5), (1, 9)):
        for j in range(4):
            for e in range(2):
                r = tile * TILE + j * 512 + lane * 2 + e
                if r < n:
                    vd[r] = False
                    vl[r] = False
    cols = []
    for name, t, v, valid in (("d", "double", d, vd), ("g", "double", g, None), ("l", "long", l, vl),
                              ("k", "long", k, None)):
        st = spark_type_of(t)
        cols.append(Column(name, st, np.ascontiguousarray(v.astype(NUMPY_OF[st])),
                           None if valid is None or valid.all() else pack_validity(valid)))
    return Table(cols)


def _column_analyzers(table, where=None):
    out = [D.Size(where)]
    for c in table.columns:
        out += [D.Completeness(c, where), D.Mean(c, where), D.Sum(c, where), D.Minimum(c, where),
                D.Maximum(c, where), D.StandardDeviation(c, where)]
    return out


@pytest.mark.parametrize("where", [None, "l < 500000"])
def test_crafted_eight_byte_columns_grid_2(monkeypatch, where):
    monkeypatch.setenv("DQ_SCAN_GRID", "2")
    for n in SIZES:
        if ("crafted", n) not in _TABLES:
            _TABLES[("crafted", n)] = _crafted(n).to_device()
        t = _TABLES[("crafted", n)]
        analyzers = _column_analyzers(t, where)
        for a, got in zip(analyzers, _states(t, analyzers)):
            if isinstance(a, D.StandardDeviation) and _selects_infinity(t, a):
                # Spark's own update order turns an infinity among the rows into inf - inf: m2 is NaN and the mean
                # NaN (or still infinite when the infinity is merged last), where the exact oracle reports the
                # mathematical mean. The count stays exact.
                exp = O.expected_state(t, a, exact=True)
                assert got.n == exp.n and math.isnan(got.m2) and not math.isfinite(got.avg), (n, a, got, exp)
                continue
            assert_state_parity(t, a, got)


def _selects_infinity(table, analyzer):
    c = table[analyzer.column]
    if c.values.dtype.kind != "f":
        return False
    keep = O._valid(c)
    if analyzer.where is not None:
        keep = keep & O.predicate_masks(table, analyzer.where)[0]
    return bool(np.isinf(c.values[keep]).any())


# ---- 3. grid independence of the exact fields -------------------------------------------------------
def _bits(state):
    if state is None:
        return None
    out = []
    for key, v in sorted(vars(state).items()):
        out.append((key, struct.pack("<d", v) if isinstance(v, float) else repr(v)))
    return tuple(out)


INTEGRAL = ("l", "i", "s", "b", "dec", "k")


def _exact_fields(analyzer, state):
    name = type(analyzer).__name__
    if state is None:
        return None
    if name in ("Size", "Completeness", "Compliance", "Minimum", "Maximum", "ApproxCountDistinct"):
        return _bits(state)
    if name == "Mean":
        return (state.count, struct.pack("<d", state.sum_) if analyzer.column in INTEGRAL else None)
    if name == "Sum":
        return struct.pack("<d", state.sum_) if analyzer.column in INTEGRAL else math.isnan(state.sum_)
    return state.n  # StandardDeviation, Correlation


def test_exact_fields_do_not_depend_on_the_grid(monkeypatch):
    t = random_table(np.random.default_rng(77), 20000, with_nan=True).to_device()
    analyzers = all_analyzers(t)
    monkeypatch.delenv("DQ_SCAN_GRID", raising=False)
    base = _states(t, analyzers)
    assert [_bits(s) for s in _states(t, analyzers)] == [_bits(s) for s in base]
    for grid in (1, 2, 3):
        monkeypatch.setenv("DQ_SCAN_GRID", str(grid))
        first = _states(t, analyzers)
        again = _states(t, analyzers)
        assert [_bits(s) for s in first] == [_bits(s) for s in again], grid
        for a, s, b in zip(analyzers, first, base):
            assert _exact_fields(a, s) == _exact_fields(a, b), (grid, a, s, b)


# ---- 4. the planner's own grid: every workgroup folds several tiles ----------------------------------
def test_default_grid_many_tiles_per_workgroup(monkeypatch):
    monkeypatch.delenv("DQ_SCAN_GRID", raising=False)
    n = 4100 * TILE + 77
    rng = np.random.default_rng(3)
    t = Table.from_arrays({"x": rng.normal(10.0, 3.0, n), "k": rng.integers(-10 ** 9, 10 ** 9, n)},
                          validity={"x": rng.random(n) >= 0.01, "k": rng.random(n) >= 0.01}).to_device()
    _check(t, _column_analyzers(t))
