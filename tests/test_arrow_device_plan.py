"""The host side of Table.from_arrow(t, device=d) that needs no GPU: the row-range planner against a brute-force row
map, the argument checks, and the C-ABI's book-keeping (symbols, kernel counters)."""
import os
import random
import re

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import deequ_amd.native as N
from deequ_amd.table import Table, _arrow_pieces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(lengths, offsets, chunk_rows):
    """[(arrow chunk, row in its buffers)] of every output row, cut into the output chunks."""
    rows = [(c, offsets[c] + i) for c, n in enumerate(lengths) for i in range(n)]
    k = len(rows) if chunk_rows is None or len(rows) <= chunk_rows else chunk_rows
    return [rows[r0:r0 + k] for r0 in range(0, len(rows), k)] if rows else [[]]


def expand(plan):
    out = []
    for pieces in plan:
        rows, at = [], 0
        for c, first, n, row0 in pieces:
            assert n > 0 and row0 == at  # never empty, consecutive inside the output chunk
            rows += [(c, first + i) for i in range(n)]
            at += n
        out.append(rows)
    return out


def test_planner_equals_the_brute_force_row_map():
    rng = random.Random(11)
    for trial in range(500):
        nchunks = rng.choice([0, 1, 1, 2, 3, 5, 9])
        lengths = [rng.choice([0, 0, 1, 2, 7, 8, 63, 64, 65, rng.randrange(200)]) for _ in range(nchunks)]
        offsets = [rng.choice([0, 0, 1, 7, 8, 9, 63, 64, 65, rng.randrange(1000)]) for _ in range(nchunks)]
        total = sum(lengths)
        chunk_rows = rng.choice([None, 1, 2, 7, 8, 64, 100, max(total - 1, 1), max(total, 1), total + 1])
        plan = _arrow_pieces(lengths, offsets, chunk_rows)
        assert expand(plan) == brute_force(lengths, offsets, chunk_rows), (lengths, offsets, chunk_rows)
        if chunk_rows is not None and total > chunk_rows:
            assert [sum(p[2] for p in pieces) for pieces in plan][:-1] == [chunk_rows] * (len(plan) - 1)


def test_planner_edge_shapes():
    assert _arrow_pieces([], [], None) == [[]]  # a column without chunks
    assert _arrow_pieces([0, 0], [3, 4], 5) == [[]]  # only empty chunks
    assert _arrow_pieces([3, 0, 5], [1, 0, 2], 4) == [[(0, 1, 3, 0), (2, 2, 1, 3)], [(2, 3, 4, 0)]]
    assert _arrow_pieces([4], [0], 4) == [[(0, 0, 4, 0)]]  # the rows fit one chunk: one output chunk
    with pytest.raises(ValueError):
        _arrow_pieces([4], [0], 0)


def test_chunk_rows_without_device_raises(tmp_path):
    t = pa.table({"a": [1, 2, 3]})
    with pytest.raises(ValueError, match="device"):
        Table.from_arrow(t, chunk_rows=2)
    p = str(tmp_path / "t.parquet")
    pq.write_table(t, p)
    with pytest.raises(ValueError, match="device"):
        Table.from_parquet(p, chunk_rows=2)
    assert Table.from_arrow(t).nrows == 3 and Table.from_parquet(p).nrows == 3  # the host path is as it was


def header():
    return open(os.path.join(ROOT, "include", "dq.h")).read()


def test_kernel_counters_extend_the_enum_without_moving_it():
    assert len(N.INGEST_KERNELS) > 0
    assert len(N.SCAN_KERNELS) == 18 and len(N.CSV_KERNELS) == 5
    entries = dict(re.findall(r"\b(DQ_KERNEL_[A-Z0-9_]+)\s*=\s*(\d+)", header()))
    assert int(entries["DQ_KERNEL_CSV_COLUMN"]) == 22
    assert int(entries["DQ_KERNEL_COUNT"]) == 18 + 5 + len(N.INGEST_KERNELS)
    ingest = sorted((int(v), k) for k, v in entries.items() if k.startswith("DQ_KERNEL_INGEST_"))
    assert [k[len("DQ_KERNEL_"):].lower() for _, k in ingest] == list(N.INGEST_KERNELS)
    assert [v for v, _ in ingest] == list(range(23, 23 + len(N.INGEST_KERNELS)))


def test_every_ingest_symbol_is_exported():
    names = set(re.findall(r"\b(dq_ingest_[a-z0-9_]+)\s*\(", header()))
    assert names and names <= set(N.EXPORTED_SYMBOLS)
    lib = N.load_library()
    for s in names:
        assert hasattr(lib, s), s
    assert re.search(r"#define DQ_ABI_VERSION 2\b", header())
