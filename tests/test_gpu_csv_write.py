"""The device CSV writer (csv_write.hip) against the host path and the model. Bar: bytes, exactly; there
is no tolerance anywhere in this feature.

`Table.to_device(0).to_csv` writes the host path's file for every supported type, with and without NULLs and bitmaps,
at the wave and tile edges; string cells at every length class, with the special bytes astride the 8-, 16- and 64-byte
boundaries of the column's byte buffer, a cell of 4096 quotes and a 200 KB cell; one column and 300 columns; both
routes of the write kernel, alone and in neighbouring tiles; a kept dictionary; a ChunkedTable; the number-text cases
of test_gpu_number_text.py; the law through from_csv(device=0); launch counts that do not depend on the rows."""
import numpy as np
import pytest

import deequ_amd as D
from deequ_amd import engine
from deequ_amd import native as N
from deequ_amd.table import ChunkedTable, Column, DictColumn, Table, pack_validity
import csv_export_cases as E
import csv_write_cases as W
import csv_write_model as M
import number_text_cases as C

pytestmark = pytest.mark.gpu


def fresh(table):
    """A copy of a host table's columns in a new Table (to_device marks the columns it is given)."""
    import copy
    return Table([copy.copy(c) for c in table.columns.values()])


def device_bytes(tmp_path, table, header=True, name="dev.csv"):
    p = str(tmp_path / name)
    n = fresh(table).to_device(0).to_csv(p, header=header)
    data = open(p, "rb").read()
    assert n == len(data)
    return p, data


def host_bytes(tmp_path, table, header=True):
    p = str(tmp_path / "host.csv")
    table.to_csv(p, header=header)
    return open(p, "rb").read()


def body_of(table):
    """The body through the tensor interface (no disk): Context.csv_write."""
    t = fresh(table).to_device(0)
    out = engine.ctx().csv_write([c.native() for c in t.columns.values()], t.nrows, 0)
    return out.cpu().numpy().tobytes()


def routes():
    return engine.ctx().csv_write_routes()


def routes_since(before):
    now = routes()
    return {k: now[k] - before[k] for k in now}


# ---- device equals host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_every_type_at_the_wave_and_tile_edges(tmp_path, n):
    for nulls, bitmap in ((True, True), (False, True), (False, False)):
        t = W.every_type_table(n, seed=n + 1, nulls=nulls, bitmap=bitmap)
        want = M.file_bytes(t)
        assert host_bytes(tmp_path, t) == want
        assert device_bytes(tmp_path, t)[1] == want, (n, nulls, bitmap)


def test_without_header(tmp_path):
    t = W.every_type_table(130)
    assert device_bytes(tmp_path, t, header=False)[1] == M.body(t) == body_of(t)


# ---- string cells ---------------------------------------------------------------------------------------------------
def _placed(length, where, byte):
    cell = bytearray(b"x" * length)
    if length:
        cell[{"first": 0, "last": length - 1, "mid": length // 2}[where]] = byte
    return bytes(cell)


def test_string_cell_lengths_and_special_bytes_at_their_places(tmp_path):
    cells = []
    for length in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65):
        cells.append(b"x" * length)
        for byte in b',"\n\r':
            for where in ("first", "last", "mid"):
                cells.append(_placed(length, where, byte))
    t = Table([W.bytes_column("c", cells), W.bytes_column("d", cells[::-1])])
    assert device_bytes(tmp_path, t)[1] == M.file_bytes(t)


@pytest.mark.parametrize("boundary", [8, 16, 64, 16384])
def test_special_bytes_across_a_boundary_of_the_byte_buffer(tmp_path, boundary):
    """Cells that start 0..3 bytes before a multiple of `boundary` in the column's byte buffer and run 2..5 bytes past
    it, the special byte on either side of the boundary: the bit ranges of the mark pass and the lane's word walk."""
    cells = []
    at = 0
    for back in range(0, 4):
        for byte in b',"\n\r':
            for side in (-1, 0):
                pad = (-at - back) % boundary or boundary  # a filler cell that ends `back` bytes before the boundary
                cells.append(b"p" * pad)
                at += pad
                cell = bytearray(b"y" * (back + 3))
                if 0 <= back + side < len(cell):
                    cell[back + side] = byte
                cells.append(bytes(cell))
                at += len(cell)
    t = Table([W.bytes_column("c", cells)])
    assert device_bytes(tmp_path, t)[1] == M.file_bytes(t)


def test_a_cell_of_4096_quotes_and_a_200_kb_cell(tmp_path):
    big = (b"0123456789abcdef" * 12800)[:200_000]
    holed = bytearray(big)
    holed[0:1], holed[70_001:70_002], holed[-1:] = b'"', b",", b'"'
    cells = [b"a", b'"' * 4096, b"b", big, bytes(holed), b"", b"c" * 100, b'"' + b"d" * 99]
    t = Table([W.bytes_column("c", cells), Column("n", N.TYPE_INT, np.arange(len(cells), dtype=np.int32))])
    before = routes()
    assert device_bytes(tmp_path, t)[1] == M.file_bytes(t)
    assert routes_since(before) == {"stage": 0, "direct": 1}  # larger than any LDS stage


# ---- wide tables ----------------------------------------------------------------------------------------------------
def test_one_column(tmp_path):
    t = Table([Column("n", N.TYPE_LONG, np.arange(-300, 300, dtype=np.int64), pack_validity(np.arange(600) % 5 != 0))])
    assert device_bytes(tmp_path, t)[1] == M.file_bytes(t)


def test_300_narrow_columns_of_5_rows_exceed_the_stage(tmp_path):
    rng = np.random.default_rng(2)
    cols = []
    for k in range(300):
        if k % 3 == 2:
            cols.append(W.strings_column("c%d" % k, ["w%d,%d" % (k, r) if r % 2 else "v" * 60 for r in range(5)]))
        else:
            cols.append(Column("c%d" % k, N.TYPE_DOUBLE, rng.normal(0, 1e6, 5)))
    t = Table(cols)
    want = M.file_bytes(t)
    assert len(M.body(t)) > N.CSV_WRITE_STAGE_BYTES
    before = routes()
    assert device_bytes(tmp_path, t)[1] == want
    assert routes_since(before) == {"stage": 0, "direct": 1}


# ---- routing --------------------------------------------------------------------------------------------------------
def test_neighbouring_tiles_take_different_routes(tmp_path):
    """Tiles of 256 rows: tile 0 and 2 are short rows (stage), tile 1 holds 256 cells of 200 bytes (direct), tile 3 one
    40 KB cell among short rows (direct), tile 4 is a partial tile (stage)."""
    rows = N.CSV_WRITE_TILE_ROWS
    cells = [b"s%d" % r for r in range(rows)] + [(b"L%03d," % r) + b"z" * 195 for r in range(rows)] + \
            [b"t%d" % r for r in range(rows)] + [b"u"] * 100 + [b'"q"' * 13400] + [b"u"] * 155 + [b"end"] * 17
    t = Table([Column("n", N.TYPE_INT, np.arange(len(cells), dtype=np.int32)), W.bytes_column("c", cells)])
    before = routes()
    assert device_bytes(tmp_path, t)[1] == M.file_bytes(t)
    assert routes_since(before) == {"stage": 3, "direct": 2}


def test_the_stage_threshold(tmp_path):
    """One tile whose body is a few bytes below, at and above the stage: both sides of the routing decision."""
    for extra in (-40, -17, -16, -1, 0, 1, 16):
        target = N.CSV_WRITE_STAGE_BYTES + extra
        cells = [b"k" * (target - 2 * 255 - 1)] + [b"r"] * 255  # 256 rows: each cell + LF
        t = Table([W.bytes_column("c", cells)])
        body = M.body(t)
        assert len(body) == target
        before = routes()
        assert body_of(t) == body, extra
        # the output tensor is 16-byte aligned, so the span needs no alignment shift in the stage
        assert routes_since(before) == ({"stage": 0, "direct": 1} if extra > 0 else {"stage": 1, "direct": 0}), extra


# ---- other inputs ---------------------------------------------------------------------------------------------------
def test_kept_dictionary_column(tmp_path):
    import pyarrow as pa
    rng = np.random.default_rng(8)
    entries = ["a,b", "plain", "", 'q"', None, "é", "x" * 70]
    idx = rng.integers(0, len(entries), 700).astype(np.int32)
    arr = pa.DictionaryArray.from_arrays(pa.array(idx, mask=rng.random(700) < 0.1), pa.array(entries, type=pa.string()))
    t = Table.from_arrow(pa.table({"k": arr, "n": pa.array(np.arange(700), type=pa.int64())}), dictionaries="keep")
    assert isinstance(t["k"], DictColumn)
    want = host_bytes(tmp_path, t)
    ctx = engine.ctx()
    before, wbefore = ctx.kernel_launches(), ctx.csv_kernel_launches()
    p = str(tmp_path / "dict.csv")
    dt = Table.from_arrow(pa.table({"k": arr, "n": pa.array(np.arange(700), type=pa.int64())}), dictionaries="keep",
                          device=0)
    assert isinstance(dt["k"], DictColumn)
    dt.to_csv(p)
    assert open(p, "rb").read() == want
    moved = {k: v - before[k] for k, v in ctx.kernel_launches().items() if v != before[k]}
    assert set(moved) <= {"dict_decode"} and ctx.csv_kernel_launches() == wbefore


def test_chunked_table_of_three_chunks(tmp_path):
    whole = W.every_type_table(700, seed=3)
    parts = [whole.select_rows(np.arange(700) // 250 == k).to_device(0) for k in range(3)]
    for header in (True, False):
        p = str(tmp_path / "chunks.csv")
        n = ChunkedTable(parts).to_csv(p, header=header)
        assert open(p, "rb").read() == M.file_bytes(whole, header) and n == len(M.file_bytes(whole, header))


# ---- special values and the number-text cases -----------------------------------------------------------------------
def test_number_text_cases_through_the_writer():
    doubles, floats = C.format_cases(103)
    sp = C.format_special_values()
    doubles = np.concatenate([doubles, np.array(sp, np.float64)])
    floats = np.concatenate([floats, np.array(sp, np.float32)])
    assert len(doubles) >= 6000 and len(floats) >= 6000
    want_d, want_f = C.oracle_texts(doubles, floats)
    for name, spark_type, vals, want in (("d", N.TYPE_DOUBLE, doubles, want_d), ("f", N.TYPE_FLOAT, floats, want_f)):
        t = Table([Column(name, spark_type, vals)])
        assert body_of(t).decode().split("\n")[:-1] == want, name
        assert body_of(t) == M.body(t)


def test_integral_decimal_date_and_timestamp_values():
    rng = np.random.default_rng(6)
    n = 6000
    longs = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
    longs[:4] = [-2 ** 63, 2 ** 63 - 1, 0, -1]
    dec = (longs // 10) % 10 ** 18
    t = Table([Column("l", N.TYPE_LONG, longs), Column("i", N.TYPE_INT, longs.astype(np.int32)),
               Column("s", N.TYPE_SHORT, longs.astype(np.int16)), Column("b", N.TYPE_BYTE, longs.astype(np.int8)),
               Column("p", N.TYPE_DECIMAL, dec - 10 ** 17, decimal_precision=18, decimal_scale=0),
               Column("q", N.TYPE_DECIMAL, dec % 1000 - 500, decimal_precision=18, decimal_scale=9),
               Column("r", N.TYPE_DECIMAL, dec - 10 ** 17, decimal_precision=18, decimal_scale=18),
               Column("day", N.TYPE_DATE, rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)),
               Column("ts", N.TYPE_TIMESTAMP, rng.integers(-2 ** 58, 2 ** 58, n))])
    assert body_of(t) == M.body(t)


# ---- round trip -----------------------------------------------------------------------------------------------------
def _law(path, table):
    back = Table.from_csv(path, device=0, infer_schema=False).to_host()
    assert back.fieldNames == table.fieldNames and back.nrows == table.nrows
    for col, want in zip(back.columns.values(), M.law_cells(table)):
        assert col.type_name == "StringType"
        assert [M.cell_text(col, i) for i in range(back.nrows)] == want, col.name


def test_the_law_through_the_device_reader(tmp_path):
    t = W.every_type_table(300, seed=14)
    p, _ = device_bytes(tmp_path, t)
    _law(p, t)
    cells = W.reader_alphabet_cells(600, seed=15)
    for t in (Table([W.bytes_column("c", cells, [k % 9 != 4 for k in range(600)])]),
              Table([W.bytes_column("a", cells[:300]), W.bytes_column("b,c", cells[300:])])):
        p, data = device_bytes(tmp_path, t)
        assert data == M.file_bytes(t)
        _law(p, t)


def test_round_trippable_table_comes_back_with_equal_buffers(tmp_path):
    t = W.round_trippable(300)
    p, _ = device_bytes(tmp_path, t)
    back = Table.from_csv(p, device=0)
    assert back.schema == t.schema
    E.assert_same_buffers(t, back.to_host(), null_slots=False)
    host = Table.from_csv(p)
    E.assert_same_buffers(t, host)


# ---- launch counts --------------------------------------------------------------------------------------------------
def test_launch_counts_do_not_depend_on_the_rows():
    ctx = engine.ctx()
    deltas = []
    for n in (10, 10_000):
        t = W.every_type_table(n, seed=n)
        scan_before, csv_before, ingest_before = ctx.kernel_launches(), ctx.csv_kernel_launches(), ctx.ingest_kernel_launches()
        before = ctx.csv_write_kernel_launches()
        assert body_of(t) == M.body(t)
        after = ctx.csv_write_kernel_launches()
        deltas.append({k: after[k] - before[k] for k in after})
        assert (ctx.kernel_launches(), ctx.csv_kernel_launches(), ctx.ingest_kernel_launches()) == \
            (scan_before, csv_before, ingest_before)
    assert deltas[0] == deltas[1] == {"csv_write_mark": 2, "csv_write_sizes": 1, "csv_write_write": 1}


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_decimal128_is_refused_by_name(tmp_path):
    from decimal import Decimal
    t = Table.from_pydict({"ok": [1, 2], "wide": [Decimal("1.5"), None]}, types={"ok": "int", "wide": "decimal(38,10)"})
    t.to_device(0)
    with pytest.raises(ValueError, match="wide"):
        t.to_csv(str(tmp_path / "w.csv"))
    with pytest.raises(N.NativeError) as e:  # and by the C-ABI, by index
        engine.ctx().csv_write([c.native() for c in t.columns.values()], 2, 0)
    assert e.value.status == -2 and "column 1" in str(e.value)


def test_a_body_at_the_size_limit_is_refused_with_its_size():
    """The 2^31-byte limit, shown at a small one (the same comparison in Context.csv_write): refused after the sizing
    call, before the body is allocated, with the size and the way out."""
    t = W.every_type_table(100).to_device(0)
    cols = [c.native() for c in t.columns.values()]
    size = len(M.body(t))
    assert len(engine.ctx().csv_write(cols, 100, 0, limit=size + 1)) == size
    with pytest.raises(ValueError, match=r"%d bytes.*2\^31.*ChunkedTable" % size):
        engine.ctx().csv_write(cols, 100, 0, limit=size)


def test_a_multi_device_context_is_refused():
    import os
    os.environ.pop("DQ_DEVICES", None)
    ctx3 = N.Context(devices=[0, 0])
    t = W.every_type_table(10).to_device(0)
    with pytest.raises(N.NativeError) as e:
        ctx3.csv_write([c.native() for c in t.columns.values()], 10, 0)
    assert e.value.status == -2 and "multi-device" in str(e.value)
    ctx3.close()


def test_a_wrong_output_size_is_refused_before_anything_is_written():
    import torch
    t = W.every_type_table(10).to_device(0)
    cols = [c.native() for c in t.columns.values()]
    ctx = engine.ctx()
    row_start = torch.empty(11, dtype=torch.int64, device="cuda:0")
    total = ctx.csv_write_size(cols, 10, row_start.data_ptr())
    out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(N.NativeError) as e:
        ctx.csv_write_body(cols, 10, row_start.data_ptr(), out.data_ptr(), total - 1)
    assert e.value.status == -1
    assert int(out.sum().item()) == 0
