"""Table.to_csv on the host: the plain Python path that defines the file. No GPU. It equals the model of
tests/csv_write_model.py (oracle.spark_cast_to_string + the quoting rule) byte for byte and hand-written literal files;
read back through the host reader it satisfies the law (same names, every cell its text, NULL exactly where the cell
was NULL or the empty string); and no file it writes is one the device reader refuses (tests/csv_model.py)."""
import csv
import io
from decimal import Decimal

import numpy as np
import pytest

from deequ_amd import native as N
from deequ_amd.table import ChunkedTable, Column, Table, pack_validity
import csv_model as R
import csv_write_cases as W
import csv_write_model as M
import number_text_cases as C


def written(tmp_path, table, header=True, name="t.csv"):
    p = str(tmp_path / name)
    n = table.to_csv(p, header=header)
    data = open(p, "rb").read()
    assert n == len(data)
    return p, data


def check_law(path, table, reader):
    """`reader(path)` -> an all-STRING table: the law of §3k."""
    back = reader(path)
    assert back.fieldNames == table.fieldNames
    assert back.nrows == table.nrows
    for col, want in zip(back.columns.values(), M.law_cells(table)):
        assert col.type_name == "StringType"
        got = [M.cell_text(col, i) for i in range(back.nrows)]
        assert got == want, col.name


def host_reader(path):
    return Table.from_csv(path, infer_schema=False)


def col(name, spark_type, values, valid=None, **kw):
    return Column(name, spark_type, np.asarray(values), None if valid is None else pack_validity(valid), **kw)


HARD = [
    # NULL against the empty string; a cell that is only a quote; a,b; LF, a lone CR and CR LF inside a cell; UTF-8
    (lambda: Table([W.bytes_column("s", [b"", b"", b'"', b"a,b", b"x\ny", b"x\ry", b"x\r\ny", "é日本".encode(), b"plain"],
                                   [False, True, True, True, True, True, True, True, True]),
                    col("n", "int", [1, 2, 3, 4, 5, 6, 7, 8, 9], [True, True, False, True, True, True, True, True, True])]),
     True,
     b's,n\n,1\n"",2\n"""",\n"a,b",4\n"x\ny",5\n"x\ry",6\n"x\r\ny",7\n' + "é日本".encode() + b',8\nplain,9\n'),
    # a one-column row that is NULL is an empty line
    (lambda: Table([col("n", "long", [1, 0, 3], [True, False, True])]), True, b"n\n1\n\n3\n"),
    # zero rows, with and without header
    (lambda: Table([col("a", "int", np.zeros(0, np.int32)), W.bytes_column("b", [])]), True, b"a,b\n"),
    (lambda: Table([col("a", "int", np.zeros(0, np.int32)), W.bytes_column("b", [])]), False, b""),
    # names that need quoting
    (lambda: Table([col("a,b", "int", [1]), col('q"', "int", [2]), col("", "int", [3]), col("new\nline", "int", [4])]),
     True, b'"a,b","q""","","new\nline"\n1,2,3,4\n'),
    (lambda: Table([col("a,b", "int", [1])]), False, b"1\n"),
    # doubles and floats
    (lambda: Table([col("d", "double", [-0.0, float("nan"), 1e10, 1e-5, float("inf"), 100.0, 0.001, 1e7, 1234567.0]),
                    col("f", "float", np.array([-0.0, np.nan, 1e10, 1e-5, -np.inf, 0.1, 1.5, 1e7, 16777216.0], np.float32))]),
     True, b"d,f\n-0.0,-0.0\nNaN,NaN\n1.0E10,1.0E10\n1.0E-5,1.0E-5\nInfinity,-Infinity\n100.0,0.1\n0.001,1.5\n1.0E7,1.0E7\n"
           b"1234567.0,1.6777216E7\n"),
    # decimals: BigDecimal.toString goes scientific below an adjusted exponent of -6
    (lambda: Table([col("p", "decimal", np.array([1, 10, -15, 0, 123456789], np.int64), decimal_precision=10, decimal_scale=8),
                    col("q", "decimal", np.array([1, 10, -15, 0, 123456789], np.int64), decimal_precision=10, decimal_scale=7),
                    col("r", "decimal", np.array([1, 10, -15, 0, 123456789], np.int64), decimal_precision=10, decimal_scale=0)]),
     True, b"p,q,r\n1E-8,1E-7,1\n1.0E-7,0.0000010,10\n-1.5E-7,-0.0000015,-15\n0E-8,0E-7,0\n1.23456789,12.3456789,123456789\n"),
    # dates on both sides of the 1582 cutover, the first Julian day, a five-digit year
    (lambda: Table([col("day", "date", np.array([-141428, -141427, -719164, 0, 2932897], np.int32))]), True,
     b"day\n1582-10-04\n1582-10-15\n0001-01-01\n1970-01-01\n10000-01-01\n"),
    # timestamps with and without a fraction, before the epoch
    (lambda: Table([col("ts", "timestamp", np.array([0, 1500000, -1, 1000001, 86399999990], np.int64))]), True,
     b"ts\n1970-01-01 00:00:00\n1970-01-01 00:00:01.5\n1969-12-31 23:59:59.999999\n1970-01-01 00:00:01.000001\n"
     b"1970-01-01 23:59:59.99999\n"),
    # booleans and the small integers
    (lambda: Table([col("t", "boolean", np.array([1, 0, 1], np.uint8), [True, True, False]),
                    col("b", "byte", np.array([-128, 127, 0], np.int8)), col("s", "short", np.array([-32768, 7, 0], np.int16)),
                    col("l", "long", np.array([-2 ** 63, 2 ** 63 - 1, 0], np.int64))]),
     True, b"t,b,s,l\ntrue,-128,-32768,-9223372036854775808\nfalse,127,7,9223372036854775807\n,0,0,0\n"),
]


@pytest.mark.parametrize("k", range(len(HARD)))
def test_hard_cases_equal_their_literal_files_and_the_model(tmp_path, k):
    make, header, literal = HARD[k]
    t = make()
    _, data = written(tmp_path, t, header)
    assert data == literal
    assert M.file_bytes(t, header) == literal


@pytest.mark.parametrize("n,nulls,bitmap", [(0, True, True), (1, True, True), (97, True, True), (97, False, True),
                                            (97, False, False)])
def test_host_file_equals_the_model(tmp_path, n, nulls, bitmap):
    t = W.every_type_table(n, nulls=nulls, bitmap=bitmap)
    p, data = written(tmp_path, t)
    assert data == M.file_bytes(t)
    check_law(p, t, host_reader)
    _, body = written(tmp_path, t, header=False, name="nh.csv")
    assert body == M.body(t) and data == M.header(t.fieldNames) + body


def test_number_text_of_the_host_path_equals_the_oracle(tmp_path):
    """The host path's own Double.toString / Float.toString (numpy's shortest digits in Java's layout) over the values
    the device formatter is pinned with."""
    doubles, floats = C.format_cases(103)
    n = min(len(doubles), len(floats))
    t = Table([col("d", "double", doubles[:n]), col("f", "float", floats[:n])])
    _, data = written(tmp_path, t, header=False)
    want_d, want_f = C.oracle_texts(doubles[:n], floats[:n])
    assert data.decode().split("\n")[:-1] == [a + "," + b for a, b in zip(want_d, want_f)]


def test_round_trippable_table_comes_back_with_its_types_and_values(tmp_path):
    t = W.round_trippable()
    assert dict(t.schema) == {"big": "LongType", "n": "IntegerType", "x": "DoubleType", "ok": "BooleanType",
                              "w": "StringType"}
    p, _ = written(tmp_path, t)
    back = Table.from_csv(p)
    assert back.schema == t.schema and back.nrows == t.nrows
    for name in t.fieldNames:
        a, b = t[name], back[name]
        assert np.array_equal(np.asarray(a.values).view(np.uint8), np.asarray(b.values).view(np.uint8)), name
        assert (a.validity is None) == (b.validity is None), name
        assert a.validity is None or np.array_equal(a.validity, b.validity), name
        if a.spark_type == N.TYPE_STRING:
            assert np.array_equal(a.offsets, b.offsets)


def test_random_cells_over_the_reader_alphabet_are_never_refused_and_survive(tmp_path):
    """The CPU proof that the device reader accepts what the writer writes: the refusal rules and the record reader of
    tests/csv_model.py, and csv.reader, over files of random cells of , " LF CR 1 a . space - é."""
    cells = W.reader_alphabet_cells(600)
    one = Table([W.bytes_column("c", cells)])
    two = Table([W.bytes_column("a", cells[:300]), W.bytes_column("b", cells[300:])])
    for t, rows in ((one, [[c] for c in cells]), (two, [list(r) for r in zip(cells[:300], cells[300:])])):
        _, data = written(tmp_path, t)
        assert R.refusal(data) is None
        want = [[c.decode("utf-8") for c in r] for r in rows]
        got = R.records(data)[1:]
        # a record of zero bytes (a one-column row holding the empty... no: "" is written for it) never occurs here
        assert got == want
        assert list(csv.reader(io.StringIO(data.decode("utf-8"), newline="")))[1:] == want
        # one file per cell as well: the cell alone, first and last in its file
    for c in cells[:200]:
        data = M.file_bytes(Table([W.bytes_column("c", [c])]), with_header=False)
        assert R.refusal(data) is None and R.records(data) == [[c.decode("utf-8")]]


def test_law_through_the_host_reader_for_strings(tmp_path):
    cells = W.reader_alphabet_cells(200, seed=12)
    valid = [k % 7 != 3 for k in range(len(cells))]
    t = Table([W.bytes_column("c", cells, valid), W.bytes_column("d", cells[::-1])])
    p, _ = written(tmp_path, t)
    check_law(p, t, host_reader)


def test_chunked_table_writes_the_file_of_the_concatenation(tmp_path):
    whole = W.every_type_table(50)
    parts = [whole.select_rows(np.arange(50) // 17 == k) for k in range(3)]
    for header in (True, False):
        _, a = written(tmp_path, whole, header, "whole.csv")
        p = str(tmp_path / "chunks.csv")
        n = ChunkedTable(parts).to_csv(p, header=header)
        assert open(p, "rb").read() == a and n == len(a)


def test_kept_dictionary_writes_what_its_decoded_column_writes(tmp_path):
    import pyarrow as pa
    arr = pa.array(["a,b", None, "x", "", "a,b", 'q"'], type=pa.string()).dictionary_encode()
    t = Table.from_arrow(pa.table({"k": arr, "n": pa.array([1, 2, 3, 4, 5, 6], type=pa.int32())}), dictionaries="keep")
    _, data = written(tmp_path, t)
    assert data == b'k,n\n"a,b",1\n,2\nx,3\n"",4\n"a,b",5\n"q""",6\n'


def test_decimal128_is_refused_by_name(tmp_path):
    t = Table.from_pydict({"ok": [1, 2], "wide": [Decimal("1.5"), None]}, types={"ok": "int", "wide": "decimal(38,10)"})
    with pytest.raises(ValueError, match="wide"):
        t.to_csv(str(tmp_path / "w.csv"))
