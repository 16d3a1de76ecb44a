"""Table.from_csv(path, device=0): the file's bytes tokenized, typed and parsed on the GPU (csv.hip) give the table the
host path gives -- names, Spark types, validity bits and cells, doubles by bit pattern, buffers laid out as
Table.to_device lays them out -- or the refusal csv_model.py predicts. Every comparison is exact."""
import csv
import io
import os
import random
import re

import numpy as np
import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import engine
from deequ_amd.table import Table, pack_validity, unpack_validity

import csv_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = N.CSV_TILE_BYTES


def assert_same(host, dev):
    """The device table against the host table: schema, then every buffer against what to_device would upload."""
    assert list(dev.schema.items()) == list(host.schema.items())
    assert dev.nrows == host.nrows
    for name, h in host.columns.items():
        d = dev[name]
        assert d.length == h.length == host.nrows and d.values is None and d.device is not None, name
        n = h.length
        if h.validity is None:
            assert d.device.get("validity") is None, name
        else:
            want = pack_validity(unpack_validity(h.validity, n))
            assert d.device["validity"].cpu().numpy().tobytes() == want.tobytes(), name  # zero at and past nrows
        if h.spark_type == N.TYPE_STRING:
            offs = d.device["offsets"].cpu().numpy()
            assert offs.dtype == np.int32 and offs.tobytes() == np.asarray(h.offsets, np.int32).tobytes(), name
            data = d.device["values"].cpu().numpy()
            assert d.device["values"].data_ptr() % 4 == 0 and len(data) >= int(offs[-1]) + 16, name
            assert data[:int(offs[-1])].tobytes() == np.asarray(h.values, np.uint8).tobytes(), name
            assert not data[int(offs[-1]):int(offs[-1]) + 16].any(), name
        else:
            got = d.device["values"].cpu().numpy().tobytes()
            assert got == np.ascontiguousarray(h.values).tobytes(), (name, h.type_name)  # doubles bit for bit


def both(tmp_path, data, name="t.csv", **kw):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data if isinstance(data, bytes) else data.encode("utf-8"))
    host = Table.from_csv(p, **kw)
    dev = Table.from_csv(p, device=0, **kw)
    assert_same(host, dev)
    return host, dev


def refused(tmp_path, data, name="r.csv", **kw):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    with pytest.raises(ValueError) as e:
        Table.from_csv(p, device=0, **kw)
    return str(e.value)


def assert_refusal(tmp_path, data):
    kind, offset = M.refusal(data)
    msg = refused(tmp_path, data)
    assert N.CSV_REFUSALS[kind] in msg and re.search(r"at byte %d\b" % offset, msg), (msg, kind, offset)


# ---- titanic --------------------------------------------------------------------------------------------------------
def test_titanic_table_and_metrics_equal_the_host():
    p = os.path.join(ROOT, "tests", "golden", "titanic.csv")
    host = Table.from_csv(p)
    dev = Table.from_csv(p, device=0)
    assert_same(host, dev)
    analyzers = [D.Size(), D.Completeness("Age"), D.Mean("Fare"), D.Uniqueness(["PassengerId"]), D.MaxLength("Name"),
                 D.DataType("Cabin")]

    def metrics(t):
        ctx = D.AnalysisRunner.onData(t).addAnalyzers(analyzers).run()
        return [ctx.metric(a).value.get() for a in analyzers]

    assert repr(metrics(dev)) == repr(metrics(host))


# ---- types ----------------------------------------------------------------------------------------------------------
def test_every_type_and_its_edges(tmp_path):
    cols = {
        "i": ["2147483647", "-2147483648", "+5", "-0", "00012", ""],
        "l": ["2147483648", "-2147483649", "9223372036854775807", "-9223372036854775808", "7", ""],
        "big": ["9223372036854775808", "-9223372036854775809", "1", "", "99999999999999999999", "-3"],
        "d": ["1.", ".5", "1.e3", "-.5e-3", "1e400", "-0.0"],
        "lit": ["NaN", "Infinity", "-Infinity", "", "0e0", "-1e-400"],
        "b": ["tRuE", "false", "", "TRUE", "False", "true"],
        "il": ["1", "3000000000", "", "-1", "2", "3"],
        "ld": ["3000000000", "1.5", "2", "", "-0", "1e3"],
        "bi": ["true", "1", "", "false", "2", "0"],
        "bs": ["true", "x", "false", "", "y", "z"],
        "empty": ["", "", "", "", "", ""],
        "s": ["nan", "inf", "+Infinity", "1.5d", "1_0", "0x10"],
        "sp": [" 1", "1 ", "a", "", "1..2", "--1"],
    }
    names = list(cols)
    lines = [",".join(names)] + [",".join(cols[c][r] for c in names) for r in range(6)]
    host, dev = both(tmp_path, "\n".join(lines) + "\n")
    want = {"i": "IntegerType", "l": "LongType", "big": "DoubleType", "d": "DoubleType", "lit": "DoubleType",
            "b": "BooleanType", "il": "LongType", "ld": "DoubleType", "bi": "StringType", "bs": "StringType",
            "empty": "StringType", "s": "StringType", "sp": "StringType"}
    assert dict(dev.schema) == want
    d = dev["d"].device["values"].cpu().numpy().view(np.float64)
    assert np.isposinf(d[4]) and np.signbit(d[5]) and d[5] == 0.0
    lit = dev["lit"].device["values"].cpu().numpy().view(np.uint64)
    assert lit[0] == 0x7FF8000000000000 and lit[5] == 0x8000000000000000
    both(tmp_path, "\n".join(lines) + "\n", infer_schema=False)
    both(tmp_path, "\n".join(lines[1:]) + "\n", header=False)
    h, _ = both(tmp_path, "\n".join(lines[1:]) + "\n", header=False, infer_schema=False)
    assert list(h.schema)[:2] == ["_c0", "_c1"]


def test_quoted_numbers_and_many_rows(tmp_path):
    rng = random.Random(5)
    rows = ["a,b,c,d"]
    for r in range(3000):  # more than one workgroup of rows, validity words that end inside a word
        rows.append('%s,"%s",%s,%s' % (rng.choice(["", str(rng.randint(-10 ** 9, 10 ** 9))]),
                                        rng.choice(["", repr(rng.uniform(-1e6, 1e6)), "%de%d" % (rng.randint(1, 99), rng.randint(-320, 310))]),
                                        rng.choice(["true", "FALSE", ""]), rng.choice(["", "x", '"q,""r"""', "é"])))
    host, dev = both(tmp_path, "\n".join(rows) + "\n")
    assert dict(dev.schema) == {"a": "IntegerType", "b": "DoubleType", "c": "BooleanType", "d": "StringType"}
    assert dev["a"].device.get("validity") is not None


def test_undecidable_rounding_fails_the_call(tmp_path):
    # 2^53 + 1 is halfway between two doubles; the digits past the 19th decide the rounding, and the device parser
    # keeps 19: it fails the call (DQ_ERR_UNSUPPORTED) and does not guess
    p = str(tmp_path / "slow.csv")
    with open(p, "wb") as f:
        f.write(b"x\n1.5\n9007199254740993.0000000001\n")
    with pytest.raises(N.NativeError) as e:
        Table.from_csv(p, device=0)
    assert e.value.status == -2 and "dq_csv_column" in str(e.value)
    both(tmp_path, b"x\n1.5\n9007199254740993.0000000001\n", infer_schema=False)
    both(tmp_path, b"x\n1.5\n9007199254740993\n9007199254740992.99999\n123456789012345678901234567890\n")


# ---- shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", [
    b"a,b\r\n1,2\r\n3,4\r\n",
    b"a,b\n1,2\n3,4",
    b"a,b\n1,2\n\n3,4\n\n\n",
    b"a,b\r\n\r\n1,2\r\n\r\n",
    b"a,b,c\n1\n1,2\n1,2,3\n1,2,3,4\n1,2,3,4,5,6\n,\n,,\n,,,\n",
    b'a,b\n"",x\ny,""\n"",""\n',
    b'a,b\n"p,q",1\n"r\ns",2\n"t\r\nu",3\n"v\rw",4\n"""",5\n"a""b""",6\n',
    b"a\n1\n2\n\n3\n",
    b"a\n",
    b"a",
    b"a,b,c",
    b"a,b\n",
    b'"a,1","b\n2"\n1,2\n',
    b"\xef\xbb\xbfid,v\n1,2\n",
])
def test_record_and_field_shapes(tmp_path, data):
    assert M.refusal(data) is None
    both(tmp_path, data)
    both(tmp_path, data, header=False)
    both(tmp_path, data, infer_schema=False)


def test_seventy_columns_and_one_column(tmp_path):
    rng = random.Random(9)
    names = ["c%d" % i for i in range(70)]
    rows = [",".join(names)]
    for r in range(200):
        k = rng.choice([70, 70, 70, 3, 0, 75])
        rows.append(",".join(rng.choice(["", "1", "2.5", "true", "x", '"a,b"']) if (i % 7) else str(r * i) for i in range(k)))
    host, dev = both(tmp_path, "\n".join(rows) + "\n")
    assert len(dev.columns) == 70 and dev.nrows == 200
    both(tmp_path, "\n".join(r.split(",")[0] for r in rows) + "\n")


def test_more_columns_than_a_workgroup_accumulates_in_lds(tmp_path):
    ncols = 4096 + 37  # csv.hip keeps the per-column classes and counts of the first 4096 columns in LDS
    rows = [",".join("c%d" % i for i in range(ncols))]
    for r in range(70):
        rows.append(",".join(("" if (i + r) % 5 == 0 else str(i * r) if i % 3 else "x%d" % r) for i in range(ncols - r % 3)))
    host, dev = both(tmp_path, "\n".join(rows) + "\n")
    assert len(dev.columns) == ncols and dev.schema["c4100"] == "IntegerType" and dev.schema["c4098"] == "StringType"


def test_header_without_fields_is_refused(tmp_path):
    assert "no fields" in refused(tmp_path, b"\n1,2\n")
    assert "no fields" in refused(tmp_path, b"\r\n1,2\n", header=False)
    assert "empty file" in refused(tmp_path, b"")


# ---- boundaries -----------------------------------------------------------------------------------------------------
PATTERNS = {  # name: (bytes of the record before the anchor, the anchor and the rest of the record)
    "escape_pair": (b'"ab', b'""cd",z,w\n'),
    "empty_quoted": (b"k,", b'"",z,w\n'),
    "crlf": (b"k,l,m", b"\r\n"),
    "closing_quote_comma": (b'"q', b'",z,w\n'),
    "opening_quote": (b"k,", b'"op,""en",w\n'),
}


def boundary_file(pattern, off):
    """A file whose `pattern` anchor starts at byte `off`: a header, then one record led by an unquoted field as long
    as it takes, then records that show the state after the anchor."""
    lead, rest = PATTERNS[pattern]
    head = b"a,b,c,d\n"
    pad = off - len(lead) - 1 - len(head)
    assert pad >= 0
    data = head + b"x" * pad + b"," + lead + rest + b'5,"s,t",,7.5\n"u""",,true\n'
    assert data[off:off + len(rest)] == rest
    return data


@pytest.mark.parametrize("bound", [64, 4096, TILE, 2 * TILE])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_patterns_across_word_and_tile_boundaries(tmp_path, pattern, bound):
    for off in range(bound - 3, bound + 2):
        data = boundary_file(pattern, off)
        assert M.refusal(data) is None
        host, dev = both(tmp_path, data, name="b%d.csv" % off)
        assert dev.nrows == 3


def test_long_fields_records_and_exact_tile_sizes(tmp_path):
    long_quoted = b'"' + (b'ab,"",\n' * (2 * TILE // 7 + 10)) + b'"'
    assert len(long_quoted) > 2 * TILE
    both(tmp_path, b"a,b\n1," + long_quoted + b"\n2,y\n")
    long_record = b",".join(b"%d" % i for i in range(TILE // 4))
    assert len(long_record) > TILE
    both(tmp_path, b"a,b,c\n" + long_record + b"\n1,2,3\n")
    for size in (TILE - 1, TILE, TILE + 1):
        for tail in (b"7,yyyyyyyyyy\n", b"7,yyyyyyyyyy", b'7,"yyyyyyyy"\n', b'7,"yyyyyyyyy"', b"7,\r\n", b"\n\n"):
            fill = size - 4 - len(tail)
            small = b"12,x\n" * ((fill - 3) // 5 - 1)
            data = b"a,b\n" + small + b"9," + b"z" * (fill - len(small) - 3) + b"\n" + tail
            assert len(data) == size
            both(tmp_path, data)
    blanks = b"a,b\n1,2\n" + b"\n" * (TILE + 100) + b"3,4\n" + b"\r\n" * 70 + b"5,6"
    host, dev = both(tmp_path, blanks)
    assert dev.nrows == TILE + 100 + 70 + 3


# ---- non-ASCII ------------------------------------------------------------------------------------------------------
def test_non_ascii_text(tmp_path):
    host, dev = both(tmp_path, "n,t\n1,é\n2,日本語\n3,\n4,ü\n")
    assert dev.schema["t"] == "StringType"
    # multibyte characters astride the 64-byte words and a tile
    for pad in range(58, 66):
        both(tmp_path, "n,t\n" + "x" * pad + ",日本語é\n" + "ü" * 40 + ',"é,""ü"\n')
    both(tmp_path, "n,t\n" + "x" * (TILE - 7) + ",日本語é\n1,ü\n")
    # digits that Python's \d accepts and the device does not parse: refused, naming the column
    msg = refused(tmp_path, "n,count\n1,١٢\n2,\n3,٣\n".encode("utf-8"))
    assert "'count'" in msg and "infer_schema=False" in msg
    both(tmp_path, "n,count\n1,١٢\n2,\n3,٣\n", infer_schema=False)
    both(tmp_path, "n,count\n1,١٢\n2,x\n3,٣\n")  # a definite string decides the column
    msg = refused(tmp_path, b'n,v\n1,"12\n"\n')  # $ matches before a trailing line feed
    assert "'v'" in msg
    both(tmp_path, b'n,v\n1,"ab\n"\n')


# ---- refusals -------------------------------------------------------------------------------------------------------
BAD = {
    M.QUOTE_IN_FIELD: (b'k"', b"m\n"),  # (up to and including the offending byte, the rest)
    M.TEXT_AFTER_QUOTE: (b'"q"', b"m\n"),
    M.LONE_CR: (b"k\r", b"m\n"),
    M.UNTERMINATED_QUOTE: (b'"', b"m\n"),
}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_each_refusal_kind_and_its_offset(tmp_path, kind):
    upto, rest = BAD[kind]
    head = b"a,b\n"
    at = len(upto) - 1  # the offending byte inside `upto`
    for where in (None, TILE - 1, TILE):
        pad = b"" if where is None else b"x" * (where - len(head) - 1 - at) + b","
        data = head + pad + upto + rest
        assert M.refusal(data) == (kind, len(head) + len(pad) + at)
        if where is not None:
            assert M.refusal(data)[1] == where
        assert_refusal(tmp_path, data)


def test_the_earlier_of_two_anomalies_is_reported(tmp_path):
    for data in (b'a,b\n1\r2,x"y\n', b'a,b\nx"y,1\r2\n', b'a,b\n"q"z,"\n', b'a,"b\n' + b"x" * TILE + b'"\r"', b'a"',
                 b'a,b\n' + b"x" * (TILE - 6) + b'\rz,"q"z\n'):
        assert M.refusal(data) is not None
        assert_refusal(tmp_path, data)


# ---- random differential --------------------------------------------------------------------------------------------
def test_random_well_formed_files(tmp_path):
    rng = random.Random(11)
    cells = ["", "", "1", "-7", "2147483648", "1.5", ".5e3", "NaN", "true", "False", "x", "a,b", 'q"r', "l1\nl2", "c\rd",
             "é", " 1", "0x10", "12345678901234567890", '"', ",", "\r\n"]
    for k in range(2000):
        ncols = rng.randint(1, 6)
        buf = io.StringIO(newline="")
        term = rng.choice(["\n", "\r\n"])
        w = csv.writer(buf, lineterminator=term)
        pool = cells if term == "\r\n" else [c for c in cells if c != "c\rd"]  # the writer quotes a CR only when it ends lines
        w.writerow(["h%d" % i for i in range(ncols)])
        for r in range(rng.randint(0, 12)):
            row = [rng.choice(pool) for _ in range(rng.randint(1, ncols + 1))]
            if row == [""]:
                row = ["", ""]  # csv.writer writes a lone empty field as "": kept, but two are the plainer case
            w.writerow(row)
        data = buf.getvalue().encode("utf-8")
        assert M.refusal(data) is None, data
        both(tmp_path, data, infer_schema=bool(k % 5))


def test_random_raw_files_are_refused_or_equal(tmp_path):
    accepted = 0
    files = list(M.random_files(5000))
    for data in files:
        bad = M.refusal(data)
        if bad is not None:
            assert_refusal(tmp_path, data)
            continue
        accepted += 1
        if data == b"":
            assert "empty file" in refused(tmp_path, data)
        elif M.records(data)[0] == []:
            assert "no fields" in refused(tmp_path, data)
        else:
            try:
                both(tmp_path, data)
            except ValueError as e:  # a column of ambiguous fields the host reads as numbers: named, not guessed
                assert "infer_schema=False" in str(e), data
                both(tmp_path, data, infer_schema=False)
    assert accepted * 4 >= len(files), accepted


# ---- launches -------------------------------------------------------------------------------------------------------
def test_launch_counts_do_not_depend_on_the_rows(tmp_path):
    def launches(rows):
        p = str(tmp_path / ("l%d.csv" % rows))
        with open(p, "w", newline="") as f:
            f.write("i,d,s,b\n" + "".join('%d,%d.5,"s,%d",true\n' % (r, r, r) for r in range(rows)))
        before = engine.ctx().csv_kernel_launches()
        t = Table.from_csv(p, device=0)
        after = engine.ctx().csv_kernel_launches()
        assert t.nrows == rows
        return {k: after[k] - before[k] for k in after}

    small, large = launches(10), launches(10_000)
    assert small == large == {"csv_quotes": 1, "csv_mark": 1, "csv_rows": 1, "csv_fields": 1, "csv_column": 5}
