"""The CSV writer's per-cell code built for the host (deequ_amd/csrc/dq_csv_cell.h with -DDQ_HOST_ONLY: the code the
kernels of csv_write.hip call, no HIP) as a stand-alone program under ASan / UBSan, against the model of
tests/csv_write_model.py. No GPU. It pins, on the host, the four format_* functions that moved from rx_engine.h into
dq_format.h (long, decimal, date, timestamp at their edges), the typed-cell switch, the quoting decision, the quoted
length and the quoted copy. Bar: text, exactly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from deequ_amd import native as N
from deequ_amd.table import Column
import csv_write_cases as W
import csv_write_model as M
import number_text_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("csv_write_host") / "csv_write_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-DDQ_HOST_ONLY", "-Wall", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "deequ_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "csv_write_host", "main.cpp")], check=True)

    def run(lines):
        p = subprocess.run([exe], input="".join(s + "\n" for s in lines), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        out = p.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def typed(host_tool, spark_type, values, scale=0):
    """(the tool's texts, the model's texts) of a column of `values`."""
    col = Column("c", spark_type, np.asarray(values), decimal_precision=18 if scale else 0, decimal_scale=scale)
    width = col.values.dtype.itemsize
    raw = np.ascontiguousarray(col.values).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width])
    got = host_tool(["T %d %d %x" % (col.spark_type, scale, int(u)) for u in raw])
    return got, [M.cell_text(col, i).decode() for i in range(col.length)]


def test_doubles_and_floats_of_the_number_text_cases(host_tool):
    doubles, floats = C.format_cases(103)
    sp = C.format_special_values()
    got, want = typed(host_tool, "double", np.concatenate([doubles, np.array(sp, np.float64)]))
    assert got == want and len(got) >= 6000
    got, want = typed(host_tool, "float", np.concatenate([floats, np.array(sp, np.float32)]))
    assert got == want and len(got) >= 6000


def test_integral_edges(host_tool):
    for t, dtype in (("byte", np.int8), ("short", np.int16), ("int", np.int32), ("long", np.int64)):
        info = np.iinfo(dtype)
        vals = np.array([info.min, info.min + 1, -10, -1, 0, 1, 9, 10, 99, 100, info.max - 1, info.max], dtype=dtype)
        got, want = typed(host_tool, t, vals)
        assert got == want, t
    got, _ = typed(host_tool, "long", np.array([-2 ** 63], np.int64))
    assert got == ["-9223372036854775808"]  # Long.MIN_VALUE
    got, want = typed(host_tool, "boolean", np.array([0, 1, 2, 255], np.uint8))
    assert got == want == ["false", "true", "true", "true"]


def test_decimal_edges(host_tool):
    vals = np.array([0, 1, -1, 9, 10, -15, 123456789, 10 ** 18 - 1, -(10 ** 18 - 1), 10 ** 17, 1000000, 999999, -1000001],
                    np.int64)
    for scale in (0, 1, 6, 7, 8, 17, 18):
        got, want = typed(host_tool, "decimal", vals, scale)
        assert got == want, scale
    assert typed(host_tool, "decimal", np.array([1, 10], np.int64), 8)[0] == ["1E-8", "1.0E-7"]
    assert typed(host_tool, "decimal", np.array([1], np.int64), 7)[0] == ["1E-7"]


def test_date_edges(host_tool):
    # both sides of the 1582 cutover, the first Julian day and the day before it (1 BC prints as year 1), leap days on
    # both calendars, years past 9999, the int32 ends
    days = [-141429, -141428, -141427, -141426, -719164, -719165, -719529, -1, 0, 59, 60, 11016, 2932896, 2932897,
            3000000, -2 ** 31, 2 ** 31 - 1, -171000, -170999, -499999, 500000]
    got, want = typed(host_tool, "date", np.array(days, np.int32))
    assert got == want
    assert got[1:3] == ["1582-10-04", "1582-10-15"] and got[13] == "10000-01-01"
    rng = np.random.default_rng(3)
    got, want = typed(host_tool, "date", rng.integers(-2 ** 31, 2 ** 31, 3000).astype(np.int32))
    assert got == want


def test_timestamp_edges(host_tool):
    us = [0, 1, -1, 999999, 1000000, -1000000, -999999, 1500000, 100000, 120000, 86399999999, 86400000000, -86400000001,
          253402300799999999, 253402300800000000, -62135596800000000, -62135596800000001, -12219292800000000,
          -12219292800000001, 10 ** 17, -10 ** 17]
    got, want = typed(host_tool, "timestamp", np.array(us, np.int64))
    assert got == want
    assert got[1] == "1970-01-01 00:00:00.000001" and got[2] == "1969-12-31 23:59:59.999999"  # negative micros floor
    rng = np.random.default_rng(4)
    got, want = typed(host_tool, "timestamp", rng.integers(-2 ** 58, 2 ** 58, 3000))
    assert got == want


def test_string_cells(host_tool):
    cells = [s.encode("utf-8") for s in W.STRING_POOL] + W.reader_alphabet_cells(500, seed=13)
    cells += [b'"' * 4096, b"\xff\xfe,\x00", b"\x00", b"," * 65, b"a" * 4095 + b"\r"]
    out = host_tool(["S " + (c.hex() or "-") for c in cells])
    for c, line in zip(cells, out):
        quoted, quotes, length, text = (line.split(" ") + [""])[:4]
        want = M.quoted(c)
        assert bytes.fromhex(text) == want, c
        assert int(length) == len(want) and int(quotes) == c.count(b'"')
        assert (quoted == "1") == (want != c or c == b"")
