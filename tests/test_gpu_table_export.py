"""Table export from the device: to_host after to_device gives equal buffers for every column kind; a device table's
to_arrow() equals the host table's; a from_parquet(device=0) table written by to_parquet reads back equal; the failed
rows of a verification run are written with to_csv and read back. Bar: buffers and bytes, exactly."""
import copy

import numpy as np
import pytest

import deequ_amd as D
from deequ_amd.table import DictColumn, Table
import csv_export_cases as E
import csv_write_model as M

pytestmark = pytest.mark.gpu


def on_device(t):
    return Table([copy.copy(c) for c in t.columns.values()]).to_device(0)


@pytest.mark.parametrize("n", [0, 1, 70, 1000])
def test_to_host_after_to_device_gives_equal_buffers(n):
    t = E.every_kind_table(n)
    dev = on_device(t)
    back = dev.to_host()
    assert back is not dev and all(c.device is None for c in back.columns.values())
    E.assert_same_buffers(t, back)
    assert back["full"].validity is None  # a column without a bitmap stays without one


def test_to_host_of_a_device_only_table():
    import pyarrow as pa
    t = E.every_kind_table(300)
    dev = Table.from_arrow(t.to_arrow(), wide_decimals=True, dictionaries="keep", device=0)
    assert all(c.values is None for c in dev.columns.values() if not isinstance(c, DictColumn))
    E.assert_same_buffers(t, dev.to_host())


def test_to_arrow_of_a_device_table_equals_the_host_tables():
    t = E.every_kind_table(300)
    assert on_device(t).to_arrow().equals(t.to_arrow())
    E.assert_same_buffers(t, Table.from_arrow(on_device(t).to_arrow(), wide_decimals=True, dictionaries="keep"))


def test_to_parquet_of_a_device_table_reads_back_equal(tmp_path):
    t = E.every_kind_table(300)
    src, dst = str(tmp_path / "src.parquet"), str(tmp_path / "dst.parquet")
    t.to_parquet(src)
    dev = Table.from_parquet(src, wide_decimals=True, dictionaries="keep", device=0)
    dev.to_parquet(dst)
    back = Table.from_parquet(dst, wide_decimals=True, dictionaries="keep", device=0)
    E.assert_same_buffers(dev.to_host(), back.to_host(), null_slots=False)
    E.assert_same_buffers(t, back.to_host(), null_slots=False)


def test_failed_rows_of_a_verification_run_are_written_and_read_back(tmp_path):
    rng = np.random.default_rng(31)
    n = 500
    words = ["ok", "a,b", 'q"', "two\nlines", "é"]
    data = {"id": [int(x) for x in rng.permutation(n)],
            "word": [None if rng.random() < 0.2 else words[int(k)] for k in rng.integers(0, len(words), n)],
            "v": [None if rng.random() < 0.1 else float(x) / 8 for x in rng.integers(-50, 50, n)]}
    t = Table.from_pydict(data, types={"id": "long", "word": "string", "v": "double"}).to_device(0)
    check = D.Check(D.CheckLevel.Error, "A").isComplete("word").isNonNegative("v")
    result = D.VerificationSuite().onData(t).addChecks([check]).run()
    res = D.VerificationResult.rowLevelResultsAsTable(result, t)
    failed = res.failedRowsTable()
    bad = [i for i in range(n) if data["word"][i] is None or (data["v"][i] is not None and data["v"][i] < 0)]
    assert failed.nrows == len(bad) > 0 and all(c.device is not None for c in failed.columns.values())
    p = str(tmp_path / "quarantine.csv")
    failed.to_csv(p)
    want = Table.from_pydict({k: [v[i] for i in bad] for k, v in data.items()},
                             types={"id": "long", "word": "string", "v": "double"})
    assert open(p, "rb").read() == M.file_bytes(want)
    back = Table.from_csv(p, device=0).to_host()
    assert dict(back.schema) == {"id": "IntegerType", "word": "StringType", "v": "DoubleType"}
    assert back["id"].to_pylist() == [data["id"][i] for i in bad]
    assert back["word"].to_pylist() == [data["word"][i] for i in bad]
    assert back["v"].to_pylist() == [data["v"][i] for i in bad]
