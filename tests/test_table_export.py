"""Table.to_arrow / to_parquet / to_host of host tables: every column kind round-trips through from_arrow /
from_parquet with equal buffers (DECIMAL128, DATE, TIMESTAMP, a kept dictionary, a column without NULLs). No GPU."""
import numpy as np

from deequ_amd.table import ChunkedTable, Table
import csv_export_cases as E


def test_to_arrow_round_trips_every_column_kind():
    import pyarrow as pa
    t = E.every_kind_table()
    at = t.to_arrow()
    assert isinstance(at, pa.Table) and at.column_names == t.fieldNames and at.num_rows == t.nrows
    assert pa.types.is_dictionary(at.schema.field("key").type) and at.schema.field("wide").type == pa.decimal128(38, 10)
    assert at.schema.field("day").type == pa.date32() and at.schema.field("ts").type == pa.timestamp("us")
    assert at["full"].null_count == 0
    E.assert_same_buffers(t, Table.from_arrow(at, wide_decimals=True, dictionaries="keep"))


def test_to_arrow_of_zero_rows_and_one_row():
    for n in (0, 1):
        t = E.every_kind_table(n)
        E.assert_same_buffers(t, Table.from_arrow(t.to_arrow(), wide_decimals=True, dictionaries="keep"))


def test_to_parquet_round_trips_every_column_kind(tmp_path):
    t = E.every_kind_table()
    p = str(tmp_path / "t.parquet")
    t.to_parquet(p)
    E.assert_same_buffers(t, Table.from_parquet(p, wide_decimals=True, dictionaries="keep"), null_slots=False)


def test_timestamp_zone_survives():
    import pyarrow as pa
    at = pa.table({"ts": pa.array([1, None, 3], type=pa.timestamp("us", tz="Europe/Berlin"))})
    t = Table.from_arrow(at)
    assert t.to_arrow().schema.field("ts").type == pa.timestamp("us", tz="Europe/Berlin")
    assert Table.from_arrow(t.to_arrow())["ts"].tz == "Europe/Berlin"


def test_a_host_table_is_its_own_host_table():
    t = E.every_kind_table(5)
    assert t.to_host() is t


def test_chunked_to_arrow_concatenates_the_chunks():
    t = E.every_kind_table(60)
    at = t.to_arrow()
    chunks = ChunkedTable([Table.from_arrow(at.slice(a, 20), wide_decimals=True, dictionaries="keep") for a in (0, 20, 40)])
    got = chunks.to_arrow()
    assert got.num_rows == 60 and got.column_names == t.fieldNames
    for name in t.fieldNames:
        assert got[name].to_pylist() == at[name].to_pylist(), name
