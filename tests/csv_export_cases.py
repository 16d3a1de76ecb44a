"""The table of every column kind for the export tests (test_table_export.py, test_gpu_table_export.py) and the
buffer-for-buffer comparison they share."""
from decimal import Decimal

import numpy as np

from deequ_amd import native as N
from deequ_amd.table import DictColumn, Table, unpack_validity


def every_kind_table(n=70, seed=21):
    """Every column kind a Table holds, as `from_arrow(..., wide_decimals=True, dictionaries="keep")` lays them out:
    the fixed-width types, DECIMAL and DECIMAL128, DATE, TIMESTAMP, a STRING column, a kept dictionary; with NULLs
    (whose slots hold zero, as ingest leaves them) and, last, a column without NULLs and without a bitmap."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)

    def nulls(v):
        return [None if rng.random() < 0.2 else x for x in v]

    words = ["", "a", "a,b", "é", "long " * 9, 'q"']
    data = {
        "flag": pa.array(nulls([bool(x) for x in rng.random(n) < 0.5]), type=pa.bool_()),
        "b": pa.array(nulls([int(x) for x in rng.integers(-128, 128, n)]), type=pa.int8()),
        "s": pa.array(nulls([int(x) for x in rng.integers(-2 ** 15, 2 ** 15, n)]), type=pa.int16()),
        "i": pa.array(nulls([int(x) for x in rng.integers(-2 ** 31, 2 ** 31, n)]), type=pa.int32()),
        "l": pa.array(nulls([int(x) for x in rng.integers(-2 ** 62, 2 ** 62, n)]), type=pa.int64()),
        "f": pa.array(nulls([float(np.float32(x)) for x in rng.normal(0, 10, n)]), type=pa.float32()),
        "d": pa.array(nulls([float(x) for x in rng.normal(0, 10, n)]), type=pa.float64()),
        "dec": pa.array(nulls([Decimal(int(x)).scaleb(-4) for x in rng.integers(-10 ** 12, 10 ** 12, n)]),
                        type=pa.decimal128(16, 4)),
        "wide": pa.array(nulls([Decimal(int(x) * 10 ** 15 + 7).scaleb(-10) for x in rng.integers(-10 ** 15, 10 ** 15, n)]),
                         type=pa.decimal128(38, 10)),
        "day": pa.array(nulls([int(x) for x in rng.integers(-200000, 200000, n)]), type=pa.int32()).cast(pa.date32()),
        "ts": pa.array(nulls([int(x) for x in rng.integers(-10 ** 15, 10 ** 15, n)]), type=pa.int64()).cast(pa.timestamp("us")),
        "text": pa.array(nulls([words[int(k)] for k in rng.integers(0, len(words), n)]), type=pa.string()),
        "key": pa.array(nulls([words[int(k)] for k in rng.integers(0, len(words), n)]), type=pa.string()).dictionary_encode(),
        "full": pa.array([int(x) for x in rng.integers(0, 100, n)], type=pa.int64()),
    }
    t = Table.from_arrow(pa.table(data), wide_decimals=True, dictionaries="keep")
    assert isinstance(t["key"], DictColumn) and t["wide"].spark_type == N.TYPE_DECIMAL128
    assert t["full"].validity is None
    assert n < 50 or all(t[c].validity is not None for c in t.fieldNames if c != "full")
    return t


def same_bytes(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def assert_same_buffers(t, back, null_slots=True):
    """`back` has the names, types and buffers of `t`: values, validity words, offsets, dictionary indices, entries.
    null_slots=False compares a fixed-width column's values at its non-NULL rows only: a parquet file does not store
    the slot of a NULL cell, so what pyarrow's reader leaves there is its own."""
    assert back.fieldNames == t.fieldNames and back.nrows == t.nrows
    assert dict(back.schema) == dict(t.schema)
    for name in t.fieldNames:
        a, b = t[name], back[name]
        if not null_slots and isinstance(b, DictColumn) and not isinstance(a, DictColumn):
            b = b.decoded()  # from_parquet(dictionaries="keep") reads every string column dictionary-encoded
        assert type(a) is type(b), name
        assert same_bytes(a.validity, b.validity), name
        if isinstance(a, DictColumn):
            assert same_bytes(a.indices, b.indices), name
            a, b = a.dictionary, b.dictionary
            assert same_bytes(a.validity, b.validity), name
        if a.spark_type == N.TYPE_STRING:
            n = a.length
            assert same_bytes(np.asarray(a.offsets)[:n + 1], np.asarray(b.offsets)[:n + 1]), name
            end = int(a.offsets[n]) if n else 0
            assert same_bytes(np.asarray(a.values)[:end], np.asarray(b.values)[:end]), name
        elif null_slots or a.validity is None:
            assert same_bytes(a.values, b.values), name
        else:
            keep = unpack_validity(a.validity, a.length)
            assert same_bytes(np.asarray(a.values)[keep], np.asarray(b.values)[keep]), name
        assert (a.decimal_precision, a.decimal_scale) == (b.decimal_precision, b.decimal_scale), name
