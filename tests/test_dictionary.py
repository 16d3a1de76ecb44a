"""Arrow dictionary-encoded string columns held encoded (`dictionaries="keep"`, table.DictColumn): ingest semantics on
the host. The kept column must read exactly as Arrow's own decode of the same array reads."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

from deequ_amd.table import Column, DictColumn, Table


def kept(arr, **kw):
    return Table.from_arrow(pa.table({"c": arr}), dictionaries="keep", **kw)["c"]


def test_null_entries_fold_into_the_validity_bitmap():
    arr = pa.DictionaryArray.from_arrays(pa.array([0, 1, 2, 3, 4, None, 0, 3], type=pa.int32()),
                                         pa.array(["a", "bb", None, "a", "", "zzz"]))
    assert arr.null_count == 1  # Arrow counts the NULL index only; the row that points at the NULL entry is NULL too
    col = kept(arr)
    assert isinstance(col, DictColumn)
    assert col.type_name == "StringType" and col.indices.dtype == np.int32
    assert col.to_pylist() == arr.dictionary_decode().to_pylist() == ["a", "bb", None, "a", "", None, "a", "a"]
    assert int(col.null_mask().sum()) == 2
    assert col.n_dict == 6  # duplicates, the unused entry and the NULL entry stay: nothing is deduplicated
    assert col.decoded().to_pylist() == col.to_pylist()
    assert col.decoded() is col.decoded()  # cached


def test_default_keyword_still_decodes():
    arr = pa.array(["x", None, "y", "x"]).dictionary_encode()
    col = Table.from_arrow(pa.table({"c": arr}))["c"]
    assert type(col) is Column and col.to_pylist() == ["x", None, "y", "x"]
    assert type(Table.from_arrow(pa.table({"c": arr}), dictionaries="decode")["c"]) is Column
    with pytest.raises(ValueError):
        Table.from_arrow(pa.table({"c": arr}), dictionaries="maybe")


def test_sliced_arrays():
    arr = pa.array(["a", "b", None, "c", "a", "ddd", None, "b"] * 5).dictionary_encode()
    for off, n in [(0, 40), (3, 17), (9, 1), (7, 0), (39, 1)]:
        s = arr.slice(off, n)
        assert kept(s).to_pylist() == s.dictionary_decode().to_pylist()


@pytest.mark.parametrize("index_type", [pa.uint8(), pa.int8(), pa.int16(), pa.uint16(), pa.uint32(), pa.int64()])
def test_narrow_and_unsigned_indices_are_widened(index_type):
    arr = pa.DictionaryArray.from_arrays(pa.array([2, 0, None, 1, 2], type=index_type), pa.array(["é", "", "zz"]))
    col = kept(arr)
    assert col.indices.dtype == np.int32
    assert col.to_pylist() == ["zz", "é", None, "", "zz"]


def test_large_string_dictionaries_are_kept_and_other_value_types_decode():
    arr = pa.DictionaryArray.from_arrays(pa.array([1, 0], type=pa.int32()), pa.array(["p", "q"], type=pa.large_string()))
    assert isinstance(kept(arr), DictColumn) and kept(arr).to_pylist() == ["q", "p"]
    ints = pa.DictionaryArray.from_arrays(pa.array([1, 0, 1], type=pa.int32()), pa.array([10, 20], type=pa.int64()))
    col = kept(ints)
    assert type(col) is Column and col.to_pylist() == [20, 10, 20]


def test_chunks_with_different_dictionaries_are_unified():
    a = pa.DictionaryArray.from_arrays(pa.array([0, 1, None], type=pa.int32()), pa.array(["x", "y"]))
    b = pa.DictionaryArray.from_arrays(pa.array([1, 0, 0], type=pa.int32()), pa.array(["y", "z"]))
    chunked = pa.chunked_array([a, b])
    col = Table.from_arrow(pa.table({"c": chunked}), dictionaries="keep")["c"]
    assert isinstance(col, DictColumn)
    assert col.to_pylist() == ["x", "y", None, "z", "y", "y"]


def test_out_of_range_index_raises():
    for bad in (3, -1):
        arr = pa.DictionaryArray.from_arrays(pa.array([0, bad, 1], type=pa.int32()), pa.array(["a", "b", "c"]), safe=False)
        with pytest.raises(ValueError, match="outside"):
            kept(arr)
    # the index under a NULL row is never looked at
    ind = pa.Array.from_buffers(pa.int32(), 3, [pa.py_buffer(bytes([0b101])),
                                                pa.py_buffer(np.array([0, 99, 1], dtype=np.int32).tobytes())])
    arr = pa.DictionaryArray.from_arrays(ind, pa.array(["a", "b"]), safe=False)
    assert kept(arr).to_pylist() == ["a", None, "b"]


def test_to_arrow_round_trips_as_a_dictionary_array():
    arr = pa.DictionaryArray.from_arrays(pa.array([0, 1, 2, None, 1], type=pa.int32()), pa.array(["a", None, "a"]))
    col = kept(arr)
    back = col.to_arrow()
    assert pa.types.is_dictionary(back.type)
    assert back.dictionary_decode().to_pylist() == arr.dictionary_decode().to_pylist() == ["a", None, "a", None, None]
    assert kept(back).to_pylist() == col.to_pylist()


def test_empty_and_all_null_columns():
    empty = pa.DictionaryArray.from_arrays(pa.array([], type=pa.int32()), pa.array([], type=pa.string()))
    assert kept(empty).to_pylist() == [] and kept(empty).decoded().length == 0
    nulls = pa.DictionaryArray.from_arrays(pa.array([None, None], type=pa.int32()), pa.array([], type=pa.string()))
    col = kept(nulls)
    assert col.to_pylist() == [None, None] and col.decoded().to_pylist() == [None, None]


def test_parquet_round_trip(tmp_path):
    import pyarrow.parquet as pq
    vals = [None if i % 7 == 0 else "cat_%d" % (i % 5) for i in range(200)]
    path = str(tmp_path / "t.parquet")
    pq.write_table(pa.table({"cat": pa.array(vals), "n": pa.array(range(200), type=pa.int64())}), path)
    t = Table.from_parquet(path, dictionaries="keep")
    assert isinstance(t["cat"], DictColumn) and type(t["n"]) is Column
    assert t["cat"].to_pylist() == vals and t["n"].to_pylist() == list(range(200))
    plain = Table.from_parquet(path)
    assert type(plain["cat"]) is Column and plain["cat"].to_pylist() == vals
    assert t.schema == plain.schema
    only = Table.from_parquet(path, columns=["cat"], dictionaries="keep")
    assert only.fieldNames == ["cat"] and only["cat"].to_pylist() == vals


def test_kept_column_reads_as_a_plain_string_column():
    """Consumers that do not know the class read `values` / `offsets` / `native()`: those of the decoded column."""
    arr = pa.array(["ab", None, "", "ab", "çé"]).dictionary_encode()
    col, plain = kept(arr), Table.from_arrow(pa.table({"c": arr}))["c"]
    assert bytes(col.values) == bytes(plain.values)
    assert list(col.offsets) == list(plain.offsets)
    assert col.device is None and col.native().length == 5
    t = Table.from_arrow(pa.table({"c": arr}), dictionaries="keep")
    assert t.select_rows([True, True, False, False, True])["c"].to_pylist() == ["ab", None, "çé"]
