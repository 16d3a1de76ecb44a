"""Table.from_arrow(t, device=0) / from_parquet(p, device=0): the Arrow buffers uploaded as they are and brought into the
column layout on the GPU (ingest.hip) give the table from_arrow(t).to_device(0) gives -- names, types, validity bytes,
offsets, string bytes and every fixed-width cell, buffer by buffer -- or the host path's error. Every comparison is
exact; the one exemption is the NULL cells of a timestamp column whose unit is not microseconds (Arrow leaves them
undefined)."""
import decimal
import random

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import deequ_amd.native as N
import deequ_amd.table as T
from deequ_amd import engine
from deequ_amd.table import ChunkedTable, DictColumn, Table, unpack_validity
from test_arrow_ingest import ROWS, NAMES, arrow_table
from test_gpu_arrow_ingest import ANALYZERS, metrics

pytestmark = pytest.mark.gpu


# ---- comparison -----------------------------------------------------------------------------------------------------
def tensor_bytes(x):
    return x.cpu().numpy().tobytes()


def loose_columns(t):
    """The timestamp columns whose unit is not microseconds: their NULL cells are not compared."""
    return {f.name for f in t.schema if pa.types.is_timestamp(f.type) and f.type.unit != "us"}


def assert_same(host, dev, loose=()):
    """`dev` (ingested on the device) against `host` (from_arrow(...).to_device(0)), buffer by buffer."""
    assert list(dev.schema.items()) == list(host.schema.items())
    assert dev.nrows == host.nrows
    for name, h in host.columns.items():
        d = dev[name]
        n = h.length
        assert type(d) is type(h), name
        assert d.length == n == host.nrows, name
        assert (d.spark_type, d.decimal_precision, d.decimal_scale, d.tz) == \
            (h.spark_type, h.decimal_precision, h.decimal_scale, h.tz), name
        kept = isinstance(h, DictColumn)
        hd, dd = (h.dict_device, d.dict_device) if kept else (h.device, d.device)
        assert d.values is None and dd is not None, name
        assert set(dd) == set(hd), (name, set(dd), set(hd))  # validity absent exactly when the host's is
        if "validity" in hd:
            assert len(tensor_bytes(dd["validity"])) == max((n + 63) // 64, 1) * 8, name
            assert tensor_bytes(dd["validity"]) == tensor_bytes(hd["validity"]), name  # zero at and past nrows
        if kept:
            assert d.indices is None and d.n_dict == h.n_dict, name
            for k in ("indices", "dict_values", "dict_offsets", "dict_validity"):
                assert dd[k].dtype == hd[k].dtype and tensor_bytes(dd[k]) == tensor_bytes(hd[k]), (name, k)
        elif h.spark_type == N.TYPE_STRING:
            assert str(dd["offsets"].dtype) == "torch.int32" and len(dd["offsets"]) == n + 1, name
            assert tensor_bytes(dd["offsets"]) == tensor_bytes(hd["offsets"]), name
            assert dd["values"].data_ptr() % 4 == 0, name
            total = int(dd["offsets"][n].item()) - int(dd["offsets"][0].item())
            got = dd["values"].cpu().numpy()
            assert len(got) == total + 16 and not got[total:].any(), name  # the 16 zero bytes after the bytes
            assert got.tobytes() == tensor_bytes(hd["values"]), name
        elif name in loose:
            valid = unpack_validity(h.validity, n)
            got = dd["values"].cpu().numpy().view(np.int64)
            want = hd["values"].cpu().numpy().view(np.int64)
            assert len(got) == len(want) == n and (got[valid] == want[valid]).all(), name
        else:
            assert tensor_bytes(dd["values"]) == tensor_bytes(hd["values"]), (name, h.type_name)  # floats bit for bit


def both(t, **kw):
    host = Table.from_arrow(t, **kw).to_device(0)
    dev = Table.from_arrow(t, device=0, **kw)
    assert isinstance(dev, Table)
    assert_same(host, dev, loose_columns(t))
    return host, dev


def error_of(f):
    try:
        f()
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return type(e), str(e)
    return None


def assert_same_error(t, **kw):
    want = error_of(lambda: Table.from_arrow(t, **kw))
    assert want is not None
    assert error_of(lambda: Table.from_arrow(t, device=0, **kw)) == want
    return want


# ---- arrays over buffers of exactly the bytes they need ----------------------------------------------------------------
def exact(arr):
    """`arr` (bool, fixed width, decimal128, string or large_string; any offset) over pa.py_buffer copies that end
    with the last byte the array needs: a read past an uploaded range has no padding to land in."""
    t, o, n = arr.type, arr.offset, len(arr)
    bufs = arr.buffers()
    cut = lambda b, nbytes: None if b is None else pa.py_buffer(b.to_pybytes()[:nbytes])  # noqa: E731
    out = [cut(bufs[0], (o + n + 7) // 8)]
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        w, dt = (8, np.int64) if pa.types.is_large_string(t) else (4, np.int32)
        offs = np.frombuffer(bufs[1], dtype=dt)[:o + n + 1]
        out += [cut(bufs[1], (o + n + 1) * w), cut(bufs[2], int(offs[-1])) if bufs[2] is not None else pa.py_buffer(b"")]
    elif pa.types.is_boolean(t):
        out.append(cut(bufs[1], (o + n + 7) // 8))
    else:
        out.append(cut(bufs[1], (o + n) * (t.bit_width // 8)))
    got = pa.Array.from_buffers(t, n, out, null_count=-1, offset=o)
    assert pa.types.is_floating(t) or got.equals(arr)  # (NaN cells never compare equal)
    return got


def null_mask(rng, n, mode):
    """True = NULL. `mode`: "some", "all", or "none" (then no mask: the array has no bitmap)."""
    if mode == "none":
        return None
    return np.ones(n, dtype=bool) if mode == "all" else rng.random(n) < 0.3


def bool_piece(rng, o, n, mode="some"):
    return exact(pa.array(rng.random(o + n) < 0.5, type=pa.bool_(), mask=null_mask(rng, o + n, mode)).slice(o, n))


def int_piece(rng, o, n, mode="some"):
    vals = rng.integers(-2 ** 31, 2 ** 31, o + n).astype(np.int32)
    return exact(pa.array(vals, type=pa.int32(), mask=null_mask(rng, o + n, mode)).slice(o, n))


def bit_table(rng, shapes):
    """A boolean and a nullable int column of the chunks `shapes` = [(offset, length, mode)]."""
    return pa.table([pa.chunked_array([bool_piece(rng, *s) for s in shapes], type=pa.bool_()),
                     pa.chunked_array([int_piece(rng, *s) for s in shapes], type=pa.int32())], names=["b", "i"])


OFFSETS = (0, 1, 7, 8, 9, 63, 64, 65)
LENGTHS = (0, 1, 63, 64, 65, 129)


# ---- bit addressing -------------------------------------------------------------------------------------------------
def test_bits_of_single_slices_at_every_offset_and_length():
    rng = np.random.default_rng(1)
    for o in OFFSETS:
        for n in LENGTHS:
            both(bit_table(rng, [(o, n, "some")]))


def test_bits_of_pieces_that_meet_inside_bytes_and_words():
    rng = np.random.default_rng(2)
    pick = random.Random(2)
    shapes = [(o, n) for o in OFFSETS for n in LENGTHS]
    totals = set()
    for nchunks in (2, 3):
        for _ in range(40):
            chosen = [pick.choice(shapes) + (pick.choice(["some", "some", "none", "all"]),) for _ in range(nchunks)]
            totals.add(sum(n for _, n, _ in chosen) % 64 == 0)
            both(bit_table(rng, chosen))
    # a chunk without a bitmap between chunks with one; an all-NULL chunk; totals that are / are not multiples of 64
    both(bit_table(rng, [(1, 63, "some"), (7, 65, "none"), (9, 1, "some")]))
    both(bit_table(rng, [(65, 129, "some"), (0, 64, "all"), (63, 63, "some")]))
    both(bit_table(rng, [(7, 63, "some"), (9, 65, "all")]))  # 128 rows
    both(bit_table(rng, [(8, 64, "all"), (1, 1, "none"), (64, 129, "some")]))  # 194 rows
    both(bit_table(rng, [(3, 64, "none"), (5, 64, "none")]))  # no bitmap anywhere: no validity
    assert totals == {True, False}


# ---- strings --------------------------------------------------------------------------------------------------------
WORDS = ["", "a", "bé", "日本語", "x" * 37, "", "tail", "ünïcødé", "0", " "]


def string_piece(rng, o, n, mode="some", large=False):
    vals = [WORDS[int(i)] for i in rng.integers(0, len(WORDS), o + n)]
    arr = pa.array(vals, type=pa.large_string() if large else pa.string(), mask=null_mask(rng, o + n, mode))
    return exact(arr.slice(o, n))


def test_strings_slices_empty_chunks_and_large_string():
    rng = np.random.default_rng(3)
    for large in (False, True):
        typ = pa.large_string() if large else pa.string()
        for shapes in ([(5, 40, "some")], [(1, 1, "none")], [(9, 65, "some"), (3, 0, "some"), (64, 70, "all"), (2, 9, "none")],
                       [(0, 0, "none")], [(7, 129, "none"), (65, 63, "some")]):
            chunks = [string_piece(rng, *s, large=large) for s in shapes]
            host, dev = both(pa.table([pa.chunked_array(chunks, type=typ)], names=["s"]))
            assert dev["s"].cells_at(np.arange(dev.nrows)) == pa.chunked_array(chunks, type=typ).to_pylist()
    sliced = string_piece(rng, 9, 65)
    assert np.frombuffer(sliced.buffers()[1], np.int32)[sliced.offset] > 0  # a slice whose first offset is not 0
    both(pa.table({"s": sliced}))
    both(pa.table({"s": pa.array(["", "", None, ""])}))


# ---- every fixed-width type -----------------------------------------------------------------------------------------
def decimal_piece(rng, n, precision, scale, mode="some", mask=None):
    """decimal128 cells over raw buffers: the NULL cells keep their (random) bytes, so zeroing them is the kernel's."""
    cells = np.empty((n, 2), dtype=np.int64)
    if precision <= 18:
        cells[:, 0] = rng.integers(-10 ** precision + 1, 10 ** precision, n)
        cells[:, 1] = np.where(cells[:, 0] < 0, -1, 0)
    else:
        cells[:] = rng.integers(-2 ** 63, 2 ** 63 - 1, (n, 2))
    mask = null_mask(rng, n, mode) if mask is None else mask
    bits = None if mask is None else pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.decimal128(precision, scale), n, [bits, pa.py_buffer(cells.tobytes())], null_count=-1)


def fixed_width_table(rng):
    def ints(dt, typ, shapes):
        info = np.iinfo(dt)
        return pa.chunked_array([exact(pa.array(rng.integers(info.min, info.max, o + n, dtype=dt, endpoint=True), type=typ,
                                                mask=null_mask(rng, o + n, mode)).slice(o, n)) for o, n, mode in shapes],
                                type=typ)

    def floats(dt, bits, typ, shapes):
        chunks = []
        for o, n, mode in shapes:
            raw = rng.integers(0, np.iinfo(bits).max, o + n, dtype=bits, endpoint=True)  # every bit pattern: NaN payloads
            raw[:2] = np.array([-0.0, np.nan], dtype=dt).view(bits)
            chunks.append(exact(pa.array(raw.view(dt), type=typ, mask=null_mask(rng, o + n, mode)).slice(o, n)))
        return pa.chunked_array(chunks, type=typ)

    def stamps(unit, tz, shapes):
        typ = pa.timestamp(unit, tz=tz)
        chunks = []
        for o, n, mode in shapes:
            v = rng.integers(-2 ** 63, 2 ** 63 - 1, o + n)
            v[:6] = [-1, -1001, 2 ** 62, -2 ** 63, 999, -1000]
            chunks.append(exact(pa.array(v, type=pa.int64(), mask=null_mask(rng, o + n, mode)).cast(typ).slice(o, n)))
        return pa.chunked_array(chunks, type=typ)

    shapes = [(1, 70, "some"), (0, 6, "none"), (9, 129, "some"), (3, 7, "all")]
    return pa.table([
        ints(np.int8, pa.int8(), shapes), ints(np.int16, pa.int16(), shapes), ints(np.int32, pa.int32(), shapes),
        ints(np.int64, pa.int64(), shapes), floats(np.float32, np.uint32, pa.float32(), shapes),
        floats(np.float64, np.uint64, pa.float64(), shapes),
        pa.chunked_array([c.cast(pa.date32()) for c in ints(np.int32, pa.int32(), shapes).chunks], type=pa.date32()),
        stamps("s", None, shapes), stamps("ms", "UTC", shapes), stamps("us", "Europe/Berlin", shapes),
        stamps("ns", None, shapes),
        pa.chunked_array([decimal_piece(rng, n, 12, 3, mode) for _, n, mode in shapes], type=pa.decimal128(12, 3)),
        pa.chunked_array([decimal_piece(rng, n, 18, 0, mode) for _, n, mode in shapes], type=pa.decimal128(18, 0)),
    ], names=["i8", "i16", "i32", "i64", "f32", "f64", "date", "ts_s", "ts_ms", "ts_us", "ts_ns", "dec12", "dec18"])


def test_every_fixed_width_type_cell_for_cell():
    t = fixed_width_table(np.random.default_rng(4))
    host, dev = both(t)
    assert dev["ts_ms"].tz == "UTC" and dev["ts_us"].tz == "Europe/Berlin" and dev["ts_s"].tz is None
    # the unit conversions the host's cast performs, on cells that are valid in the first chunk's second slice
    chunk = t["ts_ns"].chunk(1)
    assert chunk.null_count == 0
    ns = dev["ts_ns"].device["values"].cpu().numpy().view(np.int64)[70:76].tolist()
    assert ns[:2] == [0, -1] and ns[4:] == [0, -1]  # -1 ns -> 0, -1001 ns -> -1: truncated toward zero
    s = dev["ts_s"].device["values"].cpu().numpy().view(np.int64)[70:76].tolist()
    assert s[2] == 0 and s[0] == -10 ** 6  # 2^62 s wraps modulo 2^64 to 0


def test_wide_decimals_with_and_without_the_flag():
    rng = np.random.default_rng(5)
    t = pa.table([pa.chunked_array([decimal_piece(rng, 70, 38, 18, "some"), decimal_piece(rng, 9, 38, 18, "none"),
                                    decimal_piece(rng, 65, 38, 18, "all")], type=pa.decimal128(38, 18))], names=["w"])
    host, dev = both(t, wide_decimals=True)
    assert dev["w"].is_wide_decimal() and dev.schema["w"] == "DecimalType(38,18)"
    err = assert_same_error(t)
    assert err[0] is ValueError and "wide_decimals=True" in err[1]


# ---- kept dictionaries ----------------------------------------------------------------------------------------------
INDEX_TYPES = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64()]
ENTRIES = ["a", None, "ccc", "", "bé"]
PLAIN = ["a", "zz", "ccc", "", "bé"]  # for columns of several chunks: pyarrow cannot unify dictionaries with NULL entries


def dict_piece(index_type, indices, nulls, entries=ENTRIES):
    """A dictionary array whose index buffer holds `indices` as they are, NULL rows included."""
    n = len(indices)
    dt = np.dtype(index_type.to_pandas_dtype())
    bits = None if not any(nulls) else pa.py_buffer(np.packbits(~np.asarray(nulls, dtype=bool), bitorder="little").tobytes())
    ind = pa.Array.from_buffers(index_type, n, [bits, pa.py_buffer(np.asarray(indices).astype(dt).tobytes())], null_count=-1)
    return pa.DictionaryArray.from_arrays(ind, pa.array(entries, type=pa.string()), safe=False)


@pytest.mark.parametrize("index_type", INDEX_TYPES, ids=str)
def test_kept_dictionaries_of_every_index_type(index_type):
    rng = np.random.default_rng(6)
    n = 150
    idx = rng.integers(0, len(ENTRIES), n)
    nulls = rng.random(n) < 0.2
    idx[nulls] = np.where(rng.random(int(nulls.sum())) < 0.5, 100, idx[nulls])  # out of range on NULL rows: accepted
    arr, plain = dict_piece(index_type, idx, nulls), dict_piece(index_type, idx, nulls, PLAIN)
    for t in (pa.table({"d": arr}), pa.table({"d": arr.slice(7, 129)}),
              pa.table([pa.chunked_array([plain.slice(1, 63), plain.slice(64, 0), plain.slice(64, 86)])], names=["d"])):
        host, dev = both(t, dictionaries="keep")
        assert dev["d"].to_pylist() == t["d"].to_pylist()
        both(t, dictionaries="decode")
        both(t)
    # without NULL rows and NULL entries the validity is absent
    plain = dict_piece(index_type, rng.integers(0, 3, 70), np.zeros(70, bool), ["x", "yy", ""])
    host, dev = both(pa.table({"d": plain}), dictionaries="keep")
    assert "validity" not in dev["d"].dict_device
    # NULL entries alone make NULL rows
    host, dev = both(pa.table({"d": dict_piece(index_type, rng.integers(0, len(ENTRIES), 70), np.zeros(70, bool))}),
                     dictionaries="keep")
    assert "validity" in dev["d"].dict_device


@pytest.mark.parametrize("index_type", [pa.int8(), pa.uint16(), pa.int64()], ids=str)
def test_dictionary_index_out_of_range_is_the_hosts_error(index_type):
    idx = np.array([0, 1, 2, 3, 4] * 30)
    nulls = np.zeros(150, bool)
    nulls[[3, 77]] = True
    idx[3] = 99  # on a NULL row: accepted
    idx[[80, 141]] = [5, 100]
    arr = dict_piece(index_type, idx, nulls)
    err = assert_same_error(pa.table({"d": arr}), dictionaries="keep")
    assert err == (ValueError, "column d: row 80 has dictionary index 5 outside [0, 5)")
    err = assert_same_error(pa.table({"d": arr.slice(9, 135)}), dictionaries="keep")
    assert "row 71 has dictionary index 5" in err[1]
    assert_same_error(pa.table([pa.chunked_array([arr.slice(0, 70), arr.slice(70, 80)])], names=["d"]), dictionaries="keep")
    if index_type != pa.uint16():
        idx[80] = -1
        err = assert_same_error(pa.table({"d": dict_piece(index_type, idx, nulls)}), dictionaries="keep")
        assert "row 80 has dictionary index -1" in err[1]


def test_chunks_with_different_dictionaries_and_other_value_types():
    a = pa.DictionaryArray.from_arrays(pa.array([0, 1, None, 1, 0], pa.int8()), pa.array(["x", "y"]))
    b = pa.DictionaryArray.from_arrays(pa.array([1, 0, 2, None], pa.int8()), pa.array(["y", "z", "w"]))
    t = pa.table([pa.chunked_array([a, b]), pa.chunked_array([a.slice(1, 4), b.slice(0, 4), a.slice(0, 1)])],
                 names=["d", "e"])
    for mode in ("keep", "decode"):
        host, dev = both(t, dictionaries=mode)
        assert dev["d"].cells_at(np.arange(dev.nrows)) == t["d"].to_pylist()
    numbers = pa.DictionaryArray.from_arrays(pa.array([0, 1, None, 1], pa.int16()), pa.array([10, 20], pa.int64()))
    large = pa.DictionaryArray.from_arrays(pa.array([0, 1, None, 1], pa.int16()), pa.array(["p", None], pa.large_string()))
    both(pa.table({"n": numbers, "l": large}), dictionaries="keep")  # dictionaries of other values decode either way


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_errors_equal_the_hosts():
    ok = pa.array([1, 2, 3])
    e = assert_same_error(pa.table({"a": ok, "d": pa.array([1, 2, 3], pa.date64())}))
    assert e[0] is ValueError and "date64" in e[1]
    assert_same_error(pa.table({"w": pa.array([decimal.Decimal("1.5")] * 3, pa.decimal128(30, 2))}))
    e = assert_same_error(pa.table({"a": ok}), dictionaries="encode")
    assert e[0] is ValueError and "dictionaries" in e[1]
    # the first column in error speaks, as on the host
    e = assert_same_error(pa.table({"w": pa.array([decimal.Decimal("1.5")] * 3, pa.decimal128(30, 2)),
                                    "d": pa.array([1, 2, 3], pa.date64())}))
    assert "wide_decimals" in e[1]
    with pytest.raises(ValueError, match="chunk_rows"):
        Table.from_arrow(pa.table({"a": ok}), device=0, chunk_rows=0)


# ---- zero rows ------------------------------------------------------------------------------------------------------
def test_zero_rows_and_zero_chunks():
    types = [pa.int64(), pa.string(), pa.large_string(), pa.bool_(), pa.float32(), pa.timestamp("ns"),
             pa.decimal128(9, 2), pa.dictionary(pa.int8(), pa.string())]
    names = ["c%d" % i for i in range(len(types))]
    for mode in ("decode", "keep"):
        both(pa.table([pa.array([], type=t) for t in types], names=names), dictionaries=mode)
        both(pa.table([pa.chunked_array([], type=t) for t in types], names=names), dictionaries=mode)
        both(pa.table([pa.chunked_array([pa.array([], type=t), pa.array([], type=t)], type=t) for t in types], names=names),
             dictionaries=mode)


# ---- random tables, chunk_rows --------------------------------------------------------------------------------------
def random_column(rng, pick, kind, n):
    """A ChunkedArray of `n` rows of `kind`, cut into random chunks that are random slices of longer arrays."""
    cuts = sorted(pick.randrange(n + 1) for _ in range(pick.choice([0, 1, 2, 4])))
    lengths = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    chunks = []
    for m in lengths:
        o = pick.choice([0, 0, 1, 7, 8, 9, 63, 65])
        mode = pick.choice(["some", "some", "none", "all"])
        if kind == "bool":
            c = bool_piece(rng, o, m, mode)
        elif kind == "int32":
            c = int_piece(rng, o, m, mode)
        elif kind in ("string", "large_string"):
            c = string_piece(rng, o, m, mode, large=kind == "large_string")
        elif kind in ("int8", "int64", "float64", "date32"):
            dt = {"int8": np.int8, "int64": np.int64, "float64": np.int64, "date32": np.int32}[kind]
            raw = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, o + m, dtype=dt, endpoint=True)
            a = pa.array(raw.view(np.float64) if kind == "float64" else raw, mask=null_mask(rng, o + m, mode))
            c = exact((a.cast(pa.date32()) if kind == "date32" else a).slice(o, m))
        elif kind.startswith("ts_"):
            a = pa.array(rng.integers(-2 ** 63, 2 ** 63 - 1, o + m), type=pa.int64(), mask=null_mask(rng, o + m, mode))
            c = exact(a.cast(pa.timestamp(kind[3:])).slice(o, m))
        elif kind == "dec":
            c = decimal_piece(rng, m, 15, 4, mode)
        elif kind == "wide":
            c = decimal_piece(rng, m, 38, 10, mode)
        else:  # "dict"
            nulls = null_mask(rng, o + m, mode)
            c = dict_piece(pa.int16(), rng.integers(0, len(ENTRIES), o + m),
                           np.zeros(o + m, bool) if nulls is None else nulls, ENTRIES if len(lengths) == 1 else PLAIN).slice(o, m)
        chunks.append(c)
    return pa.chunked_array(chunks, type=chunks[0].type)


KINDS = ["bool", "int32", "string", "large_string", "int8", "int64", "float64", "date32", "ts_s", "ts_ms", "ts_us", "ts_ns",
         "dec", "wide", "dict"]


def assert_chunked_same(t, k, **kw):
    """from_arrow(t, device=0, chunk_rows=k) against the device tables of t's slices of k rows."""
    got = Table.from_arrow(t, device=0, chunk_rows=k, **kw)
    if t.num_rows <= k:
        assert isinstance(got, Table)
        assert_same(Table.from_arrow(t, **kw).to_device(0), got, loose_columns(t))
        return got
    assert isinstance(got, ChunkedTable) and len(got.chunks) == (t.num_rows + k - 1) // k and got.nrows == t.num_rows
    for i, chunk in enumerate(got.chunks):
        assert_same(Table.from_arrow(t.slice(i * k, k), **kw).to_device(0), chunk, loose_columns(t))
    return got


@pytest.mark.parametrize("block", range(4))
def test_random_tables_whole_and_chunked(block):
    """200 seeded tables, 50 a case."""
    rng = np.random.default_rng(70 + block)
    pick = random.Random(70 + block)
    for trial in range(50):
        n = pick.choice([0, 1, 2, 63, 64, 65, pick.randrange(301), pick.randrange(301)])
        kinds = pick.sample(KINDS, pick.randrange(1, 5))
        t = pa.table([random_column(rng, pick, kind, n) for kind in kinds], names=kinds)
        kw = dict(wide_decimals=True, dictionaries=pick.choice(["keep", "decode"]))
        both(t, **kw)
        assert_chunked_same(t, pick.choice([max(n // 3, 1), 64, 100, max(n - 1, 1), max(n, 1), n + 1]), **kw)


def test_chunk_rows_boundaries_inside_chunks_bytes_and_words():
    rng = np.random.default_rng(8)
    pick = random.Random(8)
    kinds = ["bool", "int32", "string", "ts_ns", "dec", "dict", "float64"]
    t = pa.table([random_column(rng, pick, kind, 300) for kind in kinds], names=kinds)
    for k in (60, 64, 67, 128, 299, 300, 301):
        assert_chunked_same(t, k, dictionaries="keep")
    for k in (1, 3, 8):
        assert_chunked_same(t.slice(59, 20), k, dictionaries="keep")


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_parquet_on_the_device_gives_the_row_tables_metrics(tmp_path):
    assert len(ANALYZERS) == 15
    want = metrics(Table.from_rows(ROWS, NAMES, ["string", "string", "int", "double", "boolean"]))
    p = str(tmp_path / "t.parquet")
    pq.write_table(arrow_table(), p, row_group_size=4)
    dev = Table.from_parquet(p, device=0)
    assert_same(Table.from_parquet(p).to_device(0), dev)
    assert metrics(dev) == want
    assert metrics(Table.from_parquet(p, device=0, dictionaries="keep")) == want
    chunked = Table.from_parquet(p, device=0, chunk_rows=4)
    assert isinstance(chunked, ChunkedTable) and [c.nrows for c in chunked.chunks] == [4, 2]
    assert metrics(chunked) == want  # against the unchunked host table's metrics
    assert metrics(Table.from_arrow(arrow_table(), device=0, chunk_rows=5)) == want  # a boundary inside a chunk


# ---- no host row pass, launch counts --------------------------------------------------------------------------------
def plain_table(rng, n, nchunks):
    """Types the device path handles without a host exception, `nchunks` chunks a column, a NULL in every chunk."""
    cuts = [n * i // nchunks for i in range(nchunks + 1)]

    def column(make):
        return pa.chunked_array([make(b - a) for a, b in zip(cuts, cuts[1:])])

    def nulls(m):
        mask = rng.random(m) < 0.1
        mask[0] = True
        return mask

    return pa.table({
        "l": column(lambda m: pa.array(rng.integers(-9, 9, m), mask=nulls(m))),
        "d": column(lambda m: pa.array(rng.random(m), mask=nulls(m))),
        "b": column(lambda m: pa.array(rng.random(m) < 0.5, mask=nulls(m))),
        "s": column(lambda m: pa.array([WORDS[i] for i in rng.integers(0, len(WORDS), m)], mask=nulls(m))),
        "t": column(lambda m: pa.array(rng.integers(-10 ** 12, 10 ** 12, m), pa.int64(), mask=nulls(m))
                    .cast(pa.timestamp("ns"))),
        "m": column(lambda m: decimal_piece(rng, m, 10, 2, mask=nulls(m))),
    })


def test_no_host_pass_over_the_rows(monkeypatch):
    t = plain_table(np.random.default_rng(9), 1000, 3)
    host = Table.from_arrow(t).to_device(0)

    def refuse(*a, **kw):
        raise AssertionError("the device path walked the rows on the host")

    class Guarded:
        """A pyarrow object whose combine_chunks raises: pyarrow's extension types cannot be patched, so the table
        and the columns it hands out are wrapped instead."""

        def __init__(self, inner):
            self._inner = inner

        def __getattr__(self, name):
            if name == "combine_chunks":
                return refuse
            value = getattr(self._inner, name)
            if name == "columns":
                return [Guarded(c) for c in value]
            if name == "slice":
                return lambda *a: Guarded(value(*a))
            return value

    monkeypatch.setattr(T, "_column_from_arrow", refuse)
    monkeypatch.setattr(Table, "to_device", refuse)
    with pytest.raises(AssertionError):
        Table.from_arrow(Guarded(t))  # the host path does walk the rows: the guard works
    dev = Table.from_arrow(Guarded(t), device=0)
    monkeypatch.undo()
    assert_same(host, dev, loose_columns(t))


def test_launch_counts_do_not_depend_on_the_rows():
    rng = np.random.default_rng(10)
    ctx = engine.ctx()
    grown = []
    for n in (10, 10000):
        t = plain_table(rng, n, 3)
        before = ctx.ingest_kernel_launches()
        dev = Table.from_arrow(t, device=0)
        after = ctx.ingest_kernel_launches()
        assert dev.nrows == n
        grown.append({k: after[k] - before[k] for k in after})
    assert grown[0] == grown[1] and sum(grown[0].values()) > 0, grown
    # one validity launch per column with NULLs, one boolean launch, one offsets launch per string piece
    assert grown[0]["ingest_validity"] == 6 and grown[0]["ingest_bool"] == 1 and grown[0]["ingest_offsets"] == 3
    assert grown[0]["ingest_convert"] == 6 and grown[0]["ingest_indices"] == 0
