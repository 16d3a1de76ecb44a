"""Tables for the CSV writer's tests (test_csv_write.py on the CPU, test_gpu_csv_write.py on the GPU)."""
import random

import numpy as np

from deequ_amd import native as N
from deequ_amd.table import Column, Table, pack_validity, _column_from_pylist

STRING_POOL = ["", "a", "a,b", '"', 'say "hi"', "line\nbreak", "cr\rhere", "crlf\r\nin", "é", "日本語", " lead", "trail ",
               "plain", "1", "-", "1.5", "x" * 63, "y" * 64, "z" * 65, ',' * 9, '"' * 17, "tab\there"]


def strings_column(name, items):
    return _column_from_pylist(name, "string", items)


def bytes_column(name, cells, valid=None):
    """A STRING column from raw byte strings (any bytes); `valid`: bool per row (None: no bitmap)."""
    offsets = np.zeros(len(cells) + 1, dtype=np.int32)
    if cells:
        offsets[1:] = np.cumsum([len(b) for b in cells])
    data = np.frombuffer(b"".join(cells), dtype=np.uint8).copy() if cells else np.zeros(0, np.uint8)
    return Column(name, N.TYPE_STRING, data, None if valid is None else pack_validity(valid), offsets, length=len(cells))


def every_type_table(n, seed=5, nulls=True, bitmap=True):
    """One column of every type the writer accepts, n rows. nulls: about one cell in six is NULL; bitmap without nulls:
    a bitmap with every bit set; neither: no bitmap at all."""
    rng = np.random.default_rng(seed)
    pr = random.Random(seed)

    def validity():
        if nulls:
            return pack_validity(rng.random(n) > 1 / 6)
        return pack_validity(np.ones(n, dtype=bool)) if bitmap else None

    def pick(edges, lo, hi, dtype):
        v = rng.integers(lo, hi, n, dtype=np.int64)
        k = min(n, len(edges))
        v[:k] = edges[:k]
        return v.astype(dtype)

    doubles = rng.normal(0, 1e3, n)
    special = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e10, 1e-5, 1e7, 1e-3, 9999999.999, 4.9e-324,
               1.7976931348623157e308, 123456.789]
    doubles[:min(n, len(special))] = special[:n]
    floats = rng.normal(0, 1e3, n).astype(np.float32)
    floats[:min(n, 8)] = np.array([0.0, -0.0, np.nan, np.inf, 1e10, 1e-5, 3.4028235e38, 1.17549435e-38],
                                  dtype=np.float32)[:n]
    cols = [
        Column("flag", N.TYPE_BOOLEAN, (rng.random(n) < 0.5).astype(np.uint8), validity()),
        Column("b", N.TYPE_BYTE, pick([-128, 127, 0], -128, 128, np.int8), validity()),
        Column("s", N.TYPE_SHORT, pick([-32768, 32767, 0], -32768, 32768, np.int16), validity()),
        Column("i", N.TYPE_INT, pick([-2 ** 31, 2 ** 31 - 1, 0, -1], -2 ** 31, 2 ** 31, np.int32), validity()),
        Column("l", N.TYPE_LONG, pick([-2 ** 63, 2 ** 63 - 1, 0, 10 ** 18], -2 ** 62, 2 ** 62, np.int64), validity()),
        Column("f", N.TYPE_FLOAT, floats, validity()),
        Column("d", N.TYPE_DOUBLE, doubles, validity()),
        Column("dec", N.TYPE_DECIMAL, pick([1, -1, 0, 10, 999999999999999999, -999999999999999999, 15], -10 ** 12, 10 ** 12,
                                           np.int64), validity(), decimal_precision=18, decimal_scale=8),
        Column("day", N.TYPE_DATE, pick([-141428, -141427, -719164, 0, 2932896, 2932897, -1, -719529], -800000, 3000000,
                                        np.int32), validity()),
        Column("ts", N.TYPE_TIMESTAMP, pick([0, -1, 1500000, 253402300800000000, -62135596800000000, 999999],
                                            -10 ** 17, 10 ** 17, np.int64), validity()),
    ]
    items = [pr.choice(STRING_POOL) for _ in range(n)]
    sc = strings_column("text", items)
    sc.validity = validity()
    cols.append(sc)
    return Table(cols)


def round_trippable(n=40, seed=9):
    """A table `from_csv(infer_schema=True)` reads back with the same types and values: a LONG column with a value
    beyond int32, an INT, a DOUBLE and a BOOLEAN column and a string column of non-empty, non-numeric cells; every
    column but the first has NULLs."""
    rng = np.random.default_rng(seed)
    pr = random.Random(seed)

    def some(v):
        return [None if (k and rng.random() < 0.2) else x for k, x in enumerate(v)]

    longs = [2 ** 40 + 7] + [int(x) for x in rng.integers(-2 ** 62, 2 ** 62, n - 1)]
    ints = [int(x) for x in rng.integers(-2 ** 31, 2 ** 31, n)]
    doubles = [1e10, 1e-5, -0.0, 1.5] + [float(x) for x in rng.normal(0, 100, n - 4)]
    flags = [bool(x) for x in rng.random(n) < 0.5]
    words = ["alpha", "a,b", 'q"q', "two\nlines", "é", "x y", "cr\r", "-"]
    text = [pr.choice(words) for _ in range(n)]
    return Table.from_pydict({"big": longs, "n": some(ints), "x": some(doubles), "ok": some(flags), "w": some(text)},
                             types={"big": "long", "n": "int", "x": "double", "ok": "boolean", "w": "string"})


def reader_alphabet_cells(count, seed=11):
    """Random cells over the reader model's alphabet (tests/csv_model.py), 0-14 tokens each, as bytes."""
    rng = random.Random(seed)
    alphabet = [",", '"', "\n", "\r", "\r\n", "1", "a", ".", " ", "-", "é"]
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 14))).encode("utf-8") for _ in range(count)]
