"""RowLevelSchemaValidator on the GPU against the Python model (tests/schema_model.py): the reference's test cases end
to end, the NULL-verdict quirk of an int minimum, the verdict kernel's row-tile / staging edges, a randomized table
(also in two chunks), compaction extremes, the ambiguous-cell policy and the single verdict launch."""
import functools
import random

import numpy as np
import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import engine
from deequ_amd import schema as S
from deequ_amd.table import ChunkedTable, Table, unpack_validity

import schema_model as M
from schema_cases import build_schema, check_kat_members, load_kats

pytestmark = pytest.mark.gpu


def make_table(columns, rows, device):
    t = Table.from_rows(rows, columns, types=[N.TYPE_STRING] * len(columns))
    return t.to_device(0) if device else t


def check_string_layout(col, device):
    """Offsets start at 0 and ascend; the bytes end where the offsets say, plus 16 zero bytes in HBM."""
    if device:
        assert col.values is None and col.device is not None
        off = col.device["offsets"].cpu().numpy()
        data = col.device["values"].cpu().numpy()
        assert len(data) == int(off[-1]) + 16 and not data[int(off[-1]):].any()
    else:
        assert col.device is None
        off = np.asarray(col.offsets)
        assert len(col.values) == int(off[-1])
    assert off.dtype == np.int32 and len(off) == col.length + 1 and off[0] == 0 and (np.diff(off) >= 0).all()


def table_cells(table, device):
    """Rows of Python cells: str, int (INT), unscaled int (DECIMAL), microseconds (TIMESTAMP), None for NULL."""
    cols = []
    for c in table.columns.values():
        if c.spark_type == N.TYPE_STRING:
            check_string_layout(c, device)
        h = S._to_host(c) if device else c
        valid = unpack_validity(h.validity, h.length)
        if h.spark_type == N.TYPE_STRING:
            data, off = bytes(np.asarray(h.values, dtype=np.uint8)), np.asarray(h.offsets)
            cols.append([data[off[i]:off[i + 1]].decode("utf-8") if valid[i] else None for i in range(h.length)])
        else:
            vals = np.asarray(h.values)
            cols.append([int(vals[i]) if valid[i] else None for i in range(h.length)])
    return [list(r) for r in zip(*cols)]


def check_against_model(columns, rows, spec, device, ambiguous="error"):
    """validate() == the model: counts, the rows of both outputs in order, cast values and NULLs, column types."""
    want = M.validate(columns, rows, spec)
    res = D.RowLevelSchemaValidator.validate(make_table(columns, rows, device), build_schema(spec), ambiguous=ambiguous)
    assert (res.numValidRows, res.numInvalidRows, res.numUnknownRows, res.numAmbiguousRows) == \
        (len(want.valid), len(want.invalid), want.num_unknown, want.num_ambiguous)
    assert res.validRows.nrows == len(want.valid) and res.invalidRows.nrows == len(want.invalid)
    assert list(res.validRows.columns) == columns and list(res.invalidRows.columns) == columns
    assert table_cells(res.validRows, device) == want.valid
    assert table_cells(res.invalidRows, device) == want.invalid
    types = {d["name"]: d for d in spec if d["type"] != "string"}
    for name in columns:
        d = types.get(name)
        exp = "StringType" if d is None else {"int": "IntegerType", "timestamp": "TimestampType"}.get(
            d["type"], "DecimalType(%d,%d)" % (d.get("precision", 0), d.get("scale", 0)))
        assert res.validRows[name].type_name == exp
        assert res.invalidRows[name].type_name == "StringType"
    return res, want


# ---- 1. the reference's cases --------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", load_kats(), ids=lambda c: c["name"])
def test_reference_cases_end_to_end(case, device):
    res, want = check_against_model(case["columns"], case["rows"], case["schema"], device)
    assert (res.numValidRows, res.numInvalidRows) == (case["numValid"], case["numInvalid"])
    check_kat_members(case, table_cells(res.validRows, device), table_cells(res.invalidRows, device))
    for name, t in case.get("validTypes", {}).items():
        assert res.validRows[name].type_name == t
    for name, t in case.get("invalidTypes", {}).items():
        assert res.invalidRows[name].type_name == t


# ---- 2. `colIsNull.isNull or cast >= min` ----------------------------------------------------------------------------
def test_int_minimum_makes_null_cells_unknown():
    columns, rows = ["k", "v"], [["a", "5"], ["b", None], ["c", "-20"], ["d", None], ["e", "x"]]
    spec = [{"type": "int", "name": "v", "minValue": 0}]
    res, _ = check_against_model(columns, rows, spec, True)
    assert (res.numValidRows, res.numInvalidRows, res.numUnknownRows) == (1, 2, 2)
    keys = [r[0] for r in table_cells(res.validRows, True)] + [r[0] for r in table_cells(res.invalidRows, True)]
    assert "b" not in keys and "d" not in keys
    spec = [{"type": "int", "name": "v", "minValue": 0, "isNullable": False}]
    res, _ = check_against_model(columns, rows, spec, True)
    assert (res.numValidRows, res.numInvalidRows, res.numUnknownRows) == (1, 4, 0)
    # without a minimum a NULL cell is valid
    res, _ = check_against_model(columns, rows, [{"type": "int", "name": "v", "maxValue": 10}], True)
    assert (res.numValidRows, res.numInvalidRows, res.numUnknownRows) == (4, 1, 0)


# ---- 3. kernel mechanics -------------------------------------------------------------------------------------------
MECH_SPEC = [
    {"type": "string", "name": "s", "minLength": 2, "maxLength": 6000, "matches": "^[a-z0-9_\\-\\s]+$"},
    {"type": "int", "name": "i", "minValue": -10, "maxValue": 1000},
    {"type": "decimal", "name": "d", "precision": 10, "scale": 2},
    {"type": "timestamp", "name": "t", "mask": "yyyy-MM-dd HH:mm:ss"},
]
MECH_COLUMNS = ["rowid", "s", "i", "d", "t", "z"]
S_CELLS = ["hello", "", "héllo wörld", "UPPER", None, "ab", "hello_world-1 2", "日本語", "a", "x" * 40, "tab\there"]
I_CELLS = ["12", "-7", "N/A", None, "1001", "-11", "1000", "-10", "2147483648", "3.9", "+5", "", "-2147483648"]
D_CELLS = ["299.000", "1295", "###", "-19.99", None, "0.005", "-0.005", "99999999.994", "99999999.995", "1e3", "1.5e-1",
           ".5", "5.", " 1", "12345678901", "-0"]
T_CELLS = ["2012-07-22 22:59:59", None, "N/A", "1999-12-31 00:00:00", "2024-02-29 12:30:00", "yesterday", "2012-07-22",
           "9999-12-31 23:59:59", "1583-01-01 00:00:00", ""]


@functools.lru_cache(maxsize=None)
def mech_rows(n):
    """Every 64-row group holds one 5000-byte cell per schema column (its wave then reads the bytes in place, not from
    the LDS stage): a string that passes the lengths and fails the regex at its first character, an int and a decimal
    with a long fraction (values 7 and 1.00), a timestamp cell that fails the walk."""
    rows = []
    for k in range(n):
        s, i, d, t = S_CELLS[k % len(S_CELLS)], I_CELLS[k % len(I_CELLS)], D_CELLS[k % len(D_CELLS)], T_CELLS[k % len(T_CELLS)]
        if k % 64 == 7:
            s = "X" + "x" * 4999
        if k % 64 == 21:
            i = "7." + "0" * 4998
        if k % 64 == 35:
            d = "1." + "0" * 4998
        if k % 64 == 49:
            t = "N" * 5000
        rows.append(["r%05d" % k, s, i, d, t, None])
    return rows


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257, 4099])
def test_verdict_and_compaction_mechanics(n):
    res, want = check_against_model(MECH_COLUMNS, mech_rows(n), MECH_SPEC, True)
    assert res.numAmbiguousRows == 0
    if n >= 257:
        assert res.numValidRows > 0 and res.numInvalidRows > 0 and res.numUnknownRows > 0
        assert res.validRows["rowid"].device.get("validity") is None  # no validity buffer in, none out


def test_all_null_and_never_null_schema_columns():
    rows = [[r[0], r[1], I_CELLS[k % 3 if k % 3 != 2 else 0], None, r[4], r[5]] for k, r in enumerate(mech_rows(257))]
    assert all(r[2] is not None for r in rows)
    res, _ = check_against_model(MECH_COLUMNS, rows, MECH_SPEC, True)
    assert res.numValidRows > 0 and res.numUnknownRows == 0


def test_pattern_whose_first_match_is_empty():
    """`matches` needs the FIRST match of Matcher.find() to be non-empty: "ax" has the empty match of `x*` at 0 before
    the "x" at 1, so it is invalid like ""; a NULL cell is valid. 130 rows: two full waves and a 2-row tail."""
    cells = ["", "x", "ax", "xa", None]
    rows = [["r%03d" % k, cells[k % 5]] for k in range(130)]
    res, _ = check_against_model(["rowid", "s"], rows, [{"type": "string", "name": "s", "matches": "x*"}], True)
    assert (res.numValidRows, res.numInvalidRows, res.numUnknownRows) == (78, 52, 0)
    assert {r[1] for r in table_cells(res.invalidRows, True)} == {"", "ax"}


# ---- 4. a randomized table -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_rows(n=20000, seed=77):
    rng = random.Random(seed)

    def good_s():
        return "".join(rng.choice("abcxyz019_- ") for _ in range(rng.randint(2, 20)))

    def bad_s():
        return rng.choice(["", "a", "Hello", "naïve", "semi;colon", "x" * 25, "日本"])

    def good_i():
        return str(rng.randint(-10, 1000)) + rng.choice(["", "", ".0", ".75"])

    def bad_i():
        return rng.choice(["N/A", "", "1001", "-11", "99999999999", "1e3", " 5", "5 ", "--1", "+", "0x1"])

    def good_d():
        return rng.choice(["", "-", "+"]) + str(rng.randint(0, 99999999)) + rng.choice(["", ".", ".5", ".25", ".125", ".995"])

    def bad_d():
        return rng.choice(["###", "n/a", "", "1e9", "123456789", "99999999.995", "1,5", "1.5.2", ".", "NaN", "1 ", "5e"])

    def good_t():
        return "%04d-%02d-%02d %02d:%02d:%02d" % (rng.randint(1583, 9999), rng.randint(1, 12), rng.randint(1, 28),
                                                   rng.randint(0, 23), rng.randint(0, 59), rng.randint(0, 59))

    def bad_t():  # the walk fails: NULL, never ambiguous
        return rng.choice(["N/A", "", "yesterday", "2012-07-22", "2012/07/22 10:00:00", "2012-07-22T10:00:00", "-", "12:00:00"])

    rows = []
    for k in range(n):
        row = ["r%05d" % k]
        for good, bad in ((good_s, bad_s), (good_i, bad_i), (good_d, bad_d), (good_t, bad_t)):
            x = rng.random()
            row.append(None if x < 0.04 else (bad() if x < 0.12 else good()))
        rows.append(row)
    return rows


RANDOM_COLUMNS = ["rowid", "s", "i", "d", "t"]
RANDOM_SPEC = [
    {"type": "string", "name": "s", "minLength": 2, "maxLength": 20, "matches": "^[a-z0-9_\\-\\s]+$"},
    {"type": "int", "name": "i", "minValue": -10, "maxValue": 1000, "isNullable": False},
    {"type": "decimal", "name": "d", "precision": 10, "scale": 2},
    {"type": "timestamp", "name": "t", "mask": "yyyy-MM-dd HH:mm:ss"},
]


def test_randomized_table_matches_model():
    rows = random_rows()
    res, want = check_against_model(RANDOM_COLUMNS, rows, RANDOM_SPEC, False)
    assert res.numAmbiguousRows == 0 and res.numUnknownRows == 0
    frac = res.numInvalidRows / len(rows)
    assert 0.2 < frac < 0.45, frac  # about 30 % of the rows hold a bad cell


def test_randomized_table_in_two_chunks_is_the_concatenation():
    rows = random_rows()
    want = M.validate(RANDOM_COLUMNS, rows, RANDOM_SPEC)
    cut = 9001
    chunks = ChunkedTable([make_table(RANDOM_COLUMNS, rows[:cut], True), make_table(RANDOM_COLUMNS, rows[cut:], True)])
    res = D.RowLevelSchemaValidator.validate(chunks, build_schema(RANDOM_SPEC))
    assert isinstance(res.validRows, ChunkedTable) and isinstance(res.invalidRows, ChunkedTable)
    assert (res.numValidRows, res.numInvalidRows, res.numUnknownRows, res.numAmbiguousRows) == \
        (len(want.valid), len(want.invalid), 0, 0)
    assert res.validRows.nrows == len(want.valid) and res.invalidRows.nrows == len(want.invalid)
    assert sum((table_cells(t, True) for t in res.validRows.chunks), []) == want.valid
    assert sum((table_cells(t, True) for t in res.invalidRows.chunks), []) == want.invalid


# ---- 5. compaction extremes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["all", "none", "alternating", "last"])
def test_compaction_extremes(shape):
    n = 65 if shape == "last" else 200
    good = {"all": lambda k: True, "none": lambda k: False, "alternating": lambda k: k % 2 == 0,
            "last": lambda k: k == n - 1}[shape]
    rows = [["r%03d" % k, str(k) if good(k) else "bad%d" % k] for k in range(n)]
    res, _ = check_against_model(["rowid", "v"], rows, [{"type": "int", "name": "v"}], True)
    assert res.numValidRows == sum(1 for k in range(n) if good(k))
    assert res.numValidRows + res.numInvalidRows == n


# ---- 6. ambiguous cells ----------------------------------------------------------------------------------------------
def test_ambiguous_cells_raise_or_become_invalid():
    columns = ["rowid", "t", "d"]
    rows = [["a", "2012-7-22 22:59:59", "1.0"], ["b", "2012-07-22 22:59:59", "１.5"],
            ["c", "2012-07-22 22:59:59", "2.5"], ["e", None, None]]
    spec = [{"type": "timestamp", "name": "t", "mask": "yyyy-MM-dd HH:mm:ss"},
            {"type": "decimal", "name": "d", "precision": 10, "scale": 2}]
    with pytest.raises(N.NativeError) as ei:
        D.RowLevelSchemaValidator.validate(make_table(columns, rows, True), build_schema(spec))
    assert ei.value.status == -2 and "2 rows" in str(ei.value) and "'t'" in str(ei.value)
    res, want = check_against_model(columns, rows, spec, True, ambiguous="invalid")
    assert want.first_ambiguous == "t"
    assert (res.numValidRows, res.numInvalidRows, res.numAmbiguousRows) == (2, 2, 2)
    assert [r[0] for r in table_cells(res.invalidRows, True)] == ["a", "b"]


# ---- 7. one pass -------------------------------------------------------------------------------------------------------
def test_four_definitions_are_one_verdict_launch():
    t = make_table(MECH_COLUMNS, mech_rows(257), True)
    ctx = engine.ctx()
    before = ctx.schema_launch_count()
    D.RowLevelSchemaValidator.validate(t, build_schema(MECH_SPEC))
    assert ctx.schema_launch_count() - before == 1
