"""Shared by the row-level schema tests: the reference's cases (tests/golden/schema_kats.json), a RowLevelSchema
built from their schema parameters, and the reference test's member assertions."""
import json
import os

import deequ_amd as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_kats():
    with open(os.path.join(ROOT, "tests", "golden", "schema_kats.json")) as f:
        return json.load(f)["cases"]


def build_schema(spec):
    s = D.RowLevelSchema()
    for d in spec:
        nullable = d.get("isNullable", True)
        if d["type"] == "string":
            s = s.withStringColumn(d["name"], nullable, d.get("minLength"), d.get("maxLength"), d.get("matches"))
        elif d["type"] == "int":
            s = s.withIntColumn(d["name"], nullable, d.get("minValue"), d.get("maxValue"))
        elif d["type"] == "decimal":
            s = s.withDecimalColumn(d["name"], d["precision"], d["scale"], nullable)
        else:
            s = s.withTimestampColumn(d["name"], d["mask"], nullable)
    return s


def check_kat_members(case, valid_rows, invalid_rows):
    """The reference test's member assertions over rows given as lists of cells in table column order (decimals as
    unscaled ints at the definition's scale)."""
    cols = case["columns"]
    vm = case.get("validMembers")
    if vm:
        got = [r[cols.index(vm["column"])] for r in valid_rows]
        want = vm["equals"]
        d = [x for x in case["schema"] if x["name"] == vm["column"]][-1]
        if d["type"] == "decimal":
            from decimal import Decimal
            want = [int(Decimal(w).scaleb(d["scale"])) for w in want]
        assert sorted(map(repr, got)) == sorted(map(repr, want))
    im = case.get("invalidMembers")
    if im:
        got = [r[cols.index(im["column"])] for r in invalid_rows]
        assert len(set(got)) == im["size"]
        for x in im.get("contains", []):
            assert x in got
        for x in im.get("excludes", []):
            assert x not in got
    pc = case.get("invalidPrefixCounts")
    if pc:
        got = [r[cols.index(pc["column"])] for r in invalid_rows]
        for prefix, cnt in pc["counts"].items():
            assert sum(1 for g in got if g is not None and g.startswith(prefix)) == cnt
