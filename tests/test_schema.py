"""Row-level schema validation without a GPU: the Python model against the reference's test cases, the schema
builder and mask compiler, libdq's host parser entries fuzzed against the model (identical class and value bits), and
the parsers under ASan + UBSan in a stand-alone program."""
import os
import random
import shutil
import subprocess

import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd.regex import RegexUnsupported
from deequ_amd.schema import compile_mask
from deequ_amd.table import Table

import schema_model as M
from schema_cases import build_schema, check_kat_members, load_kats  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", load_kats(), ids=lambda c: c["name"])
def test_model_reproduces_reference_cases(case):
    r = M.validate(case["columns"], case["rows"], case["schema"])
    assert (len(r.valid), len(r.invalid)) == (case["numValid"], case["numInvalid"])
    assert r.num_ambiguous == 0 and r.num_unknown == 0
    check_kat_members(case, r.valid, r.invalid)


# ---- schema builder and mask compiler -------------------------------------------------------------------------------
def test_schema_is_immutable_and_ordered():
    s0 = D.RowLevelSchema()
    s1 = s0.withIntColumn("a")
    s2 = s1.withStringColumn("b", matches="^x+$").withDecimalColumn("c", 10, 2).withTimestampColumn("d", "yyyy-MM-dd")
    assert len(s0.columnDefinitions) == 0 and len(s1.columnDefinitions) == 1
    assert [d.name for d in s2.columnDefinitions] == ["a", "b", "c", "d"]


ACCEPTED_MASKS = ["yyyy-MM-dd HH:mm:ss", "dd/MM/yyyy", "yyyy-MM-dd'T'HH:mm:ss", "HH:mm", "ss.mm 'o''clock' HH", "yyyy",
                  "'at' HH''mm", "[dd] (MM)"]


@pytest.mark.parametrize("mask", ACCEPTED_MASKS)
def test_mask_compiler_accepts(mask):
    prog = compile_mask(mask)
    want = bytearray()
    for kind, arg in M.mask_elements(mask):
        want += bytes([0, arg]) if kind == "lit" else bytes([{"yyyy": 1, "MM": 2, "dd": 3, "HH": 4, "mm": 5, "ss": 6}[arg]])
    assert prog == bytes(want)


@pytest.mark.parametrize("mask", ["yyyy-MM-dd hh:mm", "yyyy-MM-dd HH:mm:ss.SSS", "yy-MM-dd", "yyyy-M-dd", "yyyy-MMM-dd",
                                  "yyyyMMdd", "HHmm", "yyyy-MM-dd yyyy", "yyyy-MM-dd 'T", "yyyy-MM-dd Z", "yyyy-MM-dd G",
                                  "yyyyéMM", "yyyy''''MM'"])
def test_mask_compiler_rejects(mask):
    with pytest.raises(ValueError):
        compile_mask(mask)
    with pytest.raises(ValueError):
        D.RowLevelSchema().withTimestampColumn("t", mask)


def test_schema_builder_rejects_bad_parameters():
    with pytest.raises(ValueError):
        D.RowLevelSchema().withDecimalColumn("a", 19, 2)
    with pytest.raises(ValueError):
        D.RowLevelSchema().withDecimalColumn("a", 5, 6)
    with pytest.raises(ValueError):
        D.RowLevelSchema().withDecimalColumn("a", 5, -1)
    with pytest.raises(ValueError):
        D.RowLevelSchema().withIntColumn("a", minValue=-(1 << 31) - 1)
    with pytest.raises(ValueError):
        D.RowLevelSchema().withIntColumn("a", maxValue=1 << 31)
    with pytest.raises(RegexUnsupported):
        D.RowLevelSchema().withStringColumn("a", matches="(a)(b)(c)(d)(e)(f)(g)(h)(i)(j)")


def test_validate_rejects_missing_and_non_string_columns_before_any_gpu_work():
    t = Table.from_pydict({"s": ["1", None], "n": [1, 2]})
    with pytest.raises(ValueError, match="not in the table"):
        D.RowLevelSchemaValidator.validate(t, D.RowLevelSchema().withIntColumn("missing"))
    with pytest.raises(ValueError, match="STRING"):
        D.RowLevelSchemaValidator.validate(t, D.RowLevelSchema().withIntColumn("n"))
    with pytest.raises(ValueError):
        D.RowLevelSchemaValidator.validate(t, D.RowLevelSchema().withIntColumn("s"), ambiguous="guess")


# ---- fuzz of the host parser entries against the model --------------------------------------------------------------
def _digits(rng, lo, hi, lead_zero=0.2):
    n = rng.randint(lo, hi)
    s = "".join(rng.choice("0123456789") for _ in range(n))
    if s and rng.random() < lead_zero:
        s = "0" * rng.randint(1, 4) + s
    return s


SPECIAL_NUMBERS = ["", "+", "-", ".", "1.", ".5", "-.5", "+.5", "e5", "1e", "1e+", "1e-", ".e5", "1.e5", " 1", "1 ", "1\t",
                   "\t1", "1\n", "NaN", "Infinity", "-Infinity", "é", "１", "1１", "１.5", "0", "-0", "+0.0",
                   "000", "0.000", "0e10001", "0e10000", "1e10000", "1e-10000", "1e10001", "1e-10001", "1E+10000",
                   "1E+10001", "-5e-10001", "00012.50", "1e00005", "1e000010001", "--1", "+-1", "1.2.3", "1e5.0", "0x10",
                   "1d", "1f", "1L", "1,000", "1_000", "1e5e5", "\x001", "1\x00", "2147483647", "2147483648",
                   "-2147483648", "-2147483649", "2147483647.999", "-2147483648.5", "9223372036854775807",
                   "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "+2147483647", "+2147483648",
                   "4294967296", "99999999999999999999", "1.9", "-1.9", "12.x", "12.5x", "１２"]


def random_number_string(rng):
    k = rng.random()
    if k < 0.12:
        return rng.choice(SPECIAL_NUMBERS)
    sign = rng.choice(["", "", "+", "-"])
    ip = _digits(rng, 0, rng.choice([3, 6, 10, 19, 40]))
    out = sign + ip
    if rng.random() < 0.6:
        out += "." + _digits(rng, 0, rng.choice([0, 2, 3, 6, 19, 40]), lead_zero=0.1)
    if rng.random() < 0.3:
        e = rng.choice([rng.randint(-25, 25), rng.randint(-45, 45), 10000, -10000, 10001, -10001, 9999, 100000])
        out += rng.choice("eE") + rng.choice(["", "+"] if e >= 0 else [""]) + str(e)
    if rng.random() < 0.06:  # one mutation: a stray byte somewhere
        pos = rng.randint(0, len(out))
        out = out[:pos] + rng.choice([" ", "\t", "x", "-", "+", ".", "e", "é", "５", ","]) + out[pos:]
    return out


def test_fuzz_parse_int32_matches_model():
    rng = random.Random(20240601)
    cells = list(SPECIAL_NUMBERS)
    for _ in range(50000):
        if rng.random() < 0.3:  # around the int32 / int64 edges
            base = rng.choice([(1 << 31) - 1, -(1 << 31), (1 << 63) - 1, -(1 << 63), 0, 10 ** 9])
            cells.append(rng.choice(["", "+", ""]) + str(base + rng.randint(-3, 3)) + rng.choice(["", "", ".", ".0", ".99"]))
        else:
            cells.append(random_number_string(rng))
    seen = set()
    for c in cells:
        want = M.cast_int(c)
        got = N.parse_int32(c.encode("utf-8"))
        assert got == want, (c, got, want)
        seen.add(want[0])
    assert seen == {M.VALUE, M.NULL}


DECIMAL_TYPES = [(10, 2), (18, 0), (18, 18), (5, 5), (1, 0), (4, 2), (18, 6), (9, 3), (2, 1)]


def test_fuzz_parse_decimal_matches_model():
    rng = random.Random(20240602)
    items = [(c, p, s) for c in SPECIAL_NUMBERS for p, s in [(10, 2), (18, 0), (5, 5)]]
    for _ in range(50000):
        p, s = rng.choice(DECIMAL_TYPES)
        k = rng.random()
        if k < 0.15:  # a tie (or its neighbours) at digit s + 1
            c = rng.choice(["", "-", "+"]) + _digits(rng, 0, max(p - s, 0)) + "." + _digits(rng, s, s, 0) + \
                rng.choice("4569") + _digits(rng, 0, 5, 0)
        elif k < 0.3:  # +-(10^p - 1) and +-10^p at scale s, as plain digits or shifted by an exponent
            u = rng.choice([10 ** p - 1, 10 ** p, 10 ** p - 1, 10 ** (p - 1)])
            txt = str(u).rjust(s + 1, "0")
            c = txt[:len(txt) - s] + ("." + txt[len(txt) - s:] if s else "")
            if rng.random() < 0.4:
                c += rng.choice(["4", "5", "49", "50", "9"]) if s else rng.choice([".4", ".5", ".49", ".50"])
            if rng.random() < 0.3:
                sh = rng.randint(-6, 6)
                c = c + "e%d" % sh  # the value moves: the model decides
            c = rng.choice(["", "-", "+"]) + c
        else:
            c = random_number_string(rng)
        items.append((c, p, s))
    seen = set()
    for c, p, s in items:
        want = M.cast_decimal(c, p, s)
        got = N.parse_decimal(c.encode("utf-8"), p, s)
        assert got == want, (c, p, s, got, want)
        seen.add(want[0])
    assert seen == {M.VALUE, M.NULL, M.AMBIGUOUS}


FUZZ_MASKS = ["yyyy-MM-dd HH:mm:ss", "dd/MM/yyyy", "yyyy-MM-dd'T'HH:mm:ss", "HH:mm", "ss.mm 'o''clock' HH", "yyyy",
              "MM-dd"]


def format_cell(mask, y, mo, d, h, mi, s):
    vals = {"yyyy": "%04d" % y, "MM": "%02d" % mo, "dd": "%02d" % d, "HH": "%02d" % h, "mm": "%02d" % mi, "ss": "%02d" % s}
    return "".join(chr(arg) if kind == "lit" else vals[arg] for kind, arg in M.mask_elements(mask))


def random_timestamp_cell(rng, mask):
    y = rng.choice([rng.randint(1583, 9999), rng.randint(1583, 9999), 1583, 9999, 1900, 2000, 2024, 1970, 1969])
    mo = rng.randint(1, 12)
    d = rng.randint(1, 28)
    k = rng.random()
    if k < 0.1:
        y, mo, d = rng.choice([1900, 2000, 2024, 2023, 2100, 2400]), 2, 29
    elif k < 0.2:
        mo, d = rng.choice([4, 6, 9, 11, 1, 3, 12]), 31
    elif k < 0.25:
        y = rng.choice([1582, 1, 0, 999, 1500])
    elif k < 0.3:
        mo, d = rng.choice([(0, 1), (13, 1), (1, 0), (1, 32), (2, 30)])
    h, mi, s = rng.randint(0, 23), rng.randint(0, 59), rng.randint(0, 59)
    if rng.random() < 0.06:
        h, mi, s = rng.choice([(24, 0, 0), (23, 60, 0), (23, 59, 60), (99, 99, 99)])
    c = format_cell(mask, y, mo, d, h, mi, s)
    k = rng.random()
    if k < 0.5 or not c:
        return c
    pos = rng.randint(0, len(c))
    if k < 0.56:
        return c[:pos] + c[pos + 1:]                      # a dropped character (digit or literal)
    if k < 0.62:
        return c[:pos] + rng.choice("0123456789") + c[pos:]  # an extra digit
    if k < 0.70:
        return c[:pos] + rng.choice([" ", "\t", "  "]) + c[pos:]
    if k < 0.75:
        return c[:pos] + "-" + c[pos:]
    if k < 0.80:
        return c + rng.choice(["Z", " UTC", ".123", "E", " "])
    if k < 0.85:
        return c[:pos]                                     # truncated
    if k < 0.90:
        return c[:pos] + rng.choice(["/", "x", ":", "T", "é", "２"]) + c[pos + 1:]  # a wrong character
    if k < 0.95:
        return rng.choice(["2E3", "2e3", "20E1"]) + c[4:]
    return rng.choice(["", "N/A", "yesterday night", "é", "12", "-", " ", "2012-7-22 22:59:59", "2012-07-22"])


def test_fuzz_parse_timestamp_matches_model():
    rng = random.Random(20240603)
    seen = set()
    progs = {m: compile_mask(m) for m in FUZZ_MASKS}
    fixed = [("yyyy-MM-dd HH:mm:ss", c) for c in
             ["2012-07-22 22:59:59", "2012-7-22 22:59:59", "2E3-07-22 22:59:59", "1900-02-29 00:00:00",
              "2000-02-29 23:59:59", "2024-02-29 12:00:00", "2023-04-31 00:00:00", "1583-01-01 00:00:00",
              "9999-12-31 23:59:59", "1582-12-31 00:00:00", "10000-01-01 00:00:00", " 2012-07-22 22:59:59",
              "2012-07-22 22:59:59Z", "2012-07-22  22:59:59", "2012-07-22 -2:59:59", "2012-07-22 22:59", ""]]
    for i in range(50000):
        mask = FUZZ_MASKS[i % len(FUZZ_MASKS)] if i % 3 else "yyyy-MM-dd HH:mm:ss"
        fixed.append((mask, random_timestamp_cell(rng, mask)))
    for mask, c in fixed:
        want = M.cast_timestamp(mask, c)
        got = N.parse_timestamp(progs[mask], c.encode("utf-8"))
        assert got == want, (mask, c, got, want)
        seen.add(want[0])
    assert seen == {M.VALUE, M.NULL, M.AMBIGUOUS}
    assert M.cast_timestamp("yyyy-MM-dd HH:mm:ss", "2012-07-22 22:59:59") == (M.VALUE, 1342997999000000)
    assert M.cast_timestamp("yyyy-MM-dd HH:mm:ss", "1969-12-31 23:59:59") == (M.VALUE, -1000000)


# ---- the parsers under ASan + UBSan: a stand-alone program, run as a child process ------------------------------------
def test_schema_parsers_under_asan_ubsan():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    here = os.path.join(ROOT, "tests", "sanitize_schema")
    out = os.path.join(here, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "schema_checks")
    subprocess.run([cxx, "-std=c++17", "-DDQ_HOST_ONLY", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                    "-I", os.path.join(ROOT, "deequ_amd", "csrc"), "-o", exe, os.path.join(here, "main.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, \
        (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "schema_checks: ok" in p.stdout
