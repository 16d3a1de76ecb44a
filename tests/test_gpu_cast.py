"""GPU parity of dq_cast_column (cast.hip + dq_parse.h) against the oracle's restatements of Spark 2.2's
Cast(string -> long) (UTF8String.toLong) and Cast(string -> double) (java.lang.Double.parseDouble, whose
correctly rounded value is Python's float() of the same digits). Bar: bit-exact values and identical
NULLs. Strings with more than 19 significant digits match where the reference says the device can decide them and
fail loudly (DQ_ERR_UNSUPPORTED) where it says it cannot; the hard cases (ties, near-midpoints, edges) come from
tests/number_text_cases.py."""
import numpy as np
import pytest
import torch

from deequ_amd import engine
from deequ_amd import native as N
from deequ_amd.native import NativeError
from deequ_amd.table import Table, unpack_validity
import number_text_cases as C
from number_text_cases import random_numeric_strings
import oracle as O

pytestmark = pytest.mark.gpu


def gpu_cast(strings, to_type, device=False):
    valid = [s is not None for s in strings]
    t = Table.from_rows([(s,) for s in strings], ["s"], ["string"])
    if device:
        t.to_device(0)
    n = len(strings)
    vals = torch.empty(max(n, 1), dtype=torch.float64 if to_type == N.TYPE_DOUBLE else torch.int64, device="cuda")
    mask = torch.zeros(max((n + 63) // 64, 1) * 8, dtype=torch.uint8, device="cuda")
    engine.ctx().cast_column(t["s"].native(), n, to_type, vals.data_ptr(), mask.data_ptr())
    ok = unpack_validity(mask.cpu().numpy(), n)
    return vals.cpu().numpy()[:n], ok, valid


def test_cast_to_long_matches_spark():
    rng = np.random.default_rng(1)
    strings = random_numeric_strings(rng, 50_000) + [None, "123", None]
    strings = [s for s in strings if s != "0x1p3"]
    vals, ok, valid = gpu_cast(strings, N.TYPE_LONG)
    for i, s in enumerate(strings):
        exp = O.spark_string_to_long(s) if s is not None else None
        assert bool(ok[i]) == (exp is not None), (s, exp)
        if exp is not None:
            assert int(vals[i]) == exp, (s, exp, int(vals[i]))


@pytest.mark.parametrize("device", [False, True])
def test_cast_to_double_matches_java(device):
    rng = np.random.default_rng(2 + device)
    strings = random_numeric_strings(rng, 60_000) + [None, "2.5", None]
    strings = [s for s in strings if s != "0x1p3"]
    vals, ok, valid = gpu_cast(strings, N.TYPE_DOUBLE, device=device)
    bad = []
    for i, s in enumerate(strings):
        exp = O.java_parse_double(s) if s is not None else None
        if bool(ok[i]) != (exp is not None):
            bad.append((s, exp, ok[i]))
            continue
        if exp is not None:
            a, b = np.float64(vals[i]), np.float64(exp)
            if not (np.isnan(a) and np.isnan(b)) and a.view(np.uint64) != b.view(np.uint64):
                bad.append((s, exp, float(a)))
    assert not bad, bad[:10]


def _assert_bit_exact(texts, expected, vals, ok):
    bad = []
    for i, (s, exp) in enumerate(zip(texts, expected)):
        if bool(ok[i]) != (exp is not None):
            bad.append((s, exp, bool(ok[i])))
        elif exp is not None and not C.same_double(float(vals[i]), exp):
            bad.append((s, exp, float(vals[i])))
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("device", [False, True])
def test_cast_hard_cases_bit_exact(device):
    """Every hard <= 19-digit case of tests/number_text_cases.py in one call: repr / %.17g of doubles of every binade
    (subnormals, the lowest and highest binades), 17 / 18 / 19-digit truncations just below and just above the
    midpoint of adjacent doubles, exact ties (the round-half-to-even branch of el_compute_float), Clinger's
    multiplications and divisions, and the subnormal / overflow edges. The call must succeed; validity and bits equal
    Python's correctly rounded float() for every row, and every tie also equals the even neighbour it has by
    construction. tests/test_number_text_host.py shows the host build of the same header passes all of them, so a
    failure here is the device build's (__umul64hi, __clzll, the __constant__ table, the fp64 division)."""
    cases = C.parse_hard_cases(101) + [C.ParseCase(None, None, None)]
    texts = [c.text for c in cases]
    vals, ok, _ = gpu_cast(texts, N.TYPE_DOUBLE, device=device)
    _assert_bit_exact(texts, [c.expected for c in cases], vals, ok)
    ties = [(c, float(vals[i])) for i, c in enumerate(cases) if c.tie is not None]
    assert len(ties) >= 300
    bad = [(c, v) for c, v in ties if not C.same_double(v, c.tie)]
    assert not bad, (len(bad), bad[:10])


def test_cast_long_significands_match_or_fail_loudly():
    """Strings of 20 to 40 significant digits, labelled by the reference alone (tests/number_text_cases.py): where the
    first 19 digits w and w + 1 round alike (`decidable`) the call succeeds with Java's bits for every row; a string
    on a rounding boundary (the exact decimal expansions of midpoints, also with a late digit changed) or a well-formed
    hexadecimal literal fails the call loudly, all in one call and one per call; a malformed hexadecimal literal is
    NULL without an error."""
    cases = C.parse_long_cases(102)
    decidable = [c for c in cases if c.label == "decidable"]
    boundary = [c for c in cases if c.label == "boundary"]
    null = [c for c in cases if c.label == "null"]
    assert len(decidable) >= 500 and len(boundary) >= 50 and len(null) == 3
    texts = [c.text for c in decidable]
    vals, ok, _ = gpu_cast(texts, N.TYPE_DOUBLE)
    _assert_bit_exact(texts, [c.expected for c in decidable], vals, ok)
    with pytest.raises(NativeError):
        gpu_cast([c.text for c in boundary], N.TYPE_DOUBLE)
    hexes = [c for c in boundary if "x" in c.text.lower()]
    assert len(hexes) == 3
    for c in boundary[::max(1, len(boundary) // 17)] + hexes:
        with pytest.raises(NativeError):
            gpu_cast(["1.5", c.text, "2"], N.TYPE_DOUBLE)
    vals, ok, _ = gpu_cast([c.text for c in null] + ["1.5"], N.TYPE_DOUBLE)
    assert list(ok) == [False, False, False, True] and vals[3] == 1.5


def test_cast_empty_and_all_null():
    vals, ok, _ = gpu_cast([], N.TYPE_LONG)
    assert len(vals) == 0
    vals, ok, _ = gpu_cast([None] * 100, N.TYPE_DOUBLE)
    assert not ok.any()


@pytest.mark.parametrize("to_type", [N.TYPE_LONG, N.TYPE_DOUBLE])
@pytest.mark.parametrize("device", [False, True])
def test_short_numbers_fast_path_matches_the_parsers(to_type, device, monkeypatch):
    """Strings of <= 15 bytes are parsed by one branch-free DFA step per byte ([+|-] digits [. digits]; cast.hip
    cast_short_number): every form of that grammar at every length up to 15 (and the near misses around it: lone signs
    and points, second points, inner signs, spaces, exponents, letters, 16-byte numbers) equals the oracle's
    UTF8String.toLong / Double.parseDouble and the general device parsers (DQ_CAST_NO_SHORT=1), bit for bit."""
    rng = np.random.default_rng(40 + device + 2 * (to_type == N.TYPE_DOUBLE))
    strings = ["", ".", "+", "-", "+.", "-.", "-.5", ".5", "1.", "00", "-0", "-0.000", "+0", "0.", "1.2.3", "1-2", "+-1",
               " 1", "1 ", "1e5", "1d", "NaN", "a", "999999999999999", "-99999999999999", "9999999.9999999",
               "0.000000000001", "1234567890123456", "-123456789012345", "1.23456789012345", "..1", "1..", "-",
               None]
    for _ in range(30_000):
        nd = int(rng.integers(0, 15))
        digits = "".join(str(d) for d in rng.integers(0, 10, nd))
        p = int(rng.integers(0, nd + 1))
        form = int(rng.integers(0, 4))
        s = digits if form == 0 else digits[:p] + "." + digits[p:] if form == 1 else \
            ["-", "+"][int(rng.integers(0, 2))] + (digits[:p] + "." + digits[p:] if rng.random() < 0.5 else digits)
        if form == 3 and s:  # a near miss: one byte replaced
            i = int(rng.integers(0, len(s)))
            s = s[:i] + ["x", " ", "e", "-", "."][int(rng.integers(0, 5))] + s[i + 1:]
        strings.append(s[:16])
    strings += ["%d" % v for v in rng.integers(-1_000_000, 1_000_000, 2000)]  # the C5 generators' forms
    strings += ["%d.%02d" % (v // 100, v % 100) for v in rng.integers(0, 100_000, 2000)]
    strings += ["%s%d.%03d" % ("-" if v < 0 else "", abs(v) // 1000, abs(v) % 1000)
                for v in rng.integers(-999_999, 999_999, 2000)]
    fast, ok_f, _ = gpu_cast(strings, to_type, device=device)
    monkeypatch.setenv("DQ_CAST_NO_SHORT", "1")
    slow, ok_s, _ = gpu_cast(strings, to_type, device=device)
    assert np.array_equal(ok_f, ok_s)
    assert np.array_equal(fast[ok_f].view(np.uint64), slow[ok_s].view(np.uint64))
    for i, s in enumerate(strings):
        exp = None if s is None else (O.spark_string_to_long(s) if to_type == N.TYPE_LONG else O.java_parse_double(s))
        assert bool(ok_f[i]) == (exp is not None), (s, exp)
        if exp is not None and to_type == N.TYPE_LONG:
            assert int(fast[i]) == exp, (s, exp)
        elif exp is not None and not np.isnan(exp):
            assert np.float64(fast[i]).view(np.uint64) == np.float64(exp).view(np.uint64), (s, exp, fast[i])
