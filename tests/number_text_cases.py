"""Shared by the number <-> text tests (tests/test_number_text_host.py on the CPU; tests/test_gpu_cast.py and
tests/test_gpu_number_text.py on the device): the hard cases of Double.parseDouble, Double.toString and
Float.toString, deterministic from a seed.

Expectations come from the reference alone, never from the code under test: a parsed value is Python's correctly
rounded float() of the digits (oracle.java_parse_double); an exact tie additionally carries the value that round
half to even gives by construction (from the parity of its lower neighbour's significand), independent of float();
formatted text is oracle.java_double_to_string (the shortest round-trip digits in Java's layout; Java 8's documented
non-shortest outputs, JDK-4511638, stay unpinned there)."""
import math
import struct
from collections import namedtuple
from fractions import Fraction

import numpy as np

import oracle as O

# text: the string; expected: Java's value (None where Java throws); tie: the by-construction value of an exact tie
ParseCase = namedtuple("ParseCase", "text expected tie")
# label: "decidable" (w and w + 1 round alike: the device must give Java's value), "boundary" (the device must
# refuse: `slow`) or "null" (not a number); expected: Java's value (None for "null")
LongCase = namedtuple("LongCase", "text label expected")


def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_double(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def same_double(a, b):
    """Bit equality, any NaN equal to any NaN."""
    return (a != a and b != b) or double_bits(a) == double_bits(b)


def random_numeric_strings(rng, n, max_digits=19):
    """Random numeric-looking strings in the forms Cast(string -> long / double) meets, and near misses."""
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 6))
        nd = int(rng.integers(1, max_digits + 1))
        digits = "".join(str(d) for d in rng.integers(0, 10, nd))
        sign = ["", "-", "+", "- ", " "][int(rng.integers(0, 5))]
        if k == 0:
            s = sign + digits
        elif k == 1:
            p = int(rng.integers(0, nd + 1))
            s = sign + digits[:p] + "." + digits[p:]
        elif k == 2:
            s = sign + digits[:1] + "." + digits[1:] + "e" + str(int(rng.integers(-330, 320)))
        elif k == 3:
            s = sign + "0." + "0" * int(rng.integers(0, 30)) + digits
        elif k == 4:
            s = sign + digits + ["d", "f", "D", "x", "", "\n", "  "][int(rng.integers(0, 7))]
        else:
            s = ["", ".", "-", "+", "NaN", "-Infinity", "Infinity", "1e", "e5", "--1", "1.2.3", " 42 ", "\t7\n",
                 "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809",
                 "1.", ".5", "-.5", "+.", "0.1e-5", "1E+3", "4.9e-324", "2.4703282292062328e-324",
                 "1.7976931348623157e308", "1.7976931348623159e308", "0x1p3", "007"][int(rng.integers(0, 29))]
        out.append(s)
    return out


def _random_positive_doubles(rng, n):
    """Finite positive doubles: subnormals, the lowest three and highest four binades, and the middle."""
    out = []
    for i in range(n):
        kind = i % 8
        if kind == 0:
            e = 0
        elif kind == 1:
            e = int(rng.integers(1, 4))
        elif kind == 2:
            e = int(rng.integers(2043, 2047))
        else:
            e = int(rng.integers(1, 2047))
        m = int(rng.integers(0, 1 << 52))
        if e == 0 and m == 0:
            m = 1
        out.append(bits_double((e << 52) | m))
    return out


def _truncate(f, k):
    """(d, e): d = floor(f / 10^e) with exactly k decimal digits, for a Fraction f > 0."""
    e = len(str(f.numerator)) - len(str(f.denominator)) - k
    while True:
        d = f.numerator // (f.denominator * 10 ** e) if e >= 0 else f.numerator * 10 ** -e // f.denominator
        if d >= 10 ** k:
            e += 1
        elif d < 10 ** (k - 1):
            e -= 1
        else:
            return d, e


def _exact_decimal(n, e2):
    """The exact decimal text of n * 2^e2 (n > 0), without an exponent and without trailing fraction zeros."""
    if e2 >= 0:
        return str(n << e2)
    s = str(n * 5 ** -e2).rjust(1 - e2, "0")
    whole, frac = s[:e2], s[e2:].rstrip("0")
    return whole + ("." + frac if frac else "")


def significant_digits(text):
    """Number of significant decimal digits of a plain or exponent literal (leading zeros do not count; zeros after
    the first non-zero digit do, as the device parser counts them)."""
    mant = text.lower().lstrip("+- ").split("e")[0].rstrip("dDfF")
    return len(mant.replace(".", "").lstrip("0"))


def _case(text, tie=None):
    return ParseCase(text, O.java_parse_double(text), tie)


EDGES = ["9007199254740993", "9007199254740992", "9007199254740995",
         "2.2250738585072011e-308", "2.2250738585072012e-308", "2.2250738585072014e-308",
         "4.9406564584124654e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
         "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "17976931348623158e292",
         "1e-342", "1e-343", "9e-343", "123456789012345678e-360",
         "1e400", "1e-400", "0e999999999999"]


def parse_hard_cases(seed):
    """Strings of at most 19 significant digits (the device converts every one of them exactly)."""
    rng = np.random.default_rng(seed)
    cases = []
    xs = _random_positive_doubles(rng, 240)
    for x in xs:
        cases.append(_case(repr(x)))
        cases.append(_case("%.17g" % x))
    # just below and just above the midpoint of adjacent doubles, at 17 / 18 / 19 digits
    for x in xs:
        y = bits_double(double_bits(x) + 1)
        if math.isinf(y):
            continue
        mid = (Fraction(x) + Fraction(y)) / 2
        for k in (17, 18, 19):
            d, e = _truncate(mid, k)
            for dd in (d, d + 1):
                if len(str(dd)) < 20:
                    cases.append(_case("%de%d" % (dd, e)))
    # exact ties (2m + 1) / 2 * 2^e between m * 2^e and (m + 1) * 2^e: round half to even picks the even one
    for e in range(-5, 12):
        kept = 0
        for _ in range(400):
            if kept >= 24:
                break
            # smaller significands at the negative exponents, where only they stay within 19 digits
            hi = (1 << 53) if e >= -1 else (1 << 52) + (1 << 49)
            m = int(rng.integers(1 << 52, hi))
            text = _exact_decimal(2 * m + 1, e - 1)
            if significant_digits(text) > 19:
                continue
            cases.append(_case(text, tie=math.ldexp(m if m % 2 == 0 else m + 1, e)))
            kept += 1
    # ties written with a decimal exponent: w * 10^q with w * 5^q = 2m + 1 of exactly 54 bits (1e23 is the first),
    # as they are (Clinger's exact multiplication up to q = 22) and padded to 19 digits (the Eisel-Lemire tie branch)
    for q in range(1, 24):
        p5 = 5 ** q
        lo, hi = -(-(1 << 53) // p5), ((1 << 54) - 1) // p5
        ws = {w for w in (int(v) for v in rng.integers(lo, hi + 1, 12)) if w % 2 == 1}
        ws |= {w for w in (lo, lo + 1, hi - 1, hi) if w % 2 == 1 and lo <= w <= hi}
        for w in sorted(ws):
            m = (w * p5 - 1) // 2
            tie = math.ldexp(m if m % 2 == 0 else m + 1, q + 1)
            cases.append(_case("%de%d" % (w, q), tie=tie))
            pad = 19 - len(str(w))
            cases.append(_case("%d%se%d" % (w, "0" * pad, q - pad), tie=tie))
    # Clinger's fast path: one IEEE multiplication or division of two exact doubles
    for _ in range(400):
        w = int(rng.integers(1, (1 << 53) + 1)) if rng.random() < 0.7 else int(rng.integers(1, 100000))
        q = int(rng.integers(1, 23)) * (1 if rng.random() < 0.4 else -1)
        cases.append(_case("%de%d" % (w, q)))
    cases += [_case("%de%d" % (1 << 53, q)) for q in (-22, -1, 1, 22)]
    # just outside its conditions: 10^23 is not an exact double, nor is every w above 2^53
    for _ in range(240):
        if rng.random() < 0.5:
            w, q = int(rng.integers(1, (1 << 53) + 1)), int(rng.choice([23, 24, -23, -24]))
        else:
            w, q = int(rng.integers((1 << 53) + 1, 1 << 55)), int(rng.integers(1, 23)) * (1 if rng.random() < 0.5 else -1)
        cases.append(_case("%de%d" % (w, q)))
    cases += [_case(s) for s in EDGES]
    # sign, String.trim and the type suffix around a random subset
    for c in [cases[i] for i in np.flatnonzero(rng.random(len(cases)) < 0.3)]:
        form = int(rng.integers(0, 3))
        if form == 0:
            cases.append(ParseCase("-" + c.text, -c.expected, None if c.tie is None else -c.tie))
        else:
            cases.append(ParseCase(" " + c.text if form == 1 else c.text + "d", c.expected, c.tie))
    for c in cases:
        assert c.expected is not None and significant_digits(c.text) <= 19, c
    return cases


def _label(text):
    """decidable iff the first 19 significant digits w (with the exponent q that goes with them) and w + 1 round to
    the same double: the reference alone decides."""
    t = text.strip().lower().lstrip("+-").rstrip("df")
    mant, _, ex = t.partition("e")
    whole, _, frac = mant.partition(".")
    digits = whole + frac
    lead = len(digits) - len(digits.lstrip("0"))
    sig = digits[lead:]
    assert len(sig) >= 20 and sig[19:].strip("0"), text
    q = (int(ex) if ex else 0) - len(frac) + (len(sig) - 19)
    w = int(sig[:19])
    return "decidable" if same_double(float("%de%d" % (w, q)), float("%de%d" % (w + 1, q))) else "boundary"


def parse_long_cases(seed):
    """Strings of 20 to 40 significant digits, labelled by the reference, and hexadecimal literals."""
    rng = np.random.default_rng(seed)
    texts = []
    for _ in range(1500):
        nd = int(rng.integers(20, 41))
        d = "".join(str(v) for v in rng.integers(0, 10, nd))
        d = str(int(rng.integers(1, 10))) + d[1:-1] + str(int(rng.integers(1, 10)))
        form = int(rng.integers(0, 4))
        sign = ["", "-", "+", " "][int(rng.integers(0, 4))]
        if form == 0:
            s = d
        elif form == 1:
            p = int(rng.integers(0, nd + 1))
            s = d[:p] + "." + d[p:]
        elif form == 2:
            s = d[:1] + "." + d[1:] + "e" + str(int(rng.integers(-340, 312)))
        else:
            s = "0." + "0" * int(rng.integers(0, 30)) + d
        texts.append(sign + s + ("d" if rng.random() < 0.1 else ""))
    # the exact decimal expansions of midpoints of adjacent doubles, and the same with one late digit changed
    mids = []
    while len(mids) < 160:
        m = int(rng.integers(1 << 52, 1 << 53))
        e2 = int(rng.integers(-32, 76))
        s = _exact_decimal(2 * m + 1, e2 - 1)
        n = significant_digits(s)
        if not 20 <= n <= 40:
            continue
        mids.append(s)
        if n > 26:
            pos = [i for i, ch in enumerate(s) if ch != "."][int(rng.integers(25, n))]
            ch = str((int(s[pos]) + int(rng.integers(1, 9))) % 10)
            if pos == len(s) - 1 and ch == "0":
                ch = "7"
            mids.append(s[:pos] + ch + s[pos + 1:])
    for s in mids:
        assert _label(s) == "boundary", s
    texts += mids
    cases = [LongCase(s, _label(s), O.java_parse_double(s)) for s in texts]
    for c in cases:
        assert c.expected is not None and 20 <= significant_digits(c.text) <= 40, c
    # well-formed hexadecimal literals are not converted on the device; malformed ones are not numbers
    cases += [LongCase("0x1p3", "boundary", 8.0), LongCase("0x1.8p1d", "boundary", 3.0),
              LongCase("0X.8P-1", "boundary", 0.25)]
    cases += [LongCase(s, "null", None) for s in ("0x", "0x1", "0x1pz")]
    return cases


def _float_from_bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def _short_bound_neighbours(rng, bits, max_exp):
    """The two neighbours of (2m + 1) * 2^j where 2m + 1 = D * 5^k has bits + 1 bits and j >= k - 1: the bound
    between them is the short decimal D * 2^(j + 1 - k) * 10^k, which the shortest digits of the neighbour with the
    even significand may use and those of the odd one must not (Ryu's vmTrailingZeros and its vp adjustment)."""
    out = []
    lo, hi = 1 << bits, 1 << (bits + 1)
    for k in range(1, 40):
        p5 = 5 ** k
        if p5 >= hi:
            break
        first, last = -(-lo // p5), (hi - 1) // p5
        ds = {d for d in (int(v) for v in rng.integers(first, last + 1, 8)) if d % 2 == 1}
        ds |= {d for d in (first, first + 1, last - 1, last) if d % 2 == 1 and first <= d <= last}
        for d in sorted(ds):
            n = d * p5
            for j in sorted({k - 1, k, k + 2, 2 * k, 3 * k + 1}):
                if j + 1 + bits <= max_exp:
                    out += [math.ldexp(float((n - 1) // 2), j + 1), math.ldexp(float((n + 1) // 2), j + 1)]
    return out


def format_special_values():
    """NaN, the infinities and the zeros (their text is pinned by exact patterns, not by histograms)."""
    return [float("nan"), float("inf"), float("-inf"), 0.0, -0.0]


def format_cases(seed):
    """(doubles, floats): finite non-zero values of every class where Ryu or Java's layout takes another path."""
    rng = np.random.default_rng(seed)

    def signed(v):
        return -v if rng.random() < 0.3 else v

    d = []
    for _ in range(2400):  # random bit patterns over every binade
        d.append(signed(bits_double((int(rng.integers(1, 2047)) << 52) | int(rng.integers(0, 1 << 52)))))
    for _ in range(120):  # subnormals
        d.append(signed(bits_double(int(rng.integers(1, 1 << 52)) >> int(rng.integers(0, 52)) or 1)))
    for k in range(-30, 31):
        x = float("1e%d" % k)
        d += [x, bits_double(double_bits(x) - 1), bits_double(double_bits(x) + 1)]
    d += [math.ldexp(1.0, k) for k in range(-1074, 1024, 3)] + [math.ldexp(1.0, 1023)]
    d += [int(n) / 8.0 for n in rng.integers(-10 ** 7 + 1, 10 ** 7, 900) if n != 0]
    for j in range(1, 23):  # integers that are multiples of 5^j: Ryu's trailing-zero bookkeeping with e2 >= 0
        for _ in range(20):
            d.append(float(int(rng.integers(1, (1 << 53) // 5 ** j + 1)) * 5 ** j))
        d.append(float(5 ** j))
    for _ in range(400):  # few digits ending in 5, scaled: the exact-half (round half to even) branch
        n = int(rng.integers(0, 2000)) * 10 + 5
        d.append(signed(math.ldexp(float(n), int(rng.integers(-30, 60)))))
        d.append(signed(float("%de%d" % (n, int(rng.integers(-12, 22))))))
    d += _short_bound_neighbours(rng, 53, 1023)
    for x in (1e-3, 1e7):
        d += [x, bits_double(double_bits(x) - 1), -x, -bits_double(double_bits(x) - 1)]
    d += [5e-324, 2.2250738585072014e-308, bits_double(double_bits(2.2250738585072014e-308) - 1),
          1.7976931348623157e308]
    while len(d) < 6000 or len(d) % 64 == 0:
        d.append(signed(float(rng.standard_normal()) * 10.0 ** int(rng.integers(-10, 10))))
    doubles = np.array(d, dtype=np.float64)

    f = []
    for _ in range(2400):
        f.append(signed(_float_from_bits((int(rng.integers(1, 255)) << 23) | int(rng.integers(0, 1 << 23)))))
    for _ in range(120):
        f.append(signed(_float_from_bits(int(rng.integers(1, 1 << 23)) >> int(rng.integers(0, 23)) or 1)))
    for k in range(-30, 31):
        u = int(np.array([float("1e%d" % k)], dtype=np.float32).view(np.uint32)[0])
        f += [_float_from_bits(u), _float_from_bits(u - 1), _float_from_bits(u + 1)]
    f += [np.float32(math.ldexp(1.0, k)) for k in range(-149, 128)]
    f += [np.float32(int(n) / 8.0) for n in rng.integers(-10 ** 7 + 1, 10 ** 7, 900) if n != 0]
    for j in range(1, 11):
        for _ in range(30):
            v = int(rng.integers(1, (1 << 24) // 5 ** j + 1)) * 5 ** j
            f.append(np.float32(math.ldexp(float(v), int(rng.integers(0, 40)))))
        f.append(np.float32(5 ** j))
    for _ in range(400):
        n = int(rng.integers(0, 2000)) * 10 + 5
        f.append(signed(np.float32(math.ldexp(float(n), int(rng.integers(-30, 60))))))
        f.append(signed(np.float32(float("%de%d" % (n, int(rng.integers(-12, 22)))))))
    f += [np.float32(v) for v in _short_bound_neighbours(rng, 24, 127)]
    for u in (0x3a83126f, 0x4b189680):  # 1e-3f and 1e7f, their predecessors, and the negatives
        f += [_float_from_bits(u), _float_from_bits(u - 1), -_float_from_bits(u), -_float_from_bits(u - 1)]
    f += [_float_from_bits(u) for u in (0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff)]
    while len(f) < 6000 or len(f) % 64 == 0:
        f.append(signed(np.float32(float(rng.standard_normal()) * 10.0 ** int(rng.integers(-10, 10)))))
    floats = np.array(f, dtype=np.float32)
    for a in (doubles, floats):
        assert np.isfinite(a).all() and (a != 0).all() and len(a) % 64 != 0
    return doubles, floats


def oracle_texts(doubles, floats):
    return ([O.java_double_to_string(float(v)) for v in doubles],
            [O.java_double_to_string(float(v), is_float=True) for v in floats])
