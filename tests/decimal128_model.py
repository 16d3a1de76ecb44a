"""A small exact model of DQ_TYPE_DECIMAL128 (Spark decimals of precision 19..38) on Python int / decimal /
fractions and the xxhash package: what Spark's Decimal.toDouble, Decimal.toLong, XxHash64Function.hash and the
decimal aggregates return for 16-byte unscaled values. The expected values of tests/test_decimal128_host.py and
tests/test_gpu_decimal128.py come from here (the C oracle has no 128-bit type)."""
import decimal
import math
import random
import struct
from fractions import Fraction

import numpy as np

LIMIT = 10 ** 38  # results are defined for |unscaled| < 10^38
SCALES = (0, 1, 18, 22, 23, 37, 38)


def to_double(v, s):
    """The double nearest to v * 10^-s, ties to even (BigDecimal.doubleValue)."""
    with decimal.localcontext() as c:
        c.prec = 60
        return float(decimal.Decimal(v).scaleb(-s))


def to_long(v, s):
    """Decimal.toLong: truncate toward zero, then the low 64 bits as a signed long."""
    q = abs(v) // 10 ** s
    q = -q if v < 0 else q
    q &= (1 << 64) - 1
    return q - (1 << 64) if q >> 63 else q


def java_bytes(v):
    """BigInteger.toByteArray: minimal big-endian two's complement."""
    bl = v.bit_length() if v >= 0 else (~v).bit_length()
    return v.to_bytes(bl // 8 + 1, "big", signed=True)


def spark_hash(v, seed=42):
    import xxhash
    h = xxhash.xxh64_intdigest(java_bytes(v), seed=seed)
    return h - (1 << 64) if h >> 63 else h


def cell(v):
    """The 16-byte little-endian two's-complement cell."""
    return (v & ((1 << 128) - 1)).to_bytes(16, "little")


def cells(values):
    """values (ints, None = NULL -> zero cell) as a (n, 2) uint64 array of (lo, hi) limbs."""
    buf = b"".join(cell(0 if v is None else v) for v in values)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 2).copy()


def bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def hard_values():
    """Unscaled values at the conversion's and the hash's edges: 0, +-1, +-(10^38 - 1), both sides of 2^53, 2^63,
    2^64 and 2^127 (the far side of 2^127 exists for the negative value only), and the byte-length steps."""
    vs = {0, 1, -1, LIMIT - 1, -(LIMIT - 1)}
    for p in (53, 63, 64):
        for d in (-1, 0, 1):
            vs.add((1 << p) + d)
            vs.add(-((1 << p) + d))
    vs.update({(1 << 127) - 1, (1 << 127) - 2, -((1 << 127) - 1), -(1 << 127)})
    for x in (127, 128, 129, 255, 256, 32767, 32768, 32769):
        vs.add(x)
        vs.add(-x)
    return sorted(vs)


def tie_cases():
    """(v, s): exact ties (2^53 + 1) * 10^s and (2^54 + 2 +- 1) * 10^s with their neighbours +-1."""
    out = []
    for s in range(0, 39):
        for base in ((1 << 53) + 1, (1 << 54) + 1, (1 << 54) + 3):
            t = base * 10 ** s
            if t + 1 < LIMIT:
                for d in (-1, 0, 1):
                    out.append((t + d, s))
                    out.append((-(t + d), s))
    return out


def hard_cases():
    cases = [(v, s) for v in hard_values() for s in SCALES]
    return cases + tie_cases()


def random_cases(n, seed):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        nb = rnd.randint(1, 126)
        v = rnd.getrandbits(nb) % LIMIT
        if rnd.random() < 0.5:
            v = -v
        out.append((v, rnd.randint(0, 38)))
    return out


def random_values(n, seed, max_bits=126):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        v = rnd.getrandbits(rnd.randint(1, max_bits)) % LIMIT
        out.append(-v if rnd.random() < 0.5 else v)
    return out


HASH_EDGES = [s * x for x in (127, 128, 129, 1 << 63, 1 << 64, LIMIT - 1) for s in (1, -1)] + [0, 1, -1]


# ---- aggregates over a column (values: ints, None = NULL; rows: the rows `where` keeps) -----------------------
def hll_words(values):
    """The 52 packed register words of StatefulHyperloglogPlus (P = 9) over the non-NULL values."""
    regs = [0] * 512
    for v in values:
        if v is None:
            continue
        h = spark_hash(v) & ((1 << 64) - 1)
        idx = h >> 55
        w = ((h << 9) | (1 << 8)) & ((1 << 64) - 1)
        rank = 64 - w.bit_length() + 1
        regs[idx] = max(regs[idx], rank)
    words = []
    for w in range(52):
        word = 0
        for k in range(10):
            i = w * 10 + k
            if i < 512:
                word |= (regs[i] & 63) << (6 * k)
        words.append(word - (1 << 64) if word >> 63 else word)
    return words


def moments(values, s):
    """(n, avg, m2) of the per-row doubles, exactly, rounded once at the end. Every double is an integer multiple of
    2^emin (emin = the smallest exponent of the column), so the sums are plain integer arithmetic."""
    xs = [to_double(v, s) for v in values if v is not None]
    n = len(xs)
    if n == 0:
        return 0.0, 0.0, 0.0
    parts = []
    for x in xs:
        fr, ex = math.frexp(x)
        parts.append((int(fr * (1 << 53)), ex - 53))
    emin = min(e for _, e in parts)
    ints = [m << (e - emin) for m, e in parts]
    s1 = sum(ints)
    s2 = sum(i * i for i in ints)
    mean = Fraction(s1, n) * Fraction(2) ** emin
    m2 = Fraction(n * s2 - s1 * s1, n) * Fraction(2) ** (2 * emin)
    return float(n), float(mean), float(m2)


def exact_sums(values, s):
    """(sum x in units of 2^-180, sum x^2 in units of 2^-360) of the per-row doubles, as integers."""
    s1 = s2 = 0
    for v in values:
        if v is None:
            continue
        x = Fraction(to_double(v, s))
        a, b = x * (1 << 180), x * x * (1 << 360)
        assert a.denominator == 1 and b.denominator == 1
        s1 += a.numerator
        s2 += b.numerator
    return s1, s2


def metrics(values, s):
    """Expected metric values of the seven analyzers over `values` (None = NULL); None where the state is empty.
    Sum / Mean are "overflow" when the exact total has 39 or more digits."""
    nn = [v for v in values if v is not None]
    out = {"Completeness": (len(nn) / len(values)) if values else None}
    if not nn:
        out.update(Sum=None, Mean=None, Minimum=None, Maximum=None, StandardDeviation=None)
        return out
    tot = sum(nn)
    if abs(tot) >= LIMIT:
        out["Sum"] = out["Mean"] = "overflow"
    else:
        out["Sum"] = to_double(tot, s)
        out["Mean"] = to_double(tot, s) / len(nn)
    out["Minimum"] = to_double(min(nn), s)
    out["Maximum"] = to_double(max(nn), s)
    n, avg, m2 = moments(values, s)
    out["moments"] = (n, avg, m2)
    out["StandardDeviation"] = math.sqrt(m2 / n)
    return out
