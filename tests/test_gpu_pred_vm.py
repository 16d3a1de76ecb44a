"""The general predicate VM (predicate_kernel, csrc/predicate.hip) against the oracle's own parser and row evaluator
(oracle/oracle.py: Java number semantics, SQL three-valued logic), over what no other GPU test reaches: + - * / %,
unary minus, BETWEEN, <=>, coalesce, IN / NOT IN with a NULL item, a grouped IN list, LIKE, mixed-type column to
column comparisons, string ordering, BOOLEAN columns, and every predicate shape over DECIMAL(<= 18) columns -- as
Compliance predicates and as the `where` of Size / Completeness / Sum. Bar: the states (counts, Long sums) are equal,
no tolerance.

Row counts 1, 63, 64, 65, 255, 257, 2049, 4099: the kernel evaluates one row per lane, writes one ballot word per
64-lane wave, runs 256-row workgroups and pads the bitmaps to 2048-row tiles.

A DECIMAL column reads as Spark's Decimal.toDouble in the VM and in the oracle; Spark itself compares decimals
exactly. All decimal magnitudes here stay below 2^53 (|unscaled| < 10^12), where the double of a decimal with at most
15 significant digits decides =, < and > like the exact comparison does, so product, oracle and Spark agree."""
import functools
import os
import re

import numpy as np
import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import engine
from deequ_amd.table import Column, Table, _column_from_pylist, pack_validity
import oracle as O

pytestmark = pytest.mark.gpu

LONG_MAX, LONG_MIN, P53 = (1 << 63) - 1, -(1 << 63), 1 << 53
SIZES = [1, 63, 64, 65, 255, 257, 2049]  # and 4099: the full list below
FULL = 4099

ARITH = [
    "l + m > 3", "l - m - 1 > 0", "l * m = 6", "-l < -2", "l / m >= 1.5", "l / 0 IS NULL", "l % m = 1", "l % 3 = -1",
    "d % 2 = 0.5", "l % 0 IS NULL", "abs(l - 5) <= 3", "l + 1 < l", "l * 2 / 2 = l", "i + 3000000000 > 0",
    "h * b > 100", "d + l > 0", "f * 2 = d", "CAST(d AS BIGINT) % 2 = 0",
]
IN20 = "l IN (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 33, 35, 37, %d)" % (P53 + 1)
COMPARE = [
    "l < d", "d <= l", "i = h", "f = d", "l = 9007199254740992.0", "z = true AND l > 0", "z <=> NULL", "l <=> m",
    "d <=> d", "l BETWEEN -2 AND m", "d NOT BETWEEN 0 AND 1", "coalesce(l, m, 0) > 0", "coalesce(d, 0.0) >= 0",
    "l IN (1, NULL)", "l NOT IN (1, 2)", "l NOT IN (1, NULL)", "d IN (0.0, m)", IN20,
]
STRING = [
    "s < 'abd'", "s >= s2", "s = s2", "s != ''",
    "s LIKE 'a%'", "s LIKE '%c'", "s LIKE '%b%d%'", "s LIKE '_'", "s LIKE '__%'", "s LIKE '%'", "s LIKE ''",
    "s LIKE '_é%'", "s LIKE '%%x'", "s NOT LIKE 'ab_'",
    "length(s) >= 2 AND s2 IS NOT NULL", "s > 2", "s + 1 = 6",
]
# unscaled 7, 11, 1999 and -14 at scale 2, and 7 at scale 6, are values whose repeated division by 10 is not the
# literal's double (asserted in test_decimal_literals_sit_on_repeated_division_errors)
DECIMAL_LITERALS = ["0.07", "0.11", "19.99", "-0.14"]
DECIMAL = ["dec2 %s %s" % (op, lit) for lit in DECIMAL_LITERALS for op in ("=", "!=", "<", "<=", ">", ">=")] + [
    "dec2 IN (0.07, 0.17, 1.5)", "dec2 BETWEEN 0.07 AND 19.99", "dec6 = 0.000007", "dec6 <= 1.000001", "dec0 = 7",
    "dec2 > d", "dec2 * 100 >= 700", "coalesce(dec2, 0.0) >= 0", "CAST(dec2 AS BIGINT) = 19",
    "dec2 IS NULL OR dec2 < 0",
]
FAMILIES = {"arith": ARITH, "compare": COMPARE, "string": STRING, "decimal": DECIMAL}
# one predicate or more per operator family, at every small size
SUBSET = ["l + m > 3", "l % m = 1", "l / m >= 1.5", "l < d", "l BETWEEN -2 AND m", "coalesce(l, m, 0) > 0",
          "l NOT IN (1, NULL)", "l <=> m", "s >= s2", "s LIKE '%b%d%'", "z = true AND l > 0", "dec2 = 0.07"]
assert len(SUBSET) == 12 and all(any(p in f for f in FAMILIES.values()) for p in SUBSET)

# written as constants: the same truth value in every row where they are not NULL
CONSTANT = {"l / 0 IS NULL", "l % 0 IS NULL", "d <=> d", "l NOT IN (1, NULL)"}
# never NULL by construction (IS NULL, <=>, a coalesce that ends in a constant, `x IS NULL OR ...` over the same x)
NEVER_NULL = {"l / 0 IS NULL", "l % 0 IS NULL", "z <=> NULL", "l <=> m", "d <=> d", "coalesce(l, m, 0) > 0",
              "coalesce(d, 0.0) >= 0", "coalesce(dec2, 0.0) >= 0", "dec2 IS NULL OR dec2 < 0"}

WORDS = ["", "a", "ab", "abc", "abd", "abcdefghijklmnopqrstuvwxyzabcdefghijklmn", "é", "€x", "😀", "a%b", "a_b", "ab ",
         "abc  ", "5", "2.5", "-1", "aéz", "bcd", "xx", "b", "abz"]
assert len(WORDS[5].encode()) == 40


def _with_nulls(rng, name, spark_type, values, rate, **kw):
    valid = rng.random(len(values)) >= rate
    return Column(name, spark_type, np.ascontiguousarray(values), pack_validity(valid), **kw)


def _sprinkle(rng, values, specials, every):
    """`specials` over every `every`-th row or so (from row 0 on, so the smallest tables hold some too)."""
    at = np.arange(0, len(values), every)
    values[at] = np.asarray(specials, dtype=values.dtype)[rng.integers(0, len(specials), len(at))]
    return values


def vm_table(n, seed=41):
    """The one table of this file; the same rows for the same (n, seed)."""
    rng = np.random.default_rng(seed + n)
    l = _sprinkle(rng, rng.integers(-9, 10, n).astype(np.int64), [LONG_MIN, LONG_MAX, P53 + 1, -(P53 + 1), 0], 17)
    m = rng.integers(-3, 4, n).astype(np.int64)
    h = rng.integers(-300, 301, n).astype(np.int16)
    i = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    same = np.arange(3, n, 29)
    i[same] = h[same]  # rows where `i = h` holds
    b = rng.integers(-128, 128, n).astype(np.int8)
    z = (rng.random(n) < 0.4).astype(np.uint8)
    halves = rng.integers(-20, 21, n) * 0.5
    d = _sprinkle(rng, halves.copy(), [np.nan, np.inf, -np.inf, -0.0, 0.0], 13)
    f = _sprinkle(rng, (rng.integers(-20, 21, n) * 0.5).astype(np.float32), [np.nan, np.inf, -np.inf, -0.0, 0.0], 19)
    dec2 = _sprinkle(rng, rng.integers(-20000, 20001, n).astype(np.int64),
                     [7, 11, 14, 17, 1999, 0, -14, 150, 10, 100, 1900, 17000, -7], 7)
    dec6 = _sprinkle(rng, rng.integers(-10 ** 12 + 1, 10 ** 12, n).astype(np.int64),
                     [7, 1000001, 0, 1000000, -7, 1500000, 999999], 5)
    dec0 = _sprinkle(rng, rng.integers(-50, 51, n).astype(np.int64), [7, 9999999999, -9999999999, 0], 11)
    cols = [
        _with_nulls(rng, "l", N.TYPE_LONG, l, 0.07), _with_nulls(rng, "m", N.TYPE_LONG, m, 0.06),
        _with_nulls(rng, "i", N.TYPE_INT, i, 0.05), _with_nulls(rng, "h", N.TYPE_SHORT, h, 0.05),
        _with_nulls(rng, "b", N.TYPE_BYTE, b, 0.05), _with_nulls(rng, "z", N.TYPE_BOOLEAN, z, 0.08),
        _with_nulls(rng, "d", N.TYPE_DOUBLE, d, 0.07), _with_nulls(rng, "f", N.TYPE_FLOAT, f, 0.06),
        _with_nulls(rng, "dec2", N.TYPE_DECIMAL, dec2, 0.07, decimal_precision=18, decimal_scale=2),
        _with_nulls(rng, "dec6", N.TYPE_DECIMAL, dec6, 0.06, decimal_precision=18, decimal_scale=6),
        _with_nulls(rng, "dec0", N.TYPE_DECIMAL, dec0, 0.05, decimal_precision=10, decimal_scale=0),
    ]
    for name in ("s", "s2"):
        cols.append(_column_from_pylist(name, "string", [None if rng.random() < 0.08 else
                                                         WORDS[rng.integers(len(WORDS))] for _ in range(n)]))
    return Table(cols)


@functools.lru_cache(maxsize=None)
def _host_table(n):
    """The host-resident table of n rows, built once: the oracle memoises its masks per table object."""
    return vm_table(n)


def analyzers_for(k, p):
    return [D.Compliance("c%d" % k, p), D.Size(p), D.Completeness("l", p), D.Sum("l", p)]


@functools.lru_cache(maxsize=None)
def _expected(n, p):
    """The oracle's states of analyzers_for(., p) on the n-row table: computed once, shared, never changed."""
    return tuple(O.expected_state(_host_table(n), a) for a in analyzers_for(0, p))


def _run(t, analyzers, force_vm):
    """The analyzers' states from one ScanBatch, and the scan's kernel launch counts of that run. force_vm: every
    predicate on the general VM (DQ_PRED_VM=1, read per call), also the few the simple kernel would take."""
    old = os.environ.get("DQ_PRED_VM")
    if force_vm:
        os.environ["DQ_PRED_VM"] = "1"
    else:
        os.environ.pop("DQ_PRED_VM", None)
    try:
        batch = D.ScanBatch(t)
        offsets = [a.addOps(batch) for a in analyzers]
        before = engine.ctx().kernel_launches()
        res = batch.run()
        after = engine.ctx().kernel_launches()
    finally:
        if old is None:
            os.environ.pop("DQ_PRED_VM", None)
        else:
            os.environ["DQ_PRED_VM"] = old
    return ([a.fromAggregationResult(res, o) for a, o in zip(analyzers, offsets)],
            {k: after[k] - before[k] for k in after})


def _check(t, n, preds, force_vm):
    analyzers = [a for k, p in enumerate(preds) for a in analyzers_for(k, p)]
    got, launches = _run(t, analyzers, force_vm)
    bad = []
    for k, p in enumerate(preds):
        for a, g, e in zip(analyzers[4 * k:4 * k + 4], got[4 * k:4 * k + 4], _expected(n, p)):
            print(n, p, type(a).__name__, g, e)
            if not ((g is None and e is None) or (g is not None and e is not None and g == e)):
                bad.append((p, type(a).__name__, g, e))
    assert not bad, bad
    assert launches["pred_vm"] >= len(set(preds)), launches
    return launches


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("family", ["arith", "compare", "string"])
def test_vm_predicates_match_oracle(family, device):
    """Every predicate of the family at 4099 rows on the VM, host columns and device-resident ones."""
    t = vm_table(FULL).to_device(0) if device else _host_table(FULL)
    launches = _check(t, FULL, FAMILIES[family], force_vm=True)
    assert launches["pred_simple"] == 0, launches


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_decimal_predicates_match_oracle(device):
    """Every predicate over a DECIMAL column, as the scan routes it on its own: all of them run on the VM (a leaf
    `dec <op> constant` is not a simple predicate), and 0.07 = 0.07."""
    t = vm_table(FULL).to_device(0) if device else _host_table(FULL)
    launches = _check(t, FULL, DECIMAL, force_vm=False)
    assert launches["pred_simple"] == 0, launches


@pytest.mark.parametrize("n", SIZES)
def test_vm_subset_at_wave_workgroup_and_tile_edges(n):
    _check(_host_table(n), n, SUBSET, force_vm=True)


def test_predicates_are_not_vacuous():
    """From the oracle's own masks at 4099 rows: every predicate has a TRUE row and a row that is not TRUE (the few
    written as constants apart), and every predicate that can be NULL is NULL somewhere."""
    t = _host_table(FULL)
    for p in ARITH + COMPARE + STRING + DECIMAL:
        true, notnull = O.predicate_masks(t, p)
        if p not in CONSTANT:
            assert true.any() and not true.all(), p
        assert (not notnull.all()) == (p not in NEVER_NULL), p
    for p in CONSTANT:
        true, notnull = O.predicate_masks(t, p)
        assert true[notnull].all() or not true.any(), p


def test_decimal_literals_sit_on_repeated_division_errors():
    """The decimal literals are values a load by `scale` divisions by 10 gets wrong: (double) u / 10 / 10 is not the
    literal's double, (double) u / 100 is (IEEE arithmetic, computed here on the host). The table holds such rows."""
    hard = 0
    for lit in DECIMAL_LITERALS + ["0.000007"]:
        scale = len(lit.split(".")[1])
        u = int(lit.replace(".", ""))
        x = float(u)
        for _ in range(scale):
            x /= 10.0
        assert float(u) / 10.0 ** scale == float(lit)
        hard += x != float(lit)
        col = _host_table(FULL)["dec2" if scale == 2 else "dec6"]
        assert (np.asarray(col.values)[O._valid(col)] == u).any(), lit
    assert hard >= 4


def test_streamed_scan_offsets_the_vm_pass():
    """dq_scan_streamed in 2048-row chunks (2048 + 2048 + 3 rows): the VM runs per chunk at the chunk's row offset.
    The three rows of the last chunk are set by hand: TRUE (1, 19.99), FALSE (4, 20.00), FALSE (2, 0.07)."""
    full = _host_table(FULL)
    cols = []
    for name, tail in (("l", [1, 4, 2]), ("dec2", [1999, 2000, 7])):
        c = full[name]
        values, valid = np.asarray(c.values).copy(), O._valid(c).copy()
        values[4096:], valid[4096:] = tail, True
        cols.append(Column(name, c.spark_type, values, pack_validity(valid), decimal_precision=c.decimal_precision,
                           decimal_scale=c.decimal_scale))
    t = Table(cols)
    w = "l % 3 = 1 AND dec2 <= 19.99"
    analyzers = analyzers_for(0, w)
    batch = D.ScanBatch(t)
    offsets = [a.addOps(batch) for a in analyzers]
    before = engine.ctx().kernel_launches()["pred_vm"]
    got = D.runners.ScanResult(engine.ctx().scan_streamed(batch.native_columns(), t.nrows, batch.ops,
                                                          [p.to_native() for p in batch.preds], 2048))
    assert engine.ctx().kernel_launches()["pred_vm"] - before >= 3
    for a, o in zip(analyzers, offsets):
        g, e = a.fromAggregationResult(got, o), O.expected_state(t, a)
        print(w, type(a).__name__, g, e)
        assert g is not None and g == e, (a, g, e)
    true, notnull = O.predicate_masks(t, w)
    assert true[:2048].any() and true[2048:4096].any() and not notnull.all()
    assert true[4096:].tolist() == [True, False, False] and notnull[4096:].all()


RLIKE_PATTERNS = [r"\.50$", r"^-?\d+\.\d{2}$", r"0$", r"^1\.5$", r"E-"]


def test_decimal_rlike_reads_bigdecimal_text():
    """dec RLIKE p matches Cast(decimal AS STRING) = BigDecimal.toString of the cell ("1.50", "100.00", "7E-8"), the
    text PatternMatch matches, not the double's ("1.5"). Expected counts are built here: the oracle's
    java_bigdecimal_to_string of each cell and Python's re.search on plain anchored digit patterns, where Java and
    Python agree. dec6 never prints in scientific form (BigDecimal switches below an adjusted exponent of -6, which
    needs a scale of 7 at least), so a DECIMAL(18,8) column of small values stands beside it for `E-`."""
    n = 257
    rng = np.random.default_rng(7)
    dec2 = _sprinkle(rng, rng.integers(-20000, 20001, n).astype(np.int64), [150, -150, 10, 100, 10000, 0, 7, 1950], 3)
    dec6 = _sprinkle(rng, rng.integers(-10 ** 7, 10 ** 7, n).astype(np.int64), [7, 1500000, 0, 1000000, -10], 4)
    dec0 = _sprinkle(rng, rng.integers(-500, 501, n).astype(np.int64), [0, 10, -150, 9999999990], 5)
    dec8 = _sprinkle(rng, rng.integers(-300, 301, n).astype(np.int64), [7, 15, 0, 150000000, -1, 100], 3)
    t = Table([_with_nulls(rng, "dec2", N.TYPE_DECIMAL, dec2, 0.07, decimal_precision=18, decimal_scale=2),
               _with_nulls(rng, "dec6", N.TYPE_DECIMAL, dec6, 0.07, decimal_precision=18, decimal_scale=6),
               _with_nulls(rng, "dec0", N.TYPE_DECIMAL, dec0, 0.07, decimal_precision=10, decimal_scale=0),
               _with_nulls(rng, "dec8", N.TYPE_DECIMAL, dec8, 0.07, decimal_precision=18, decimal_scale=8)])
    cases, analyzers = [], []
    for name in t.columns:
        col = t[name]
        valid = O._valid(col)
        texts = [O.java_bigdecimal_to_string(int(u), col.decimal_scale)
                 for u, ok in zip(np.asarray(col.values), valid) if ok]
        for p in RLIKE_PATTERNS:
            cases.append((name, p, sum(re.search(p, x) is not None for x in texts)))
            # a SQL string literal takes `\\` for one backslash
            analyzers += [D.Compliance("c", "%s RLIKE '%s'" % (name, p.replace("\\", "\\\\"))), D.PatternMatch(name, p)]
    got, launches = _run(t, analyzers, force_vm=False)
    bad = []
    for k, (name, p, want) in enumerate(cases):
        rlike, pm = got[2 * k], got[2 * k + 1]
        print(name, p, want, rlike, pm)
        if (rlike.numMatches, rlike.count, pm.numMatches, pm.count) != (want, n, want, n):
            bad.append((name, p, want, rlike, pm))
    assert not bad, bad
    assert launches["pred_vm"] >= len(cases) and launches["pred_simple"] == 0, launches
    hits = {(name, p): want for name, p, want in cases}
    assert hits[("dec2", r"\.50$")] and hits[("dec8", "E-")] and hits[("dec6", "E-")] == 0
    assert hits[("dec2", r"^1\.5$")] == 0 and hits[("dec2", r"^-?\d+\.\d{2}$")] == int(O._valid(t["dec2"]).sum())
