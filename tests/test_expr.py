"""Predicate compiler (Spark SQL strings -> dq_predicate postfix programs). CPU only."""
import pytest

import deequ_amd.native as N
from deequ_amd.expr import compile_predicate, PredicateSyntaxError, UnresolvedColumnError


COLS = {"item": 0, "att1": 1, "att2": 2}


def ops(text):
    p = compile_predicate(text, COLS)
    code = list(p._code)
    return [(code[i], code[i + 1]) for i in range(0, len(code), 2)]


def test_reference_predicates_compile():
    # the predicates the reference tests use
    for t in ["item IN ('1', '2')", "att1 > 3", "att1 > 2", "att2 = 0", "att1 < 4", "item != '6'",
              "unique < 4".replace("unique", "att1"), "att1 = 'b'", "att1 != ''", "att1 != 'dddd'",
              "att1 IS NULL OR att2 IS NOT NULL", "NOT (att1 >= 2 AND att2 <= 5)", "att1 BETWEEN 1 AND 3",
              "coalesce(att1, 0) > 1", "att1 LIKE '%fac%ets'", "length(item) >= 2", "att1 + att2 * 2 > 3",
              "`att1` <=> NULL", "att1 NOT IN (1, 2)", "CAST(item AS DOUBLE) > 1.5", "att1 == 3", "att1 <> 3"]:
        p = compile_predicate(t, COLS)
        assert len(p._code) % 2 == 0 and len(p._code) > 0, t


def test_postfix_shape():
    assert ops("att1 > 3") == [(N.P_COL, 1), (N.P_CONST, 0), (N.P_GT, 0)]
    assert ops("item IN ('1', '2')") == [(N.P_COL, 0), (N.P_CONST, 0), (N.P_CONST, 1), (N.P_IN, 2)]
    assert ops("att1 > 1 AND att2 < 2 OR att1 IS NULL")[-1] == (N.P_OR, 0)
    assert ops("NOT att1 > 1")[-1] == (N.P_NOT, 0)


def test_precedence_and_or():
    # a OR b AND c == a OR (b AND c)
    o = ops("att1 = 1 OR att1 = 2 AND att2 = 3")
    assert o[-1] == (N.P_OR, 0) and o[-2] == (N.P_AND, 0)


def test_unknown_column_is_an_analysis_error():
    with pytest.raises(UnresolvedColumnError):
        compile_predicate("attNoSuchColumn > 3", COLS)


def test_syntax_errors():
    for t in ["att1 >", "(att1 > 1", "att1 > 1)", "att1 LIKE att2", "frobnicate(att1)"]:
        with pytest.raises(PredicateSyntaxError):
            compile_predicate(t, COLS)


def test_string_constants_pool():
    p = compile_predicate("item = 'héllo' OR item = 'it''s'", COLS)
    pool = bytes(p._strings[:p._strings_len])
    assert "héllo".encode() in pool and b"it's" in pool


# The oracle parses predicates with its own precedence-climbing parser (oracle.OracleParser): the
# product parse trees are pinned by evaluating both over a grid of rows with NULLs, and by the truth
# tables of the reference's own predicates on the reference fixtures.
CORPUS = ["item IN ('1', '2')", "att1 > 3", "att2 = 0", "att1 < 4", "item != '6'", "att1 != 2",
          "att1 IS NULL OR att2 IS NOT NULL", "NOT (att1 >= 2 AND att2 <= 5)", "att1 BETWEEN 1 AND 3",
          "coalesce(att1, 0) > 1", "item LIKE '%1%'", "length(item) >= 2", "att1 + att2 * 2 > 3", "`att1` <=> NULL",
          "att1 NOT IN (1, 2)", "CAST(item AS DOUBLE) > 1.5", "att1 == 3", "att1 <> 3", "-att1 < -2 OR att2 % 2 = 1",
          "att1 - att2 - 1 > 0", "att1 / 2 >= 1.5", "NOT att1 > 1 AND att2 IS NULL", "att1 NOT BETWEEN 2 AND 4",
          "item NOT LIKE '_'", "att1 IN (1, NULL)", "att1 = 1 OR att1 = 2 AND att2 = 3", "(att1 = 1 OR att1 = 2) AND att2 = 3",
          "att2 >= 0 AND att2 < 6 OR att1 IS NULL", "CAST(att1 AS BIGINT) * 2 = 4", "isnull(att2) OR att1 > 5",
          "`att1` IS NULL OR `att1` >= 0", "1.5e0 < att1", "att1 > 2.0d", "item = 'it''s'"]


def _rows():
    import itertools
    items = ["1", "2", "11", None, "it's", "2.5"]
    vals = [None, 0, 1, 2, 3, 4, 5, 6, 7]
    return [{"item": i, "att1": a, "att2": b} for i, a, b in itertools.product(items, vals, vals)]


def test_oracle_parser_agrees_with_product_parser():
    import oracle as O
    from deequ_amd.expr import _Parser
    rows = _rows()
    for text in CORPUS:
        mine, theirs = O.OracleParser(text).parse(), _Parser(text).parse()
        for r in rows:
            assert O._eval(mine, r) == O._eval(theirs, r), (text, r)


def test_oracle_parser_reference_truth_tables(kats):
    """Compliance KATs of the reference (tests/golden/kats.json) re-evaluated through the oracle parser."""
    import oracle as O
    from helpers import table_from_fixture
    seen = 0
    for k in kats["kats"]:
        if k["analyzer"][0] != "Compliance" or not isinstance(k["expected"], (int, float)):
            continue
        t = table_from_fixture(kats["fixtures"][k["fixture"]])
        truth, _ = O.predicate_masks(t, k["analyzer"][2])
        where = k["analyzer"][3] if len(k["analyzer"]) > 3 else None
        wt = O.predicate_masks(t, where)[0] if where else [True] * t.nrows
        den = sum(1 for w in wt if w) if where else t.nrows
        got = sum(1 for a, w in zip(truth, wt) if a and w) / den
        assert got == k["expected"], k
        seen += 1
    assert seen >= 3


# Spark SQL beyond the predicates Check.scala generates (VERDICT r04 missing #4): CASE WHEN, RLIKE, string and date
# functions, isnan / nanvl / abs, DATE literals. Compiled programs here; GPU parity against the oracle in
# tests/test_gpu_pred_surface.py.
SURFACE = ["CASE WHEN att1 > 1 THEN 'big' WHEN att1 = 1 THEN 'one' ELSE 'small' END = 'big'",
           "CASE att1 WHEN 1 THEN TRUE WHEN 2 THEN FALSE END", "if(att1 > 2, att2, -1) >= 0",
           "item RLIKE '^[0-9]+$'", "item NOT RLIKE '\\\\.'", "item REGEXP '(?i)IT'", "lower(item) = 'it''s'",
           "upper(item) LIKE 'IT%'", "trim(item) = '1'", "ltrim(item) <> rtrim(item)", "substring(item, 2) = '1'",
           "substr(item, -1, 1) = '5'", "isnan(att1)", "nanvl(att1, 0) > 1", "abs(att1 - 3) <= 1",
           "nvl(att1, 0) + ifnull(att2, 0) > 3", "lcase(item) = ucase(item)", "length(trim(item)) = 1"]


def test_sql_surface_compiles():
    from deequ_amd.expr import compile_predicate
    for text in SURFACE:
        p = compile_predicate(text, COLS)
        assert len(p._code) % 2 == 0 and len(p._code) > 0, text
    p = compile_predicate("item RLIKE 'a+'", COLS)
    ops = list(p._code[0::2])
    assert N.P_RLIKE in ops
    k = p._code[list(p._code[0::2]).index(N.P_RLIKE) * 2 + 1]
    assert p._consts[k].str_offset % 4 == 0 and p._consts[k].str_len >= 32  # an aligned regex program image
    with pytest.raises(PredicateSyntaxError):
        compile_predicate("year(att1) = 2020", COLS, {"att1": N.TYPE_LONG})  # year() of a non-date column
    d = compile_predicate("year(d) = 2020 AND d >= DATE '2020-02-01'", dict(COLS, d=3),
                          {"d": N.TYPE_DATE})
    assert N.P_YEAR in list(d._code[0::2])


def test_sql_surface_oracle_known_answers():
    """The oracle's evaluation of the new forms against hand-computed Spark 2.2 results (three-valued logic: a NULL
    input gives NULL, isnan(NULL) is FALSE, CASE without a matching WHEN and without ELSE is NULL)."""
    import oracle as O
    rows = [({"item": " 12 ", "att1": 2, "att2": None}, {
        "trim(item) = '12'": True, "ltrim(item) = '12 '": True, "rtrim(item) = ' 12'": True,
        "substring(item, 2, 2) = '12'": True, "substring(item, -2, 1) = '2'": True, "substring(item, 0, 2) = ' 1'": True,
        "item RLIKE '\\\\d{2}'": True, "item RLIKE '^\\\\d'": False, "item RLIKE ''": True,
        "CASE WHEN att2 > 1 THEN 1 END = 1": None, "CASE WHEN att2 > 1 THEN 1 ELSE 2 END = 2": True,
        "CASE att1 WHEN 2 THEN 'two' ELSE 'other' END = 'two'": True, "if(att2 IS NULL, 1, 0) = 1": True,
        "isnan(att2)": False, "nanvl(att2, 1) = 1": None, "abs(att1 - 5) = 3": True,
        "upper(item) = ' 12 '": True, "nvl(att2, 7) = 7": True}),
        ({"item": "AbC", "att1": float("nan"), "att2": 3}, {
            "lower(item) = 'abc'": True, "upper(item) LIKE 'AB_'": True, "item RLIKE '(?i)abc'": True,
            "item RLIKE 'abc'": False, "isnan(att1)": True, "nanvl(att1, 5) = 5": True, "att1 > 1e308": True})]
    for row, cases in rows:
        for text, want in cases.items():
            got = O._eval(O.OracleParser(text).parse(), row)
            assert got == want, (text, row, got, want)


def test_oracle_casts_follow_java_not_python():
    """CAST in the oracle is Java's, where Python's float() / int() differ: Cast(string -> double) is
    Double.parseDouble ("inf", "nan", "1_0" throw -> NULL; "Infinity", String.trim and hexadecimal literals are
    accepted), Cast(string -> long) is UTF8String.toLong (no exponent, no trimming), Cast(double -> long) saturates
    (NaN -> 0). The implicit string -> double promotion of a comparison takes the same parser."""
    import math
    import oracle as O
    big, small = (1 << 63) - 1, -(1 << 63)
    cases = [({"item": "1e5"}, {"CAST(item AS BIGINT) IS NULL": True, "CAST(item AS DOUBLE) = 100000": True,
                                "item = 100000": True}),
             ({"item": "inf"}, {"CAST(item AS DOUBLE) IS NULL": True, "CAST(item AS BIGINT) IS NULL": True,
                                "item > 0": None, "isnan(item)": False}),
             ({"item": "Infinity"}, {"CAST(item AS DOUBLE) > 1e308": True, "CAST(item AS BIGINT) IS NULL": True}),
             ({"item": "nan"}, {"CAST(item AS DOUBLE) IS NULL": True, "isnan(item)": False}),
             ({"item": "NaN"}, {"isnan(CAST(item AS DOUBLE))": True, "isnan(item)": True}),
             ({"item": " 7"}, {"CAST(item AS DOUBLE) = 7": True, "CAST(item AS BIGINT) IS NULL": True}),
             ({"item": "1_0"}, {"CAST(item AS DOUBLE) IS NULL": True, "CAST(item AS BIGINT) IS NULL": True,
                                "item = 10": None, "abs(item) = 10": None, "item + 1 = 11": None}),
             ({"item": "0x1p3"}, {"CAST(item AS DOUBLE) = 8": True, "CAST(item AS DOUBLE) = 0": False}),
             ({"item": "12.9"}, {"CAST(item AS BIGINT) = 12": True}),
             ({"att1": 1e19}, {"CAST(att1 AS BIGINT) = %d" % big: True}),
             ({"att1": -1e19}, {"CAST(att1 AS BIGINT) = %d" % small: True}),
             ({"att1": float("inf")}, {"CAST(att1 AS BIGINT) = %d" % big: True}),
             ({"att1": float("-inf")}, {"CAST(att1 AS BIGINT) = %d" % small: True}),
             ({"att1": float("nan")}, {"CAST(att1 AS BIGINT) = 0": True}),
             ({"att1": -0.9}, {"CAST(att1 AS BIGINT) = 0": True}),
             ({"att1": 9223372036854775807.0}, {"CAST(att1 AS BIGINT) = %d" % big: True}),
             ({"att1": -9223372036854777856.0}, {"CAST(att1 AS BIGINT) = %d" % small: True})]
    for row, want in cases:
        row = dict({"item": None, "att1": None, "att2": None}, **row)
        for text, exp in want.items():
            got = O._eval(O.OracleParser(text).parse(), row)
            assert got is exp or (got == exp and type(got) is type(exp)), (text, row, got, exp)
    assert math.isinf(O._eval(O.OracleParser("CAST(item AS DOUBLE)").parse(), {"item": "-Infinity"}))


def test_oracle_numbers_follow_java_not_python():
    """Numbers in the oracle are Java's, where Python's differ: long + - *, unary minus and abs wrap to 64 bits; % on
    longs is Java's remainder in integer arithmetic (sign of the dividend, exact past 2^53, NULL for a zero divisor)
    and stays fmod with a double operand; a long against a double is cast to double first (round to nearest even),
    in comparisons, IN and <=>; a DECIMAL cell is Decimal.toDouble, (double) unscaled / 10.0^scale. Every expected
    value below is worked out by hand from those rules, none is taken from the oracle."""
    import numpy as np
    import oracle as O
    from deequ_amd.table import Column
    big, small = (1 << 63) - 1, -(1 << 63)
    p53 = 1 << 53  # 9007199254740992: from here on only even longs are doubles
    cases = [
        # + - * wrap: Long.MAX + 1 = Long.MIN, Long.MIN - 1 = Long.MAX, Long.MAX * 2 = -2, Long.MIN * -1 = Long.MIN
        ({"att1": big}, {"att1 + 1": small, "att1 * 2": -2, "att1 + 1 < att1": True, "att1 + att1": -2}),
        ({"att1": small}, {"att1 - 1": big, "att1 * -1": small, "-att1": small, "abs(att1)": small,
                           "att1 % -1": 0, "-att1 < 0": True}),
        ({"att1": -5}, {"-att1": 5, "abs(att1)": 5, "abs(att1 - 5)": 10}),
        # Java's %: truncated division, the sign follows the dividend; NULL for x % 0
        ({"att1": -7}, {"att1 % 3": -1, "att1 % -3": -1, "att1 % 0": None, "att1 % 7": 0,
                        "att1 % 2.0": -1.0, "att1 % 0.0": None, "att1 % 2.5": -2.0}),
        ({"att1": 7}, {"att1 % -3": 1, "att1 % 3": 1, "att1 % 0": None, "att1 % -2.0": 1.0}),
        # in integer arithmetic: 2^53 + 1 is odd, and ends in ...993 (as doubles it would be 2^53: even, ...992)
        ({"att1": p53 + 1}, {"att1 % 2": 1, "att1 % 10": 3, "-att1 % 2": -1}),
        ({"att1": big}, {"att1 % 10": 7, "att1 % 2": 1}),
        ({"att1": 7.5}, {"att1 % 2": 1.5, "-att1 % 2": -1.5}),
        # Java's double %: an infinite dividend gives NaN (Python's math.fmod raises), an infinite divisor the dividend
        ({"att1": float("inf"), "att2": 7.5}, {"isnan(att1 % 2)": True, "isnan(-att1 % 2.5)": True,
                                               "att2 % att1": 7.5, "att1 % 0": None}),
        # long vs double: the long becomes a double first; (double)(2^53 + 1) = 2^53 (the tie goes to the even
        # mantissa), (double)(2^53 - 1) is exact
        ({"att1": p53 + 1, "att2": float(p53)},
         {"att1 = att2": True, "att2 = att1": True, "att1 > att2": False, "att2 < att1": False, "att1 <= att2": True,
          "att2 >= att1": True, "att1 != att2": False, "att1 <=> att2": True, "att2 <=> att1": True,
          "att1 IN (att2)": True, "att2 IN (att1)": True, "att1 IN (1.0, 2.0)": False,
          "att1 = 9007199254740992.0": True, "9007199254740992.0 = att1": True, "att1 < 9007199254740994.0": True}),
        ({"att1": p53 - 1, "att2": float(p53)},
         {"att1 = att2": False, "att2 = att1": False, "att1 < att2": True, "att2 > att1": True,
          "att1 <=> att2": False, "att1 IN (att2)": False, "att1 = 9007199254740991.0": True}),
        ({"att1": -(p53 + 1), "att2": -float(p53)}, {"att1 = att2": True, "att2 = att1": True, "att1 < att2": False}),
        # long vs long stays exact
        ({"att1": p53 + 1, "att2": p53}, {"att1 = att2": False, "att1 > att2": True, "att1 <=> att2": False,
                                          "att1 IN (att2)": False, "att1 - att2": 1}),
    ]
    for row, want in cases:
        row = dict({"item": None, "att1": None, "att2": None}, **row)
        for text, exp in want.items():
            got = O._eval(O.OracleParser(text).parse(), row)
            assert got is exp or (got == exp and type(got) is type(exp)), (text, row, got, exp)
    # DECIMAL cells: 7 / 100.0 = 0.07 and -14 / 100.0 = -0.14 (one correctly rounded division: the literal's double);
    # past 2^53, (double) 9007199254740995 = 9007199254740996.0 (tie to the even mantissa) and / 10.0 =
    # 900719925474099.6 -> 900719925474099.625 (doubles there are 0.125 apart), where the exact quotient
    # 900719925474099.5 is a double itself: Spark gives the former
    col = Column("x", N.TYPE_DECIMAL, np.array([7, -14, 1999, 0], dtype=np.int64), decimal_precision=18, decimal_scale=2)
    wide = Column("y", N.TYPE_DECIMAL, np.array([p53 + 3, -(p53 + 3)], dtype=np.int64), decimal_precision=18,
                  decimal_scale=1)
    for cells in ([O._cell(col, i) for i in range(4)], O._pylist(col)):
        assert [float(c) for c in cells] == [0.07, -0.14, 19.99, 0.0]
        assert all(isinstance(c, float) for c in cells)
    for cells in ([O._cell(wide, i) for i in range(2)], O._pylist(wide)):
        assert [float(c) for c in cells] == [900719925474099.625, -900719925474099.625]
    row = {"x": O._pylist(col)[0], "att1": 7}
    for text, exp in {"x = 0.07": True, "x <= 0.07": True, "x IN (0.07)": True, "x * 100 = att1": False,
                      "x RLIKE '^0[.]07$'": True, "x RLIKE '^0[.]07$' AND x * 100 > 7": True}.items():
        got = O._eval(O.OracleParser(text).parse(), row)
        assert got is exp, (text, got, exp)
