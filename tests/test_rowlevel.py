"""Row-level results on the host: the term planner (which constraint becomes which term, what is ignored, what is
skipped and why), the name checks, and the numpy model of the contract against a hand-written example. No GPU."""
import numpy as np
import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd.metrics import Entity, Failure, UnsupportedOnDevice
from deequ_amd.rowlevel import check_names, plan_row_level, row_level_results
from deequ_amd.table import Table
import rowlevel_model as M


def _table():
    return Table.from_pydict({"id": [1, 2, 2, None], "s": ["a", "bb", None, "a"], "x": [1.0, None, -2.0, 3.0],
                              "y": [2.0, 2.0, 2.0, 2.0], "f": [1, 0, None, 2]},
                             types={"id": "long", "s": "string", "x": "double", "y": "double", "f": "long"})


def _one(_):
    return True


def _every_check_method():
    """A check per family of Check methods; `row` holds every method with a row-level form, `agg` every other one."""
    E = D.CheckLevel.Error
    row = (D.Check(E, "row")
           .isComplete("x").hasCompleteness("s", _one).where("f > 0")
           .satisfies("x > 0", "x positive").where("f > 0")
           .isContainedIn("s", ["a", "bb"]).isContainedIn("x", lowerBound=0, upperBound=5)
           .isNonNegative("x").isPositive("x")
           .isLessThan("x", "y").isLessThanOrEqualTo("x", "y").isGreaterThan("y", "x").isGreaterThanOrEqualTo("y", "x")
           .hasPattern("s", r"^a").where("f > 0")
           .containsCreditCardNumber("s").containsEmail("s").containsURL("s").containsSocialSecurityNumber("s")
           .isUnique("id").isPrimaryKey("id", "s").where("f > 0").hasUniqueness(["id"], _one)
           .hasUniqueValueRatio(["s"], _one))
    agg = (D.Check(E, "agg")
           .hasSize(_one).hasMin("x", _one).hasMax("x", _one).hasMean("x", _one).hasSum("x", _one)
           .hasStandardDeviation("x", _one).hasMinLength("s", _one).hasMaxLength("s", _one)
           .hasApproxCountDistinct("id", _one).hasCorrelation("x", "y", _one).hasDataType("s", D.ConstrainableDataTypes.String)
           .hasDistinctness(["id"], _one).hasNumberOfDistinctValues("s", _one).hasHistogramValues("s", _one)
           .hasEntropy("s", _one).hasMutualInformation("id", "s", _one).hasApproxQuantile("x", 0.5, _one))
    return row, agg


def test_plan_maps_every_check_method():
    row, agg = _every_check_method()
    plan = plan_row_level([agg, row], _table(), {})
    assert plan.descriptions == ["row"] and plan.skipped == []  # `agg` has no row-level form: no column, not skipped
    assert len(plan.terms) == len(row.constraints) == 20
    kinds = [t.kind for t in plan.terms]
    assert kinds == [N.ROW_NOT_NULL] * 2 + [N.ROW_PREDICATE] * 14 + [N.ROW_BITS] * 4
    assert all(t.check == 0 and t.description == "row" for t in plan.terms)
    assert [t.constraint for t in plan.terms] == row.constraints
    assert (plan.terms[0].column, plan.terms[0].where) == ("x", -1)
    w = plan.batch.pred_index["f > 0"]
    assert (plan.terms[1].column, plan.terms[1].where) == ("s", w)
    assert plan.terms[2].where == w and plan.terms[11].where == w
    assert plan.terms[2].predicate == plan.batch.pred_index["x > 0"]
    # PatternMatch is the [COL, REGEX] program
    code = plan.batch.preds[plan.terms[11].predicate].to_native()
    assert code.code_len == 4
    assert [(t.columns, t.where_text) for t in plan.terms[16:]] == [(["id"], None), (["id", "s"], "f > 0"), (["id"], None),
                                                                     (["s"], None)]
    assert isinstance(plan.terms[19].analyzer, D.UniqueValueRatio)


def test_plan_compiles_a_shared_text_once():
    E = D.CheckLevel.Error
    a = D.Check(E, "a").satisfies("f > 0", "f positive").isComplete("x").where("f > 0")
    b = D.Check(E, "b").satisfies("f > 0", "again").where("x > 0").hasPattern("s", "a").hasPattern("s", "a").where("f > 0")
    plan = plan_row_level([a, b], _table(), {})
    assert plan.descriptions == ["a", "b"] and [t.check for t in plan.terms] == [0, 0, 1, 1, 1]
    assert len(plan.batch.preds) == 3  # "f > 0", "x > 0" and the regex, however often they are named
    p = plan.batch.pred_index["f > 0"]
    assert plan.terms[0].predicate == p and plan.terms[1].where == p and plan.terms[2].predicate == p
    assert plan.terms[4].where == p and plan.terms[3].predicate == plan.terms[4].predicate


def test_plan_skips_what_cannot_be_evaluated():
    E = D.CheckLevel.Error
    check = (D.Check(E, "c").isComplete("x").satisfies("x >", "broken").hasPattern("s", "(a").isComplete("nope")
             .satisfies("x > 0", "fine").hasMean("x", _one))
    failed = check.constraints[0].inner.analyzer
    metrics = {failed: D.DoubleMetric(Entity.Column, "Completeness", "x", Failure(RuntimeError("boom")))}
    plan = plan_row_level([check], _table(), metrics)
    assert plan.descriptions == ["c"]
    assert [t.constraint for t in plan.terms] == [check.constraints[4]]
    assert [(d, c) for d, c, _ in plan.skipped] == [("c", k) for k in check.constraints[:4]]
    reasons = [r for _, _, r in plan.skipped]
    assert "boom" in reasons[0] and all(reasons)
    for bad in (check.constraints[0], check.constraints[1], check.constraints[2]):
        with pytest.raises(UnsupportedOnDevice):
            plan_row_level([D.Check(E, "c", [bad])], _table(), metrics, strict=True)
    # uniqueness over a ChunkedTable: a group spans chunks
    u = D.Check(E, "u").isUnique("id").isComplete("x")
    plan = plan_row_level([u], _table(), {}, chunked=True)
    assert [t.kind for t in plan.terms] == [N.ROW_NOT_NULL] and [c for _, c, _ in plan.skipped] == [u.constraints[0]]
    with pytest.raises(UnsupportedOnDevice):
        plan_row_level([u], _table(), {}, strict=True, chunked=True)


def test_names_are_checked_before_any_work():
    E = D.CheckLevel.Error
    t = _table()
    with pytest.raises(ValueError, match="two checks"):
        check_names([D.Check(E, "a").isComplete("x"), D.Check(E, "a").isComplete("s")], t)
    with pytest.raises(ValueError, match="column of the data"):
        check_names([D.Check(E, "x").isComplete("x")], t)
    result = D.VerificationResult(D.CheckStatus.Success, {D.Check(E, "s").isComplete("x"): None}, {})
    with pytest.raises(ValueError, match="column of the data"):
        D.VerificationResult.rowLevelResultsAsTable(result, t)
    with pytest.raises(ValueError, match="filteredRow"):
        row_level_results(result, t, filteredRow="false")
    assert D.RowLevelResults is not None


def test_model_on_a_hand_written_example():
    """8 rows, one check of three terms (T = passes, F = fails, - = not considered):
         row            0  1  2  3  4  5  6  7
         not null       T  F  T  T  F  T  T  T
         p, where w     T  -  F  -  -  T  -  F
         unique         T  T  T  F  F  -  -  -
       true mode        T  F  F  F  F  T  T  F
       null mode        T  F  F  F  F  N  N  F      (row 1: FALSE and NULL = FALSE)"""
    T, F = True, False
    nn = (0, np.array([T, F, T, T, F, T, T, T]), np.ones(8, dtype=bool))
    pw = (0, np.array([T, T, F, F, T, T, F, F]), np.array([T, F, T, F, F, T, F, T]))
    un = (0, np.array([T, T, T, F, F, F, F, F]), np.array([T, T, T, T, T, F, F, F]))
    single = (1, np.array([T, F, T, T, F, T, T, T]), np.array([T, T, F, T, T, T, T, T]))
    counts, (a, b) = M.fold([nn, pw, un, single], 2, 8, False)
    assert counts == [(6, 8), (2, 4), (3, 5), (5, 7)]
    assert a.value.tolist() == [T, F, F, F, F, T, T, F] and a.validity is None
    assert (a.true_rows, a.false_rows, a.null_rows) == (3, 5, 0)
    assert b.value.tolist() == [T, F, T, T, F, T, T, T]
    counts_n, (a, b) = M.fold([nn, pw, un, single], 2, 8, True)
    assert counts_n == counts
    assert a.value.tolist() == [T, F, F, F, F, F, F, F]
    assert a.validity.tolist() == [T, T, T, T, T, F, F, T]
    assert (a.true_rows, a.false_rows, a.null_rows) == (1, 5, 2)
    assert b.value.tolist() == [T, F, F, T, F, T, T, T] and b.validity.tolist() == [T, T, F, T, T, T, T, T]


def test_model_terms_read_the_oracle():
    """The term builders over the 4-row table: `f > 0` is TRUE on rows 0 and 3 (NULL on row 2)."""
    t = _table()
    T, F = True, False

    def rows(term):
        return term[0], term[1].tolist(), term[2].tolist()
    assert rows(M.term_not_null(0, t, "s", "f > 0")) == (0, [T, T, F, T], [T, F, F, T])
    assert rows(M.term_predicate(1, t, "x > 0")) == (1, [T, F, F, T], [T, T, T, T])  # NULL x: not TRUE
    assert rows(M.term_pattern(0, t, "s", "^a")) == (0, [T, F, F, T], [T, T, T, T])  # NULL s fails
    assert rows(M.term_unique(2, t, ["id"])) == (2, [T, F, F, F], [T, T, T, F])  # NULL key: not considered
    assert M.group_counts(t, ["id", "s"], "f > 0").tolist() == [1, 0, 0, 1]  # row 3: (NULL, "a") takes part
    assert M.group_counts(t, ["id"], "f > 0").tolist() == [1, 0, 0, 0]
