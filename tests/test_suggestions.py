"""Constraint suggestion on the host: the rules against known answers (tests/golden/suggestion_kats.json), the JSON
documents, the split definition through the C-ABI's host entry against the `xxhash` package, and the builder's
argument check. No GPU."""
import json
import os
import struct

import pytest
import xxhash

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import suggestions as SG
from deequ_amd.checks import CheckResult, ConstraintResult, is_one

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "suggestion_kats.json")) as _f:
    KATS = json.load(_f)

RULES = {
    "CompleteIfCompleteRule": D.CompleteIfCompleteRule, "RetainCompletenessRule": D.RetainCompletenessRule,
    "RetainTypeRule": D.RetainTypeRule, "CategoricalRangeRule": D.CategoricalRangeRule,
    "FractionalCategoricalRangeRule": D.FractionalCategoricalRangeRule,
    "NonNegativeNumbersRule": D.NonNegativeNumbersRule,
    "UniqueIfApproximatelyUniqueRule": D.UniqueIfApproximatelyUniqueRule,
}


def make_profile(p):
    hist = None
    if p["histogram"] is not None:
        hist = D.Distribution({k: D.DistributionValue(c, r) for k, c, r in p["histogram"]["values"]},
                              p["histogram"]["numberOfBins"])
    common = (p["column"], p["completeness"], p["approximateNumDistinctValues"], p["dataType"],
              p["isDataTypeInferred"], {}, hist)
    if "minimum" in p:
        return D.NumericColumnProfile(*common, None, None, p.get("maximum"), p["minimum"], None, None, None)
    return D.StandardColumnProfile(*common)


def make_rule(spec):
    kwargs = {k: v for k, v in spec.items() if k != "type"}
    return RULES[spec["type"]](**kwargs)


def test_fixture_names_every_rule():
    assert sorted(KATS["rules"]) == sorted(RULES)


@pytest.mark.parametrize("case", KATS["profiles"], ids=lambda c: c["name"])
def test_should_be_applied_for_every_rule(case):
    profile = make_profile(case["profile"])
    for name in KATS["rules"]:
        assert RULES[name]().shouldBeApplied(profile, case["numRecords"]) is (name in case["applies"]), name


@pytest.mark.parametrize("case", KATS["candidates"], ids=lambda c: c["name"])
def test_candidates(case):
    rule = make_rule(case["rule"])
    profile = make_profile(case["profile"])
    assert rule.shouldBeApplied(profile, case["numRecords"])
    s = rule.candidate(profile, case["numRecords"])
    exp = case["expected"]
    assert s.codeForConstraint == exp["codeForConstraint"]
    assert s.currentValue == exp["currentValue"]
    assert s.description == exp["description"]
    assert repr(s.suggestingRule) == exp["suggestingRule"]
    assert s.columnName == case["profile"]["column"] and s.suggestingRule is rule
    if "condition" in exp:  # a compliance constraint: named by the description, over exactly this predicate
        a = s.constraint.inner.analyzer
        assert isinstance(a, D.Compliance)
        assert (a.instance, a.predicate, a.where) == (exp["description"], exp["condition"], None)
        assert s.constraint.inner.hint == exp.get("hint")


def test_constraints_are_the_check_dsl_constraints():
    """Each rule's constraint prints as the same constraint written through Check (its name in the JSON and in a
    VerificationResult)."""
    check = D.Check(D.CheckLevel.Warning, "by hand")
    p = make_profile({"column": "c", "completeness": 0.5, "approximateNumDistinctValues": 100, "dataType": "Integral",
                      "isDataTypeInferred": True, "histogram": None, "minimum": 1.0})
    pairs = [
        (D.CompleteIfCompleteRule(), check.isComplete("c")),
        (D.RetainCompletenessRule(), check.hasCompleteness("c", lambda v: v >= 0.4)),
        (D.NonNegativeNumbersRule(), check.satisfies("c >= 0", "'c' has no negative values")),
        (D.UniqueIfApproximatelyUniqueRule(), check.isUnique("c")),
    ]
    for rule, by_hand in pairs:
        assert repr(rule.candidate(p, 100).constraint) == repr(by_hand.constraints[-1]), rule
    got = D.RetainTypeRule().candidate(p, 100).constraint
    want = check.hasDataType("c", D.ConstrainableDataTypes.Integral).constraints[-1]
    assert type(got) is type(want) and got.analyzer == want.analyzer
    dist = D.Distribution({"Integral": D.DistributionValue(3, 0.75), "Unknown": D.DistributionValue(1, 0.25)}, 2)
    assert got.value_picker(dist) == want.value_picker(dist) == 1.0


def test_bound_assertions():
    """The suggested bound is what the constraint asserts: >= the truncated value."""
    p = make_profile({"column": "c", "completeness": 0.4375, "approximateNumDistinctValues": 1, "dataType": "String",
                      "isDataTypeInferred": False, "histogram": None})
    a = D.RetainCompletenessRule().candidate(p, 672).constraint.inner.assertion
    assert a(0.39) and a(1.0) and not a(0.3899)
    assert D.CompleteIfCompleteRule().candidate(p, 672).constraint.inner.assertion is is_one


def test_round_down_reads_the_shortest_decimal():
    assert SG._round_down_2(0.4) == 0.4
    assert SG._round_down_2(0.39999999999999997) == 0.39
    assert SG._round_down_2(0.3999921883136326) == 0.39
    assert SG._round_down_2(0.402) == 0.4
    assert SG._round_down_2(-0.019) == -0.01  # DOWN is towards zero
    assert SG._round_down_2(1e-5) == 0.0       # Double.toString gives 1.0E-5


def test_escape_java():
    assert SG._escape_java('a"b\\c') == 'a\\"b\\\\c'
    assert SG._escape_java("it's/") == "it's/"
    assert SG._escape_java("\b\n\t\f\r") == "\\b\\n\\t\\f\\r"
    assert SG._escape_java("\x01\x1f\x7f") == "\\u0001\\u001F\x7f"
    assert SG._escape_java("é€") == "\\u00E9\\u20AC"
    assert SG._escape_java("\U0001F600") == "\\uD83D\\uDE00"


def test_default_rules():
    assert [repr(r) for r in D.Rules.DEFAULT] == [
        "CompleteIfCompleteRule()", "RetainCompletenessRule()", "RetainTypeRule()", "CategoricalRangeRule()",
        "FractionalCategoricalRangeRule(0.9)", "NonNegativeNumbersRule()"]


# ---- long IN lists ----------------------------------------------------------------------------------------------------
def in_program(nvalues):
    from deequ_amd.expr import compile_predicate
    text = "`cat` IN (%s)" % ", ".join("'v%d'" % i for i in range(nvalues))
    code = [int(x) for x in compile_predicate(text, {"cat": 0})._code]
    return [(code[i], code[i + 1]) for i in range(0, len(code), 2)]


def stack_depth(program):
    depth = top = 0
    for op, arg in program:
        depth += {N.P_COL: 1, N.P_CONST: 1, N.P_IN: -arg, N.P_OR: -1}[op]
        top = max(top, depth)
    assert depth == 1
    return top


@pytest.mark.parametrize("nvalues", [1, 15, 16, 17, 100, 120])
def test_long_in_lists_fit_the_predicate_stack(nvalues):
    """The rules emit IN lists of up to the histogram threshold's 120 categories; the predicate VM's stack holds 16
    values. Up to 15 constants stay one IN; longer lists run as ORed groups, every constant exactly once, in order."""
    program = in_program(nvalues)
    assert stack_depth(program) <= 16
    assert [arg for op, arg in program if op == N.P_CONST] == list(range(nvalues))
    assert sum(arg for op, arg in program if op == N.P_IN) == nvalues
    ins = sum(1 for op, _ in program if op == N.P_IN)
    assert sum(1 for op, _ in program if op == N.P_OR) == ins - 1
    assert sum(1 for op, _ in program if op == N.P_COL) == ins
    if nvalues <= 15:
        assert ins == 1 and program[-1] == (N.P_IN, nvalues)


# ---- JSON -----------------------------------------------------------------------------------------------------------
FIELDS = {"constraint_name", "column_name", "current_value", "description", "suggesting_rule", "rule_description",
          "code_for_constraint"}


def some_suggestions():
    out = []
    for case in KATS["candidates"][:4]:
        out.append(make_rule(case["rule"]).candidate(make_profile(case["profile"]), case["numRecords"]))
    return out


def test_to_json_fields():
    sugg = some_suggestions()
    doc = json.loads(D.ConstraintSuggestions.toJson(sugg))
    assert list(doc) == ["constraint_suggestions"] and len(doc["constraint_suggestions"]) == len(sugg)
    for j, s in zip(doc["constraint_suggestions"], sugg):
        assert set(j) == FIELDS
        assert j["constraint_name"] == repr(s.constraint) and j["column_name"] == s.columnName
        assert j["current_value"] == s.currentValue and j["description"] == s.description
        assert j["suggesting_rule"] == repr(s.suggestingRule)
        assert j["rule_description"] == s.suggestingRule.ruleDescription
        assert j["code_for_constraint"] == s.codeForConstraint


def test_evaluation_results_to_json_pads_with_unknown():
    sugg = some_suggestions()
    check = D.Check(D.CheckLevel.Warning, "generated constraints", [s.constraint for s in sugg])
    results = [ConstraintResult(sugg[0].constraint, D.ConstraintStatus.Success),
               ConstraintResult(sugg[1].constraint, D.ConstraintStatus.Failure, "no")]
    vr = D.VerificationResult(D.CheckStatus.Warning, {check: CheckResult(check, D.CheckStatus.Warning, results)}, {})
    doc = json.loads(D.ConstraintSuggestions.evaluationResultsToJson(sugg, vr))
    rows = doc["constraint_suggestions"]
    assert [set(j) for j in rows] == [FIELDS | {"constraint_result_on_test_set"}] * len(sugg)
    assert [j["constraint_result_on_test_set"] for j in rows] == ["Success", "Failure", "Unknown", "Unknown"]
    assert [j["code_for_constraint"] for j in rows] == [s.codeForConstraint for s in sugg]
    # a result without a verification run: every suggestion Unknown
    res = D.ConstraintSuggestionResult({}, 0, {"a": sugg[:2], "b": sugg[2:]}, None)
    doc = json.loads(D.ConstraintSuggestionResult.getEvaluationResultsAsJson(res))
    assert [j["constraint_result_on_test_set"] for j in doc["constraint_suggestions"]] == ["Unknown"] * len(sugg)
    doc = json.loads(D.ConstraintSuggestionResult.getConstraintSuggestionsAsJson(res))
    assert [j["code_for_constraint"] for j in doc["constraint_suggestions"]] == [s.codeForConstraint for s in sugg]


# ---- the split definition ---------------------------------------------------------------------------------------------
def model_is_test(g, seed, ratio):
    return (xxhash.xxh64_intdigest(struct.pack("<q", g), seed=seed) >> 11) < int(ratio * 2 ** 53)


@pytest.mark.parametrize("row0", [0, 2 ** 32 - 100])
@pytest.mark.parametrize("seed", [0, 2 ** 64 - 1, 42])
def test_split_row_is_test_matches_xxhash(seed, row0):
    for ratio in (0.1, 0.5):
        got = [N.split_row_is_test(g, seed, ratio) for g in range(row0, row0 + 10000)]
        assert got == [int(model_is_test(g, seed, ratio)) for g in range(row0, row0 + 10000)]
        assert 0 < sum(got) < 10000


def test_split_row_is_test_rejects_bad_arguments():
    for ratio in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert N.split_row_is_test(5, 1, ratio) < 0
    assert N.split_row_is_test(-1, 1, 0.5) < 0
    assert N.split_row_is_test(2 ** 63 - 1, 1, 0.5) in (0, 1)


def test_split_symbols_are_exported():
    assert {"dq_split_rows", "dq_split_row_is_test"} <= set(N.EXPORTED_SYMBOLS)
    assert N.load_library().dq_abi_version() == 2


# ---- builder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0, 1, 0.0, 1.0, -0.1, 1.5])
def test_builder_rejects_bad_testset_ratio(ratio):
    t = D.Table.from_pydict({"a": [1, 2, 3]})
    b = D.ConstraintSuggestionRunner().onData(t).addConstraintRules(D.Rules.DEFAULT) \
        .useTrainTestSplitWithTestsetRatio(ratio, 0)
    with pytest.raises(ValueError, match=r"^Testset ratio must be in \]0, 1\[$"):
        b.run()
    with pytest.raises(ValueError, match=r"^Testset ratio must be in \]0, 1\[$"):
        D.split_train_test(t, ratio, 0)


def test_builder_is_fluent():
    t = D.Table.from_pydict({"a": [1, 2, 3]})
    b = D.ConstraintSuggestionRunner().onData(t)
    for call in (lambda: b.addConstraintRule(D.CompleteIfCompleteRule()), lambda: b.addConstraintRules(D.Rules.DEFAULT),
                 lambda: b.printStatusUpdates(False), lambda: b.cacheInputs(True),
                 lambda: b.useTrainTestSplitWithTestsetRatio(0.2), lambda: b.withLowCardinalityHistogramThreshold(10),
                 lambda: b.restrictToColumns(["a"]), lambda: b.setKLLParameters(None),
                 lambda: b.setPredefinedTypes({}), lambda: b.saveColumnProfilesJsonToPath("p.json"),
                 lambda: b.saveConstraintSuggestionsJsonToPath("s.json"),
                 lambda: b.saveEvaluationResultsJsonToPath("e.json"), lambda: b.overwritePreviousFiles(True)):
        assert call() is b
