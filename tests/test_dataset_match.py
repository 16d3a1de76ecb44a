"""Cross-table checks, the part that needs no GPU: the state algebra, the refusals that must be decided
before any device work (a missing column, an empty primary, a type pair the probe does not compare), analyzer equality
and repr, the constraint Check.doesDatasetMatch builds, and the C-ABI declaration."""
from decimal import Decimal

import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import comparison as C
from deequ_amd import engine
from deequ_amd.checks import is_one
from deequ_amd.table import Table
import join_model as M


@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to reach the device fails the test."""
    def refuse(*a, **k):
        raise AssertionError("this call must be decided without a device context")
    monkeypatch.setattr(engine, "ctx", refuse)
    monkeypatch.setattr(engine, "frequencies", refuse)
    monkeypatch.setattr(N, "context", refuse)


def _orders():
    return Table.from_pydict({"customer_id": [1, 2, None, 4], "note": ["a", "b", "c", None]},
                             types={"customer_id": "long", "note": "string"})


def _customers():
    return Table.from_pydict({"id": [1, 2, 3], "name": ["a", "b", "x"]}, types={"id": "int", "name": "string"})


# ---- the model itself ----------------------------------------------------------------------------------------------
def test_model_semantics():
    ref = [(7, None), (7, "x"), (None, None), (1, "")]
    assert M.hits([(7, None), (7, "x"), (None, None), (1, ""), (1, None), (2, "x")], ref) == \
        [False, True, False, True, False, False]
    assert M.groups_and_rows([(None,), (None,), (1,)]) == (2, 3)
    assert M.keys_unique([(None, None), (1, None), (None, 1)]) and not M.keys_unique([(None, None), (None, None)])
    assert M.bitmap([True] + [False] * 63 + [True]) == b"\x01" + b"\x00" * 7 + b"\x01" + b"\x00" * 7
    assert M.bitmap([]) == b""


# ---- state algebra -------------------------------------------------------------------------------------------------
def test_state_adds_both_members_and_divides():
    a, b = D.DatasetMatchState(3, 4), D.DatasetMatchState(1, 6)
    s = a.sum(b)
    from deequ_amd.states import DoubleValuedState
    assert isinstance(s, DoubleValuedState)
    assert (s.matchedDataCount, s.totalDataCount) == (4, 10) and s == D.DatasetMatchState(4, 10)
    assert s.metricValue() == 0.4 and a.metricValue() == 0.75
    assert a.sum(b) == b.sum(a) and a.sum(b).sum(a) == a.sum(b.sum(a))
    assert D.DatasetMatchState(0, 0).metricValue() != D.DatasetMatchState(0, 0).metricValue()  # NaN: nothing to divide
    assert repr(s) == "DatasetMatchState(4,10)" and a != D.DatasetMatchState(3, 5)


def test_state_goes_through_the_in_memory_provider():
    from deequ_amd.analyzers import merge
    ref = _customers()
    a = D.DatasetMatchAnalyzer(ref, {"customer_id": "id"})
    p, q, out = D.InMemoryStateProvider(), D.InMemoryStateProvider(), D.InMemoryStateProvider()
    p.persist(a, D.DatasetMatchState(2, 3))
    q.persist(a, D.DatasetMatchState(5, 7))
    a.aggregateStateTo(p, q, out)
    assert out.load(a) == D.DatasetMatchState(7, 10) == merge(p.load(a), None, q.load(a))
    m = a.loadStateAndComputeMetric(out)
    assert m.value.get() == 0.7 and (m.name, m.instance, m.entity) == ("DatasetMatch", "customer_id", D.Entity.Dataset)


# ---- refusals that need no device ----------------------------------------------------------------------------------
def test_missing_column_names_the_column_and_the_side(no_context):
    r = D.ReferentialIntegrity.subsetCheck(_orders(), "customer", _customers(), "id")
    assert isinstance(r, D.ComparisonFailed) and "customer" in r.errorMessage and "primary" in r.errorMessage
    assert r.ratio == 0.0
    r = D.ReferentialIntegrity.subsetCheck(_orders(), ["customer_id"], _customers(), ["ident"])
    assert isinstance(r, D.ComparisonFailed) and "ident" in r.errorMessage and "reference" in r.errorMessage
    r = D.DataSynchronization.columnMatch(_orders(), _customers(), {"customer_id": "id"}, {"note": "nome"})
    assert isinstance(r, D.ComparisonFailed) and "nome" in r.errorMessage and "reference" in r.errorMessage
    r = D.DataSynchronization.columnMatchRowLevel(_orders(), _customers(), {"cid": "id"})
    assert isinstance(r, D.ComparisonFailed) and "cid" in r.errorMessage and "primary" in r.errorMessage
    r = D.ReferentialIntegrity.subsetCheckRowLevel(_orders(), "customer_id", _customers(), ["id", "name"])
    assert isinstance(r, D.ComparisonFailed)  # one column against two


def test_empty_primary_is_a_failure_not_a_nan(no_context):
    empty = Table.from_pydict({"customer_id": []}, types={"customer_id": "long"})
    seen = []
    r = D.ReferentialIntegrity.subsetCheck(empty, "customer_id", _customers(), "id", assertion=seen.append)
    assert isinstance(r, D.ComparisonFailed) and "empty" in r.errorMessage and "primary" in r.errorMessage
    r = D.DataSynchronization.columnMatch(empty, _customers(), {"customer_id": "id"}, assertion=seen.append)
    assert isinstance(r, D.ComparisonFailed) and "empty" in r.errorMessage
    assert seen == []  # no ratio, NaN or other, reached the assertion


@pytest.mark.parametrize("ptype, pvals, rtype, rvals, words", [
    ("double", [1.0, 2.0], "double", [1.0], ["k", "DoubleType"]),
    ("float", [1.0, 2.0], "float", [1.0], ["k", "FloatType"]),
    ("long", [1, 2], "double", [1.0], ["r", "DoubleType"]),
    ("decimal(38,4)", [Decimal("1.5"), Decimal("2.5")], "decimal(38,4)", [Decimal("1.5")], ["k", "DecimalType(38,4)"]),
    ("decimal", [Decimal("1.25"), Decimal("2.50")], "decimal", [Decimal("1.250")], ["DecimalType", "scale"]),
    ("string", ["1", "2"], "long", [1], ["k", "StringType", "LongType"]),
    ("long", [1, 2], "date", [1], ["LongType", "DateType"]),
    ("boolean", [True, False], "byte", [1], ["BooleanType", "ByteType"]),
])
def test_type_pairs_the_probe_does_not_compare(no_context, ptype, pvals, rtype, rvals, words):
    p = Table.from_pydict({"k": pvals}, types={"k": ptype})
    r = Table.from_pydict({"r": rvals}, types={"r": rtype})
    for res in (D.ReferentialIntegrity.subsetCheck(p, "k", r, "r"),
                D.ReferentialIntegrity.subsetCheckRowLevel(p, "k", r, "r"),
                D.DataSynchronization.columnMatch(p, r, {"k": "r"}),
                D.DataSynchronization.columnMatchRowLevel(p, r, {"k": "r"})):
        assert isinstance(res, D.ComparisonFailed), res
        for w in words:
            assert w in res.errorMessage, (w, res.errorMessage)
    a = D.DatasetMatchAnalyzer(r, {"k": "r"})
    m = a.calculate(p)
    assert m.value.isFailure and isinstance(m.value.failed, D.metrics.UnsupportedOnDevice)
    assert all(w in str(m.value.failed) for w in words)


@pytest.mark.parametrize("ptype, rtype", [("byte", "long"), ("short", "int"), ("long", "byte"), ("int", "int"),
                                          ("string", "string"), ("date", "date"), ("boolean", "boolean"),
                                          ("timestamp", "timestamp")])
def test_type_pairs_the_probe_compares(ptype, rtype):
    val = {"string": "a", "boolean": True}
    p = Table.from_pydict({"k": [val.get(ptype, 1)]}, types={"k": ptype})
    r = Table.from_pydict({"r": [val.get(rtype, 1)]}, types={"r": rtype})
    assert C.pair_refusal("k", p["k"], "r", r["r"]) is None


def test_equal_decimal_scales_are_accepted():
    p = Table.from_pydict({"k": [Decimal("1.25")]}, types={"k": "decimal"})
    r = Table.from_pydict({"r": [Decimal("7.50")]}, types={"r": "decimal"})
    assert C.pair_refusal("k", p["k"], "r", r["r"]) is None


# ---- analyzer value semantics ---------------------------------------------------------------------------------------
def test_analyzer_equality_is_the_dataset_identity_plus_the_mappings():
    ref, twin = _customers(), _customers()
    a = D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}, is_one)
    assert a == D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}, lambda v: v > 0.5)
    assert hash(a) == hash(D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}))
    assert a != D.DatasetMatchAnalyzer(twin, {"customer_id": "id"})  # equal contents, another dataset
    assert a != D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}, is_one, {"note": "name"})
    assert a != D.DatasetMatchAnalyzer(ref, {"note": "name"})
    assert len({a, D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}), D.DatasetMatchAnalyzer(twin, {"customer_id": "id"})}) == 2
    assert repr(a) == "DatasetMatchAnalyzer(Map(customer_id -> id),None)"
    b = D.DatasetMatchAnalyzer(ref, {"customer_id": "id", "x": "y"}, is_one, {"note": "name"})
    assert repr(b) == "DatasetMatchAnalyzer(Map(customer_id -> id, x -> y),Some(Map(note -> name)))"
    assert (b.name, b.instance, b.entity) == ("DatasetMatch", "customer_id,x", D.Entity.Dataset)


def test_analyzer_preconditions_need_the_mapped_columns_on_both_sides(no_context):
    from deequ_amd.analyzers import Preconditions
    ref, data = _customers(), _orders()
    ok = D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}, is_one, {"note": "name"})
    assert Preconditions.findFirstFailing(data.schema, ok.preconditions()) is None
    for a, word in ((D.DatasetMatchAnalyzer(ref, {"cid": "id"}), "cid"),
                    (D.DatasetMatchAnalyzer(ref, {"customer_id": "ident"}), "ident"),
                    (D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}, is_one, {"note": "nome"}), "nome"),
                    (D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}, is_one, {"remark": "name"}), "remark")):
        e = Preconditions.findFirstFailing(data.schema, a.preconditions())
        assert isinstance(e, D.NoSuchColumnException) and word in str(e)
        m = a.calculate(data)
        assert m.value.isFailure and word in str(m.value.failed) and m.entity == D.Entity.Dataset


# ---- the check ------------------------------------------------------------------------------------------------------
def test_does_dataset_match_builds_one_constraint_over_the_analyzer():
    ref = _customers()

    def at_least_half(v):
        return v >= 0.5
    check = D.Check(D.CheckLevel.Error, "sync").doesDatasetMatch(ref, {"customer_id": "id"}, at_least_half,
                                                                {"note": "name"}, hint="keep in sync")
    assert len(check.constraints) == 1
    a = D.DatasetMatchAnalyzer(ref, {"customer_id": "id"}, at_least_half, {"note": "name"})
    assert list(check.requiredAnalyzers()) == [a]
    assert repr(check.constraints[0]) == "DatasetMatchConstraint(%r)" % a
    metric = D.DoubleMetric(D.Entity.Dataset, "DatasetMatch", "customer_id", D.Success(0.75))
    assert check.constraints[0].evaluate({a: metric}).status == D.ConstraintStatus.Success
    low = D.DoubleMetric(D.Entity.Dataset, "DatasetMatch", "customer_id", D.Success(0.25))
    res = check.constraints[0].evaluate({a: low})
    assert res.status == D.ConstraintStatus.Failure and "0.25" in res.message and "keep in sync" in res.message
    assert check.evaluate(D.AnalyzerContext({a: low})).status == D.CheckStatus.Error


# ---- the C-ABI ------------------------------------------------------------------------------------------------------
def test_probe_is_declared_and_exported():
    assert "dq_freq_probe" in N.EXPORTED_SYMBOLS
    lib = N.load_library()
    assert hasattr(lib, "dq_freq_probe") and lib.dq_freq_probe.restype is not None
    assert N.SCAN_KERNELS[-1] == "freq_probe" and len(N.SCAN_KERNELS) == 18
    assert callable(N.Context.freq_probe) and callable(engine.FrequencyTable.probe)
    assert lib.dq_abi_version() == 2
