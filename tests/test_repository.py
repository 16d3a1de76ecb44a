"""Metrics repositories (deequ_amd/repository.py), the runner hooks that use them and the anomaly check of a
verification run, on the host: AnalysisResultSerde per analyzer class and metric kind, a hand-written document in
the reference's wire format, both stores through one suite, and the cases of the reference's AnalysisResultTest and
MetricsRepositoryMultipleResultsLoaderTest kept as data in tests/golden/repository_kats.json. The runner-hook tests
run AnalysisRunner.doAnalysisRun over a host table with an analyzer that counts on the host, so no GPU is needed."""
import json
import os
import threading

import pytest

import deequ_amd as D
from deequ_amd.analyzers import Analyzer
from deequ_amd.metrics import (DoubleMetric, Entity, Failure, Success, HistogramMetric, KeyedDoubleMetric,
                               Distribution, DistributionValue)
from deequ_amd.runners import AnalyzerContext
from deequ_amd.table import Table
from helpers import analyzer_from_spec

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repository_kats.json")) as f:
    KATS = json.load(f)

DATE_ONE, DATE_TWO = KATS["dates"]["DATE_ONE"], KATS["dates"]["DATE_TWO"]


def metric(value, name="Completeness", instance="ColumnA", entity=Entity.Column):
    return DoubleMetric(entity, name, instance, Success(value))


def fixture_context():
    """The metrics the reference's repository tests compute over their fixture table."""
    return AnalyzerContext({analyzer_from_spec(spec): DoubleMetric(Entity(entity), name, instance, Success(value))
                            for spec, entity, name, instance, value in KATS["metrics"]})


def same_rows(text, expected):
    """The reference's assertSameJson: the same rows, in any order."""
    def canon(rows):
        return sorted(json.dumps(r, sort_keys=True) for r in rows)
    assert canon(json.loads(text)) == canon(expected)


# ---- serde ----------------------------------------------------------------------------------------------------------------
ANALYZERS = [
    D.Size(), D.Size("a > 1"),
    D.Completeness("ColumnA"), D.Completeness("ColumnA", "b = 2"),
    D.Compliance("rule1", "att1 > 3"), D.Compliance("rule1", "att1 > 3", "att2 < 1"),
    D.PatternMatch("ColumnA", D.Patterns.EMAIL), D.PatternMatch("ColumnA", r"\d+", "b = 2"),
    D.Sum("ColumnA"), D.Sum("ColumnA", "w"), D.Mean("ColumnA"), D.Mean("ColumnA", "w"),
    D.Minimum("ColumnA"), D.Minimum("ColumnA", "w"), D.Maximum("ColumnA"), D.Maximum("ColumnA", "w"),
    D.CountDistinct(["columnA", "columnB"]), D.CountDistinct(["columnA"], "w"),
    D.Distinctness(["columnA", "columnB"]), D.Distinctness(["columnA"], "w"),
    D.Entropy("ColumnA"), D.Entropy("ColumnA", "w"),
    D.MutualInformation(["ColumnA", "ColumnB"]), D.MutualInformation(["ColumnA", "ColumnB"], "w"),
    D.UniqueValueRatio(["columnA", "columnB"]), D.UniqueValueRatio(["columnA"], "w"),
    D.Uniqueness("ColumnA"), D.Uniqueness(["ColumnA", "ColumnB"]), D.Uniqueness(["ColumnA"], "w"),
    D.Histogram("ColumnA"), D.Histogram("ColumnA", None, 5),
    D.DataType("ColumnA"), D.DataType("ColumnA", "w"),
    D.ApproxCountDistinct("columnA"), D.ApproxCountDistinct("columnA", "test"),
    D.Correlation("firstColumn", "secondColumn"), D.Correlation("firstColumn", "secondColumn", "test"),
    D.StandardDeviation("ColumnA"), D.StandardDeviation("ColumnA", "w"),
    D.ApproxQuantile("col", 0.5, relativeError=0.2), D.ApproxQuantile("col", 0.5), D.ApproxQuantile("col", 0.25, where="w"),
    D.ApproxQuantiles("col", [0.25, 0.5, 0.75], relativeError=0.2), D.ApproxQuantiles("col", [0.1]),
    D.MinLength("ColumnA"), D.MinLength("ColumnA", "w"), D.MaxLength("ColumnA"), D.MaxLength("ColumnA", "w"),
]


def test_every_serializable_analyzer_class_is_covered():
    from deequ_amd import repository
    assert {type(a) for a in ANALYZERS} == set(repository._WRITERS)
    assert {type(a).__name__ for a in ANALYZERS} == set(repository._READERS)


@pytest.mark.parametrize("analyzer", ANALYZERS, ids=[repr(a)[:40] for a in ANALYZERS])
def test_analyzer_survives_the_serde_as_an_equal_object(analyzer):
    result = D.AnalysisResult(D.ResultKey(DATE_ONE, {"Region": "EU"}), AnalyzerContext({analyzer: metric(5.0)}))
    text = D.AnalysisResultSerde.serialize([result])
    (back,) = D.AnalysisResultSerde.deserialize(text)
    (restored,) = back.analyzerContext.metricMap
    assert restored == analyzer and hash(restored) == hash(analyzer) and repr(restored) == repr(analyzer)
    assert type(restored) is type(analyzer)
    assert back == result
    wire = json.loads(text)[0]["analyzerContext"]["metricMap"][0]["analyzer"]
    assert wire["analyzerName"] == type(analyzer).__name__
    # an absent filter is left out (gson drops the reference's null property), a present one is under `where`
    assert ("where" in wire) == (getattr(analyzer, "where", None) is not None)
    if "where" in wire:
        assert wire["where"] == analyzer.where


METRICS = [
    metric(5.0, "Size", "*", Entity.Dataset), metric(0.1 + 0.2), metric(float("nan")), metric(-1e-300),
    metric(0.25, "Uniqueness", "a,b", Entity.Mutlicolumn),
    HistogramMetric("ColumnA", Success(Distribution({"some": DistributionValue(10, 0.5)}, 10))),
    HistogramMetric("ColumnA", Success(Distribution({"some": DistributionValue(10, 0.5),
                                                     "other": DistributionValue(0, 0.0)}, 10))),
    HistogramMetric("ColumnA", Success(Distribution({}, 0))),
    KeyedDoubleMetric(Entity.Column, "ApproxQuantiles", "col", Success({"0.25": 10.0, "0.5": 20.0, "0.75": 30.0})),
    KeyedDoubleMetric(Entity.Column, "ApproxQuantiles", "col", Success({})),
]


@pytest.mark.parametrize("m", METRICS, ids=[type(m).__name__ + str(i) for i, m in enumerate(METRICS)])
def test_metric_survives_the_serde_as_an_equal_object(m):
    result = D.AnalysisResult(D.ResultKey(0), AnalyzerContext({D.Completeness("ColumnA"): m}))
    (back,) = D.AnalysisResultSerde.deserialize(D.AnalysisResultSerde.serialize([result]))
    (restored,) = back.analyzerContext.metricMap.values()
    assert type(restored) is type(m) and restored == m
    assert (restored.entity, restored.name, restored.instance) == (m.entity, m.name, m.instance)
    assert back == result


def test_wire_format_field_for_field():
    """The reference's field names (AnalysisResultSerde.scala): what its deserializer reads."""
    ctx = AnalyzerContext({
        D.Correlation("a", "b", "t"): metric(0.5, "Correlation", "a,b", Entity.Mutlicolumn),
        D.Histogram("h", None, 7): HistogramMetric("h", Success(Distribution({"x": DistributionValue(3, 0.75)}, 2))),
        D.ApproxQuantiles("q", [0.25, 0.5], 0.2): KeyedDoubleMetric(Entity.Column, "ApproxQuantiles", "q",
                                                                    Success({"0.25": 1.0, "0.5": 2.0})),
        D.ApproxQuantile("q", 0.5, 0.2): metric(2.0, "ApproxQuantile-0.5", "q"),
        D.Compliance("rule", "x > 1"): metric(1.0, "Compliance", "rule"),
        D.PatternMatch("p", r"\d"): metric(1.0, "PatternMatch", "p"),
        D.Uniqueness(["a", "b"]): metric(1.0, "Uniqueness", "a,b", Entity.Mutlicolumn)})
    doc = json.loads(D.AnalysisResultSerde.serialize([D.AnalysisResult(D.ResultKey(12, {"k": "v"}), ctx)]))
    assert list(doc[0]) == ["resultKey", "analyzerContext"]
    assert doc[0]["resultKey"] == {"dataSetDate": 12, "tags": {"k": "v"}}
    entries = doc[0]["analyzerContext"]["metricMap"]
    assert [list(e) for e in entries] == [["analyzer", "metric"]] * 7
    assert [e["analyzer"] for e in entries] == [
        {"analyzerName": "Correlation", "firstColumn": "a", "secondColumn": "b", "where": "t"},
        {"analyzerName": "Histogram", "column": "h", "maxDetailBins": 7},
        {"analyzerName": "ApproxQuantiles", "column": "q", "quantiles": "0.25,0.5", "relativeError": 0.2},
        {"analyzerName": "ApproxQuantile", "column": "q", "quantile": 0.5, "relativeError": 0.2},
        {"analyzerName": "Compliance", "instance": "rule", "predicate": "x > 1"},
        {"analyzerName": "PatternMatch", "column": "p", "pattern": r"\d"},
        {"analyzerName": "Uniqueness", "columns": ["a", "b"]}]
    assert entries[0]["metric"] == {"metricName": "DoubleMetric", "entity": "Mutlicolumn", "instance": "a,b",
                                    "name": "Correlation", "value": 0.5}
    assert entries[1]["metric"] == {"metricName": "HistogramMetric", "column": "h", "numberOfBins": 2,
                                    "value": {"numberOfBins": 2, "values": {"x": {"absolute": 3, "ratio": 0.75}}}}
    assert entries[2]["metric"] == {"metricName": "KeyedDoubleMetric", "entity": "Column", "instance": "q",
                                    "name": "ApproxQuantiles", "value": {"0.25": 1.0, "0.5": 2.0}}


def test_document_in_the_reference_format_loads_to_the_expected_context():
    first, second = D.AnalysisResultSerde.deserialize(json.dumps(KATS["wire_document"]))
    assert first.resultKey == D.ResultKey(DATE_ONE, {"Region": "EU"})
    assert second == D.AnalysisResult(D.ResultKey(DATE_TWO), AnalyzerContext.empty())
    expected = AnalyzerContext({
        D.Size(): metric(5.0, "Size", "*", Entity.Dataset),
        D.Completeness("ColumnA", "b > 1"): metric(0.5),
        D.Compliance("rule1", "att1 > 3"): metric(0.25, "Compliance", "rule1"),
        D.Uniqueness(["ColumnA", "ColumnB"]): metric(1.0, "Uniqueness", "ColumnA,ColumnB", Entity.Mutlicolumn),
        D.Correlation("a", "b", "test"): metric(-0.5, "Correlation", "a,b", Entity.Mutlicolumn),
        D.Histogram("ColumnA", None, 5): HistogramMetric("ColumnA", Success(Distribution(
            {"some": DistributionValue(10, 0.5), "other": DistributionValue(0, 0.0)}, 10))),
        D.ApproxQuantile("col", 0.5, 0.2): metric(0.5, "ApproxQuantile-0.5", "col"),
        D.ApproxQuantiles("col", [0.25, 0.5, 0.75], 0.2): KeyedDoubleMetric(
            Entity.Column, "ApproxQuantiles", "col", Success({"0.25": 10.0, "0.5": 20.0, "0.75": 30.0})),
        D.PatternMatch("ColumnA", r"\d+"): metric(1.0, "PatternMatch", "ColumnA")})
    assert first.analyzerContext == expected
    assert list(first.analyzerContext.metricMap) == list(expected.metricMap)  # document order
    # and what is written for it is the document again
    assert json.loads(D.AnalysisResultSerde.serialize([first, second])) == KATS["wire_document"]


def test_unknown_names_are_refused():
    with pytest.raises(ValueError, match="Unable to deserialize analyzer KLLSketch"):
        D.AnalysisResultSerde.analyzer_from_json({"analyzerName": "KLLSketch", "column": "x"})
    with pytest.raises(ValueError, match="Unable to deserialize analyzer KLLMetric"):
        D.AnalysisResultSerde.metric_from_json({"metricName": "KLLMetric"})


def test_failed_metrics_are_not_serialized_and_not_saved(tmp_path):
    failed = DoubleMetric(Entity.Column, "Completeness", "ColumnA", Failure(ValueError("Some")))
    ctx = AnalyzerContext({D.Size(): metric(5.0, "Size", "*"), D.Completeness("ColumnA"): failed})
    with pytest.raises(ValueError, match="Unable to serialize failed metrics"):  # "serialization with mixed Values"
        D.AnalysisResultSerde.serialize([D.AnalysisResult(D.ResultKey(DATE_ONE, {"Region": "EU"}), ctx)])
    for repo in (D.InMemoryMetricsRepository(), D.FileSystemMetricsRepository(tmp_path / "m.json")):
        repo.save(D.ResultKey(1), ctx)
        assert repo.loadByKey(D.ResultKey(1)) == AnalyzerContext({D.Size(): metric(5.0, "Size", "*")})


@pytest.mark.parametrize("analyzer", [D.KLLSketch("x"), D.Histogram("x", lambda v: v),
                                      D.DatasetMatchAnalyzer(None, {"a": "a"}, lambda v: v == 1.0)],
                         ids=["KLLSketch", "Histogram-binningUdf", "DatasetMatchAnalyzer"])
def test_unserializable_analyzer_raises_by_name(analyzer, tmp_path):
    result = D.AnalysisResult(D.ResultKey(0), AnalyzerContext({analyzer: metric(1.0)}))
    with pytest.raises(ValueError) as e:
        D.AnalysisResultSerde.serialize([result])
    assert type(analyzer).__name__ in str(e.value) and "Unable to serialize" in str(e.value)
    with pytest.raises(ValueError, match=type(analyzer).__name__):
        D.FileSystemMetricsRepository(tmp_path / "m.json").save(D.ResultKey(0), result.analyzerContext)
    assert not os.path.exists(tmp_path / "m.json") and os.listdir(tmp_path) == []


def test_result_key_is_a_value():
    a, b = D.ResultKey(5, {"x": "1", "y": "2"}), D.ResultKey(5, {"y": "2", "x": "1"})
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a != D.ResultKey(5, {"x": "1"}) and a != D.ResultKey(6, {"x": "1", "y": "2"}) and D.ResultKey(5) == D.ResultKey(5, {})


# ---- AnalysisResult / loader JSON (reference cases) -------------------------------------------------------------------------
@pytest.mark.parametrize("case", KATS["analysis_result_cases"], ids=[c["source"][20:70] for c in KATS["analysis_result_cases"]])
def test_analysis_result_success_metrics_json(case):
    ctx = AnalyzerContext.empty() if case.get("no_metrics") else fixture_context()
    text = D.AnalysisResult.getSuccessMetricsAsJson(
        D.AnalysisResult(D.ResultKey(DATE_ONE, case["tags"]), ctx),
        [analyzer_from_spec(s) for s in case.get("forAnalyzers", ())], case.get("withTags", ()))
    same_rows(text, case["expected"])


# ---- both stores through one suite ---------------------------------------------------------------------------------------------
@pytest.fixture(params=["memory", "file"])
def repo(request, tmp_path):
    if request.param == "memory":
        return D.InMemoryMetricsRepository()
    return D.FileSystemMetricsRepository(str(tmp_path / "metrics.json"))


@pytest.mark.parametrize("case", KATS["loader_cases"], ids=["two-results", "empty", "different-tags"])
def test_loader_success_metrics_json(repo, case):
    for date, tags in case["saves"]:
        repo.save(D.ResultKey(date, tags), fixture_context())
    loader = repo.load()
    if "after" in case:
        loader = loader.after(case["after"]).before(case["before"])
    same_rows(loader.getSuccessMetricsAsJson(), case["expected"])


def test_loader_json_with_tags(repo):
    repo.save(D.ResultKey(DATE_ONE, {"Region": "EU", "dataset_name": "Some"}), fixture_context())
    rows = json.loads(repo.load().getSuccessMetricsAsJson(withTags=["Region"]))
    assert len(rows) == 4 and all(set(r) == {"entity", "instance", "name", "value", "dataset_date", "region"} for r in rows)


def test_save_then_load_by_key_and_replace(repo):
    key = D.ResultKey(DATE_ONE, {"Region": "EU"})
    assert repo.loadByKey(key) is None and repo.load().get() == []
    repo.save(key, fixture_context())
    assert repo.loadByKey(key) == fixture_context()
    assert repo.loadByKey(D.ResultKey(DATE_ONE, {"Region": "NA"})) is None
    assert repo.loadByKey(D.ResultKey(DATE_TWO, {"Region": "EU"})) is None
    other = AnalyzerContext({D.Size(): metric(7.0, "Size", "*", Entity.Dataset)})
    repo.save(D.ResultKey(DATE_TWO, {"Region": "EU"}), fixture_context())
    repo.save(key, other)  # a save under an existing key replaces that key's result, and only that one
    assert repo.loadByKey(key) == other
    assert repo.loadByKey(D.ResultKey(DATE_TWO, {"Region": "EU"})) == fixture_context()
    assert len(repo.load().get()) == 2


def test_loader_filters(repo):
    keys = [D.ResultKey(10, {"Region": "EU"}), D.ResultKey(20, {"Region": "NA"}),
            D.ResultKey(30, {"Region": "EU", "dataset_name": "Some"}), D.ResultKey(40)]
    for k in keys:
        repo.save(k, fixture_context())

    def dates(loader):
        return sorted(r.resultKey.dataSetDate for r in loader.get())
    assert dates(repo.load()) == [10, 20, 30, 40]
    assert dates(repo.load().after(20)) == [20, 30, 40]  # inclusive
    assert dates(repo.load().before(30)) == [10, 20, 30]  # inclusive
    assert dates(repo.load().after(20).before(30)) == [20, 30]
    assert dates(repo.load().after(21).before(29)) == []
    assert dates(repo.load().withTagValues({"Region": "EU"})) == [10, 30]  # a subset of the key's tags
    assert dates(repo.load().withTagValues({"Region": "EU", "dataset_name": "Some"})) == [30]
    assert dates(repo.load().withTagValues({"Region": "EU", "dataset_name": "Other"})) == []
    assert dates(repo.load().withTagValues({})) == [10, 20, 30, 40]
    wanted = [D.Completeness("att1"), D.Uniqueness(["att1", "att2"]), D.Mean("nowhere")]
    got = repo.load().forAnalyzers(wanted).after(30).get()
    assert len(got) == 2
    for r in got:  # every result stays, with only the asked metrics
        assert set(r.analyzerContext.metricMap) == set(wanted[:2])
        assert r.analyzerContext.metric(D.Completeness("att1")) == fixture_context().metric(D.Completeness("att1"))
    assert all(r.analyzerContext.metricMap == {} for r in repo.load().forAnalyzers([D.Mean("nowhere")]).get())


def test_second_file_repository_sees_the_first_ones_results(tmp_path):
    path = str(tmp_path / "sub.dir" / "metrics.json")
    os.makedirs(os.path.dirname(path))
    first = D.FileSystemMetricsRepository(path)
    first.save(D.ResultKey(1, {"a": "b"}), fixture_context())
    second = D.FileSystemMetricsRepository(path)
    assert second.loadByKey(D.ResultKey(1, {"a": "b"})) == fixture_context()
    second.save(D.ResultKey(2), fixture_context())
    assert sorted(r.resultKey.dataSetDate for r in first.load().get()) == [1, 2]
    assert os.listdir(os.path.dirname(path)) == ["metrics.json"]  # the temporary name was renamed into place
    with open(path) as f:
        assert [r["resultKey"]["dataSetDate"] for r in json.load(f)] == [1, 2]


def test_in_memory_repository_takes_saves_from_many_threads():
    repo, n = D.InMemoryMetricsRepository(), 64
    threads = [threading.Thread(target=lambda i=i: repo.save(D.ResultKey(i % 16, {"t": str(i)}), fixture_context()))
               for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(repo.load().get()) == n


# ---- runner hooks on a host table ---------------------------------------------------------------------------------------------
class HostRows(Analyzer):
    """An analyzer outside the fused scan: counts the host table's rows (times a factor) and its own runs."""
    _fields = ("factor",)
    runs = {}

    def __init__(self, factor=1.0):
        self.factor = factor

    def computeStateFrom(self, data):
        HostRows.runs[self.factor] = HostRows.runs.get(self.factor, 0) + 1
        return data.nrows * self.factor

    def calculate(self, data, aggregateWith=None, saveStatesWith=None):
        return DoubleMetric(Entity.Dataset, "HostRows", "*", Success(self.computeStateFrom(data)))

    def toFailureMetric(self, exception):
        return DoubleMetric(Entity.Dataset, "HostRows", "*", Failure(exception))


@pytest.fixture
def host_table():
    HostRows.runs = {}
    return Table.from_pydict({"k": [1, 2, 3, 4, 5]}, types={"k": "long"})


def test_run_without_a_repository_is_unchanged(host_table):
    ctx = D.AnalysisRunner.onData(host_table).addAnalyzer(HostRows()).run()
    assert ctx.metric(HostRows()).value.get() == 5.0 and HostRows.runs == {1.0: 1}
    with pytest.raises(ValueError, match="useRepository"):
        D.AnalysisRunner.onData(host_table).saveOrAppendResult(D.ResultKey(1))
    with pytest.raises(ValueError, match="useRepository"):
        D.VerificationSuite().onData(host_table).reuseExistingResultsForKey(D.ResultKey(1))
    with pytest.raises(ValueError, match="useRepository"):
        D.VerificationSuite().onData(host_table).addAnomalyCheck(D.AbsoluteChangeStrategy(-1.0, 1.0), D.Size())


def test_reuse_skips_the_analyzers_the_repository_has(host_table):
    key = D.ResultKey(7, {"ds": "t"})
    memory = D.InMemoryMetricsRepository()
    first = D.AnalysisRunner.onData(host_table).useRepository(memory).addAnalyzer(HostRows()) \
        .saveOrAppendResult(key).run()
    assert HostRows.runs == {1.0: 1} and memory.loadByKey(key) == first
    again = D.AnalysisRunner.onData(host_table).useRepository(memory).reuseExistingResultsForKey(key) \
        .addAnalyzers([HostRows(), HostRows(2.0)]).run()
    assert HostRows.runs == {1.0: 1, 2.0: 1}  # only the new analyzer ran
    assert again.metric(HostRows()) == first.metric(HostRows()) and again.metric(HostRows(2.0)).value.get() == 10.0
    assert list(again.metricMap) == [HostRows(), HostRows(2.0)]  # previous ++ new
    assert memory.loadByKey(key) == first  # nothing was saved: no saveOrAppendResult on the second run
    # a stored metric of a real analyzer is reused as it stands: nothing is launched for it
    memory.save(key, AnalyzerContext({D.Size(): metric(123.0, "Size", "*", Entity.Dataset)}))
    reused = D.AnalysisRunner.doAnalysisRun(host_table, [D.Size()], metricsRepository=memory,
                                            reuseExistingResultsForKey=key, failIfResultsForReusingMissing=True)
    assert reused.metric(D.Size()).value.get() == 123.0


def test_fail_if_results_missing(host_table):
    memory, key = D.InMemoryMetricsRepository(), D.ResultKey(7)
    D.AnalysisRunner.onData(host_table).useRepository(memory).addAnalyzer(HostRows()).saveOrAppendResult(key).run()
    ok = D.AnalysisRunner.onData(host_table).useRepository(memory).reuseExistingResultsForKey(key, True) \
        .addAnalyzer(HostRows()).run()
    assert ok.metric(HostRows()).value.get() == 5.0 and HostRows.runs == {1.0: 1}
    with pytest.raises(D.ReusingNotPossibleResultsMissingException) as e:
        D.AnalysisRunner.onData(host_table).useRepository(memory).reuseExistingResultsForKey(key, True) \
            .addAnalyzers([HostRows(), HostRows(3.0), D.Completeness("k")]).run()
    assert str(e.value) == ("Could not find all necessary results in the MetricsRepository, the calculation of the "
                            "metrics for these analyzers would be needed: HostRows(3.0), Completeness(k,None)")
    assert HostRows.runs == {1.0: 1}  # it raised before anything ran
    with pytest.raises(D.ReusingNotPossibleResultsMissingException):  # nothing under the key at all
        D.VerificationSuite().onData(host_table).useRepository(memory) \
            .reuseExistingResultsForKey(D.ResultKey(8), failIfResultsMissing=True).addRequiredAnalyzer(HostRows()).run()


def test_save_appends_and_the_new_metrics_win(host_table):
    memory, key = D.InMemoryMetricsRepository(), D.ResultKey(7)
    stale = DoubleMetric(Entity.Dataset, "HostRows", "*", Success(-1.0))
    memory.save(key, AnalyzerContext({HostRows(): stale, HostRows(9.0): stale}))
    D.AnalysisRunner.onData(host_table).useRepository(memory).addAnalyzers([HostRows(), HostRows(2.0)]) \
        .saveOrAppendResult(key).run()
    saved = memory.loadByKey(key)
    assert saved.metric(HostRows(9.0)) == stale  # appended to what the key held, not overwritten
    assert saved.metric(HostRows()).value.get() == 5.0  # the right-hand side (this run) wins
    assert saved.metric(HostRows(2.0)).value.get() == 10.0
    assert list(saved.metricMap) == [HostRows(), HostRows(9.0), HostRows(2.0)]
    # reuse and save under two keys: the reused metric travels to the new key
    D.AnalysisRunner.onData(host_table).useRepository(memory).reuseExistingResultsForKey(key) \
        .addAnalyzers([HostRows(9.0), HostRows(4.0)]).saveOrAppendResult(D.ResultKey(8)).run()
    assert memory.loadByKey(D.ResultKey(8)).metric(HostRows(9.0)) == stale
    assert memory.loadByKey(D.ResultKey(8)).metric(HostRows(4.0)).value.get() == 20.0


def test_run_async_goes_through_the_hooks(host_table, monkeypatch):
    monkeypatch.setenv("DQ_RUN_SERIAL", "1")  # no device here: the handle is computed on this thread
    memory, key = D.InMemoryMetricsRepository(), D.ResultKey(7)
    handle = D.AnalysisRunner.onData(host_table).useRepository(memory).addAnalyzer(HostRows()) \
        .saveOrAppendResult(key).runAsync()
    assert handle.result() == memory.loadByKey(key)
    assert memory.loadByKey(key).metric(HostRows()).value.get() == 5.0


# ---- the anomaly check of a verification run -----------------------------------------------------------------------------------
def test_anomaly_check_over_a_saved_history(host_table, tmp_path):
    memory = D.InMemoryMetricsRepository()
    rows = HostRows()

    def day(n, size, check=True):
        table = Table.from_pydict({"k": list(range(size))}, types={"k": "long"})
        b = D.VerificationSuite().onData(table).useRepository(memory).saveOrAppendResult(D.ResultKey(n, {"ds": "o"}))
        if check:
            b = b.addAnomalyCheck(D.RelativeRateOfChangeStrategy(maxRateIncrease=1.5), rows)
        else:
            b = b.addRequiredAnalyzer(rows)
        return b.run()
    assert day(1, 100, check=False).status == D.CheckStatus.Success
    assert day(2, 101).status == D.CheckStatus.Success
    result = day(3, 210)
    assert result.status == D.CheckStatus.Warning
    (check,) = result.checkResults
    assert check.level == D.CheckLevel.Warning and check.description == "Anomaly check for HostRows(1.0)"
    (constraint,) = result.checkResults[check].constraintResults
    assert str(constraint.constraint) == "AnomalyConstraint(HostRows(1.0))"
    assert constraint.message == "Value: 210.0 does not meet the constraint requirement!"
    assert len(memory.load().get()) == 3  # the judged run is saved after the check, anomalous or not
    # other tags, or a window without results: the reference's require, as the constraint's message
    config = D.AnomalyCheckConfig(D.CheckLevel.Error, "windowed", {"ds": "other"}, None, None)
    table = Table.from_pydict({"k": [1]}, types={"k": "long"})
    r = D.VerificationSuite().onData(table).useRepository(memory) \
        .addAnomalyCheck(D.AbsoluteChangeStrategy(-1.0, 1.0), rows, config).run()
    assert r.status == D.CheckStatus.Error
    ((c, cr),) = r.checkResults.items()
    assert c.description == "windowed" and cr.constraintResults[0].message == (
        "Can't execute the assertion: requirement failed: There have to be previous results in the MetricsRepository!!")
    # afterDate / beforeDate bound the history: days 1..2 only, against which 102 rows are no anomaly
    config = D.AnomalyCheckConfig(D.CheckLevel.Error, "early", {"ds": "o"}, 1, 2)
    table = Table.from_pydict({"k": list(range(102))}, types={"k": "long"})
    r = D.VerificationSuite().onData(table).useRepository(memory) \
        .addAnomalyCheck(D.RelativeRateOfChangeStrategy(maxRateIncrease=1.5), rows, config).run()
    assert r.status == D.CheckStatus.Success


def test_newest_point_requires(host_table):
    memory = D.InMemoryMetricsRepository()
    value = AnalyzerContext({D.Size(): metric(5.0, "Size", "*", Entity.Dataset)})
    strategy = D.AbsoluteChangeStrategy(-1.0, 1.0)
    with pytest.raises(ValueError, match="There have to be previous results in the MetricsRepository!"):
        D.Check.isNewestPointNonAnomalousAssertion(memory, strategy, D.Size(), {}, None, None, 5.0)
    memory.save(D.ResultKey((1 << 63) - 2), value)
    with pytest.raises(ValueError, match="Test DateTime cannot be Long.MaxValue"):
        D.Check.isNewestPointNonAnomalousAssertion(memory, strategy, D.Size(), {}, None, None, 5.0)
    # two results of one date: ordered by their tag values first, whatever order the store returns
    for order in (("b", "a"), ("a", "b")):
        memory = D.InMemoryMetricsRepository()
        for tag in order:
            memory.save(D.ResultKey(1, {"t": tag}), AnalyzerContext(
                {D.Size(): metric(5.0 if tag == "a" else 50.0, "Size", "*", Entity.Dataset)}))
        # history (1, 5.0), (1, 50.0): the new point follows 50.0
        assert D.Check.isNewestPointNonAnomalousAssertion(memory, strategy, D.Size(), {}, None, None, 50.5)
        assert not D.Check.isNewestPointNonAnomalousAssertion(memory, strategy, D.Size(), {}, None, None, 5.0)


def test_verification_file_outputs(host_table, tmp_path):
    checks_path, metrics_path = str(tmp_path / "checks.json"), str(tmp_path / "metrics.json")
    check = D.Check(D.CheckLevel.Error, "rows").addConstraint(
        D.checks._named(HostRows(), lambda v: v == 4.0, "HostRowsConstraint", hint="five rows"))

    def run(overwrite=None):
        b = D.VerificationSuite().onData(host_table).addCheck(check).saveCheckResultsJsonToPath(checks_path) \
            .saveSuccessMetricsJsonToPath(metrics_path)
        if overwrite is not None:
            b = b.overwritePreviousFiles(overwrite)
        return b.run()
    result = run()
    with open(checks_path) as f:
        assert json.load(f) == [{"check": "rows", "check_level": "Error", "check_status": "Error",
                                 "constraint": "HostRowsConstraint", "constraint_status": "Failure",
                                 "constraint_message": "Value: 5.0 does not meet the constraint requirement! five rows"}]
    with open(metrics_path) as f:
        assert json.load(f) == json.loads(D.VerificationResult.successMetricsAsJson(result)) == [
            {"entity": "Dataset", "instance": "*", "name": "HostRows", "value": 5.0}]
    with pytest.raises(FileExistsError):
        run()
    with pytest.raises(FileExistsError):
        run(False)
    run(True)
