"""Metrics repository and anomaly check where they meet the GPU: a verification run over device-resident tables saves,
reloads and judges its metrics day by day; a run that reuses a key's results launches nothing for them (the context's
launch counters); a ChunkedTable of device chunks goes through the same hooks."""
import numpy as np
import pytest

import deequ_amd as D
from deequ_amd import engine
from deequ_amd.table import Table

pytestmark = pytest.mark.gpu

TAGS = {"ds": "orders"}


def device_table(n, seed=11):
    rng = np.random.default_rng(seed)
    data = {"id": [int(v) for v in rng.permutation(n)],
            "s": [None if rng.random() < 0.1 else "v%d" % int(v) for v in rng.integers(0, 50, n)],
            "c": ["abcde"[int(v)] for v in rng.integers(0, 5, n)],
            "x": [None if rng.random() < 0.05 else float(v) for v in rng.normal(size=n)]}
    return Table.from_pydict(data, types={"id": "long", "s": "string", "c": "string", "x": "double"}).to_device()


WATCHED = [D.Size(), D.Completeness("s"), D.Uniqueness(["id"]), D.Histogram("c")]


def counters():
    ctx = engine.ctx()
    return ctx.kernel_launches(), ctx.freq_paths()


def delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def test_history_is_saved_and_the_newest_day_is_judged(tmp_path):
    path = str(tmp_path / "metrics.json")
    repo = D.FileSystemMetricsRepository(path)
    results = {}
    for day, rows in enumerate((1000, 1010, 1020, 2100), start=1):
        t = device_table(rows, seed=day)
        builder = D.VerificationSuite().onData(t).useRepository(repo) \
            .saveOrAppendResult(D.ResultKey(day, TAGS)).addRequiredAnalyzers(WATCHED)
        if day > 1:  # the check requires previous results in the repository: the first day saves only
            builder = builder.addAnomalyCheck(D.RelativeRateOfChangeStrategy(maxRateIncrease=1.5), D.Size())
        results[day] = builder.run()
        assert results[day].metrics[D.Size()].value.get() == float(rows)
    assert [results[d].status for d in (1, 2, 3)] == [D.CheckStatus.Success] * 3
    assert results[4].status == D.CheckStatus.Warning  # the table doubled
    ((check, outcome),) = results[4].checkResults.items()
    assert check.description == "Anomaly check for Size(None)" and check.level == D.CheckLevel.Warning
    assert outcome.constraintResults[0].message == "Value: 2100.0 does not meet the constraint requirement!"
    assert sorted(r.resultKey.dataSetDate for r in repo.load().get()) == [1, 2, 3, 4]
    assert all(r.resultKey.tags == TAGS for r in repo.load().get())
    fresh = D.FileSystemMetricsRepository(path)
    for day, result in results.items():
        for store in (repo, fresh):
            saved = store.loadByKey(D.ResultKey(day, TAGS))
            assert set(saved.metricMap) == set(WATCHED)
            for a in WATCHED:
                assert result.metrics[a].value.isSuccess and saved.metric(a) == result.metrics[a], (day, a)
    # the history of one analyzer, as the check read it
    history = fresh.load().withTagValues(TAGS).forAnalyzers([D.Size()]).get()
    assert sorted((r.resultKey.dataSetDate, r.analyzerContext.metric(D.Size()).value.get()) for r in history) == \
        [(1, 1000.0), (2, 1010.0), (3, 1020.0), (4, 2100.0)]


def test_reused_results_launch_nothing(monkeypatch):
    monkeypatch.setenv("DQ_RUN_SERIAL", "1")  # every pass on this thread's context: its counters see the whole run
    t = device_table(3000)
    analyzers = WATCHED + [D.Mean("x"), D.Entropy("c")]
    repo, key = D.InMemoryMetricsRepository(), D.ResultKey(1, TAGS)
    start = counters()
    first = D.AnalysisRunner.onData(t).useRepository(repo).addAnalyzers(analyzers).saveOrAppendResult(key).run()
    ran = counters()
    assert delta(start[0], ran[0]) and delta(start[1], ran[1])  # the first run did launch scans and build tables
    assert all(m.value.isSuccess for m in first.metricMap.values())
    second = D.AnalysisRunner.onData(t).useRepository(repo).reuseExistingResultsForKey(key) \
        .addAnalyzers(analyzers).run()
    assert counters() == ran  # nothing launched
    assert second == first and list(second.metricMap) == list(first.metricMap)
    # what one new analyzer launches on its own ...
    new = D.Maximum("x")
    before = counters()
    alone = D.AnalysisRunner.onData(t).addAnalyzer(new).run()
    after = counters()
    its_launches = delta(before[0], after[0])
    assert its_launches and after[1] == before[1]
    # ... is all that a reusing run with it launches
    before = counters()
    third = D.AnalysisRunner.onData(t).useRepository(repo).reuseExistingResultsForKey(key) \
        .addAnalyzers(analyzers + [new]).run()
    after = counters()
    assert delta(before[0], after[0]) == its_launches and after[1] == before[1]
    assert third.metric(new) == alone.metric(new)
    assert all(third.metric(a) == first.metric(a) for a in analyzers)
    # and with failIfResultsMissing the run raises instead, before any launch
    with pytest.raises(D.ReusingNotPossibleResultsMissingException, match=r"Maximum\(x,None\)"):
        D.AnalysisRunner.onData(t).useRepository(repo).reuseExistingResultsForKey(key, failIfResultsMissing=True) \
            .addAnalyzers(analyzers + [new]).run()
    assert counters() == after
    # a verification run reuses them the same way
    check = D.Check(D.CheckLevel.Error, "reused").hasSize(lambda n: n == 3000).isUnique("id")
    result = D.VerificationSuite().onData(t).useRepository(repo) \
        .reuseExistingResultsForKey(key, failIfResultsMissing=True).addCheck(check).run()
    assert result.status == D.CheckStatus.Success and counters() == after


def test_chunked_table_goes_through_the_repository(tmp_path):
    chunks = [device_table(1500, seed=21), device_table(1700, seed=22)]
    chunked = D.ChunkedTable(chunks)
    analyzers = [D.Size(), D.Completeness("s"), D.Mean("x"), D.Uniqueness(["c", "s"]), D.Histogram("c")]
    path = str(tmp_path / "chunked.json")
    repo, key = D.FileSystemMetricsRepository(path), D.ResultKey(5, TAGS)
    first = D.AnalysisRunner.onData(chunked).useRepository(repo).addAnalyzers(analyzers).saveOrAppendResult(key).run()
    assert first.metric(D.Size()).value.get() == 3200.0
    assert all(first.metric(a).value.isSuccess for a in analyzers)
    for store in (repo, D.FileSystemMetricsRepository(path)):
        saved = store.loadByKey(key)
        assert set(saved.metricMap) == set(analyzers) and all(saved.metric(a) == first.metric(a) for a in analyzers)
    again = D.AnalysisRunner.onData(chunked).useRepository(repo) \
        .reuseExistingResultsForKey(key, failIfResultsMissing=True).addAnalyzers(analyzers).run()
    assert all(again.metric(a) == first.metric(a) for a in analyzers)
