"""Anomaly detection (deequ_amd/anomaly.py) against the cases of the reference's own tests, kept as data in
tests/golden/anomaly_kats.json: the seven strategies, AnomalyDetector, HistoryUtils and the deterministic cases of
HoltWinters. Index lists, anomaly values and confidences are compared exactly; a double is compared with a tolerance
only where the reference's test does, and then with that tolerance. Host logic only, no GPU."""
import json
import os
import re
import sys

import pytest

import deequ_amd as D
from deequ_amd import anomaly as AD
from deequ_amd.metrics import DoubleMetric, Entity, Failure, Success

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anomaly_kats.json")) as f:
    KATS = json.load(f)

NUMBER = re.compile(r"[+-]?(?:\d*\.)?\d+(?:[Ee]\d+)?")  # what the reference's tests read out of a detail text


def series(ref):
    return list(KATS["series"][ref]) if isinstance(ref, str) else list(ref)


def strategy(case):
    return getattr(AD, case["strategy"])(**case["params"])


def detect(s, data, interval):
    return s.detect(data) if interval is None else s.detect(data, tuple(interval))


def ids(cases):
    return ["%02d-%s" % (i, c["source"].split(":")[0]) for i, c in enumerate(cases)]


@pytest.mark.parametrize("case", KATS["strategy_cases"], ids=ids(KATS["strategy_cases"]))
def test_strategy_cases(case):
    data = series(case["series"])
    got = detect(strategy(case), data, case["interval"])
    if case["expected_indices"] is not None:
        assert [i for i, _ in got] == case["expected_indices"]
        assert got == [(i, D.Anomaly(data[i], 1.0)) for i in case["expected_indices"]]
        assert all(a.value == data[i] and a.confidence == 1.0 for i, a in got)
    check = case.get("check_detail")
    if check:  # "produce error message with correct value and bounds"
        assert got
        for _, a in got:
            value, lower, upper = [float(x) for x in NUMBER.findall(a.detail)[:3]]
            if check["value_is_anomaly_value"]:
                assert a.value is not None and value == a.value
            assert value + check["offset"] < lower or value + check["offset"] > upper


@pytest.mark.parametrize("case", KATS["require_cases"], ids=ids(KATS["require_cases"]))
def test_require_cases(case):
    with pytest.raises(ValueError, match="^requirement failed: "):
        s = strategy(case)
        assert "series" in case, "the constructor had to refuse these parameters"
        detect(s, series(case["series"]), case["interval"])


@pytest.mark.parametrize("case", KATS["diff_cases"], ids=ids(KATS["diff_cases"]))
def test_diff_cases(case):
    assert strategy(case).diff(case["data"], case["order"]) == case["expected"]


@pytest.mark.parametrize("case", KATS["online_statistics_cases"], ids=ids(KATS["online_statistics_cases"]))
def test_online_statistics(case):
    data = series(case["series"])
    last = D.OnlineNormalStrategy(**case["params"]).computeStatsAndAnomalies(data)[-1]
    if case.get("against") == "meanAndVariance":
        mean, variance, _ = AD.meanAndVariance(data)
        std = variance ** 0.5
        assert last.mean == mean
        assert abs(last.stdDev - std) < std * case["stdDev_relative_tolerance"]
    else:
        assert last.mean == case["mean"] and last.stdDev == case["stdDev"]


def test_mean_and_variance_is_the_sample_variance():
    assert AD.meanAndVariance([1.0, 2.0, 3.0, 4.0]) == (2.5, 5.0 / 3.0, 4)
    assert AD.meanAndVariance([7.0]) == (7.0, 0.0, 1)


class Recorded(D.AnomalyDetectionStrategy):
    """The reference's stubbed strategy: answers the one call it expects."""

    def __init__(self, sees, returns):
        self.sees, self.returns, self.calls = sees, returns, []

    def detect(self, dataSeries, searchInterval=(0, AD.INT_MAX)):
        self.calls.append((list(dataSeries), tuple(searchInterval)))
        if self.sees is not None and self.calls[-1] == (self.sees["series"], tuple(self.sees["interval"])):
            return [(i, D.Anomaly(v, c)) for i, v, c in self.returns]
        return []


@pytest.mark.parametrize("case", KATS["detector_cases"], ids=ids(KATS["detector_cases"]))
def test_detector_cases(case):
    fake = Recorded(case.get("strategy_sees"), case.get("strategy_returns"))
    detector = D.AnomalyDetector(fake)
    points = [D.DataPoint(t, v) for t, v in case["points"]]
    if case.get("raises"):
        with pytest.raises(ValueError, match="^requirement failed: The first interval element"):
            detector.detectAnomaliesInHistory(points, tuple(case["interval"]))
        return
    got = detector.detectAnomaliesInHistory(points) if case["interval"] is None else \
        detector.detectAnomaliesInHistory(points, tuple(case["interval"]))
    assert fake.calls == [(case["strategy_sees"]["series"], tuple(case["strategy_sees"]["interval"]))]
    assert got == D.DetectionResult([(t, D.Anomaly(v, c)) for t, v, c in case["expected"]])


def test_detector_with_a_real_strategy_over_unordered_points():
    """AnomalyDetectorTest builds this detector beside its stub: the same points through SimpleThresholdStrategy."""
    points = [D.DataPoint(t, v) for t, v in ((10, -1.0), (25, 2.0), (11, 3.0), (0, 0.5))]
    got = D.AnomalyDetector(D.SimpleThresholdStrategy(lowerBound=-0.5, upperBound=1.0)).detectAnomaliesInHistory(points)
    assert got == D.DetectionResult([(10, D.Anomaly(-1.0, 1.0)), (11, D.Anomaly(3.0, 1.0)), (25, D.Anomaly(2.0, 1.0))])


def test_new_point_is_judged_against_the_sorted_history():
    detector = D.AnomalyDetector(D.AbsoluteChangeStrategy(-2.0, 2.0))
    history = [D.DataPoint(3, 1.0), D.DataPoint(1, 1.0), D.DataPoint(2, None)]
    assert detector.isNewPointAnomalous(history, D.DataPoint(4, 1.5)).anomalies == []
    assert detector.isNewPointAnomalous(history, D.DataPoint(4, 9.0)).anomalies == [(4, D.Anomaly(9.0, 1.0))]
    with pytest.raises(ValueError, match="historicalDataPoints must not be empty!"):
        detector.isNewPointAnomalous([], D.DataPoint(4, 1.0))
    with pytest.raises(ValueError) as e:
        detector.isNewPointAnomalous(history, D.DataPoint(3, 1.0))
    assert str(e.value) == ("requirement failed: Can't decide which range to use for anomaly detection. New data "
                            "point with time 3 is in history range (1 - 3)!")


def test_anomaly_equality_ignores_the_detail():
    assert D.Anomaly(1.0, 1.0, "a") == D.Anomaly(1.0, 1.0, "b") and hash(D.Anomaly(1.0, 1.0, "a")) == \
        hash(D.Anomaly(1.0, 1.0))
    assert D.Anomaly(1.0, 1.0) != D.Anomaly(1.0, 0.5) and D.Anomaly(1.0, 1.0) != D.Anomaly(None, 1.0)
    assert D.Anomaly(1.0, 1.0) != (1.0, 1.0)


def test_history_utils():
    case = KATS["history_case"]
    kinds = {"none": None, "failure": DoubleMetric(Entity.Column, "metric-name", "instance-name",
                                                   Failure(ValueError()))}
    metrics = [(t, kinds[m] if isinstance(m, str) else
                DoubleMetric(Entity.Column, "metric-name", "instance-name", Success(m))) for t, m in case["metrics"]]
    for (_, metric), (_, want) in zip(metrics, case["expected_points"]):
        assert AD.extractMetricValue(metric) == want
    assert AD.extractMetricValues(metrics) == [D.DataPoint(t, v) for t, v in case["expected_points"]]


# ---- HoltWinters ------------------------------------------------------------------------------------------------------
def weekly():
    return D.HoltWinters(D.HoltWinters.MetricInterval.Daily, D.HoltWinters.SeriesSeasonality.Weekly)


@pytest.mark.parametrize("case", KATS["holt_winters_cases"], ids=ids(KATS["holt_winters_cases"]))
def test_holt_winters_cases(case):
    pytest.importorskip("scipy")
    data = series(case["series"])
    model = weekly() if not case.get("monthly") else \
        D.HoltWinters(D.HoltWinters.MetricInterval.Monthly, D.HoltWinters.SeriesSeasonality.Yearly)
    if "raises" in case:
        with pytest.raises(ValueError) as e:
            model.detect(data, tuple(case["interval"]))
        assert str(e.value) == case["raises"]
        return
    got = model.detect(data, tuple(case["interval"]))
    if "expected_count" in case:  # the reference asserts how many
        assert len(got) == case["expected_count"]
        assert all(a == D.Anomaly(data[i], 1.0) for i, a in got)
        return
    assert [i for i, _ in got] == case["expected_indices"]
    assert got == [(i, D.Anomaly(data[i], 1.0)) for i in case["expected_indices"]]


def test_holt_winters_periodicity_and_parameters():
    assert weekly().seriesPeriodicity == 7
    assert D.HoltWinters(D.HoltWinters.MetricInterval.Monthly, D.HoltWinters.SeriesSeasonality.Yearly) \
        .seriesPeriodicity == 12
    with pytest.raises(ValueError):
        D.HoltWinters(D.HoltWinters.MetricInterval.Monthly, D.HoltWinters.SeriesSeasonality.Weekly)


def test_holt_winters_names_itself_when_scipy_is_missing(monkeypatch):
    monkeypatch.setitem(sys.modules, "scipy.optimize", None)  # the import inside the strategy now fails
    with pytest.raises(ImportError, match="HoltWinters"):
        weekly().detect([1.0] * 21, (14, 21))


def test_package_imports_without_scipy():
    """scipy is imported by the strategy when it fits, never by the package."""
    import subprocess
    code = ("import sys; sys.modules['scipy'] = None; import deequ_amd; "
            "assert 'scipy.optimize' not in sys.modules; print('ok')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
