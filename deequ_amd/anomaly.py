"""Anomaly detection over a metric's history (M/anomalydetection/*.scala): the detector that prepares a time series
(AnomalyDetector.scala:29-102) and the reference's seven strategies. A strategy reads the tens of doubles a
MetricsRepository holds for one analyzer: host arithmetic in the reference's order of operations, no device work.
Scala's `require(cond, msg)` is a ValueError("requirement failed: " + msg); `Option[Double]` is a float or None."""
import enum
import math

from .analyzers import _java_double_to_string

LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
INT_MAX = (1 << 31) - 1
DOUBLE_MAX = 1.7976931348623157e308
DOUBLE_MIN = -DOUBLE_MAX  # Scala's Double.MinValue: the most negative double


def require(condition, message):
    if not condition:
        raise ValueError("requirement failed: %s" % message)


def _d(v):
    """A double inside a Scala s"..." string."""
    return _java_double_to_string(float(v))


class DataPoint:
    """AnomalyDetector.scala:21: a time and the metric's value there (None: missing)."""

    def __init__(self, time, metricValue):
        self.time, self.metricValue = int(time), metricValue

    def __eq__(self, other):
        return isinstance(other, DataPoint) and (self.time, self.metricValue) == (other.time, other.metricValue)

    def __hash__(self):
        return hash((self.time, self.metricValue))

    def __repr__(self):
        return "DataPoint(%d,%r)" % (self.time, self.metricValue)


class Anomaly:
    """DetectionResult.scala:19-54: equal on value and confidence; the detail text takes no part."""

    def __init__(self, value, confidence, detail=None):
        self.value, self.confidence, self.detail = value, confidence, detail

    def __eq__(self, other):
        return isinstance(other, Anomaly) and other.value == self.value and other.confidence == self.confidence

    def __hash__(self):
        return hash((self.value, self.confidence))

    def __repr__(self):
        return "Anomaly(%r,%r,%r)" % (self.value, self.confidence, self.detail)


class DetectionResult:
    """DetectionResult.scala:56: (time, Anomaly) pairs."""

    def __init__(self, anomalies=()):
        self.anomalies = list(anomalies)

    def __eq__(self, other):
        return isinstance(other, DetectionResult) and self.anomalies == other.anomalies

    def __repr__(self):
        return "DetectionResult(%r)" % (self.anomalies,)


def extractMetricValue(metric):
    """HistoryUtils.extractMetricValue: the value of a present, successful metric, else None."""
    if metric is None or not metric.value.isSuccess:
        return None
    return metric.value.get()


def extractMetricValues(metrics):
    """HistoryUtils.extractMetricValues: (date, metric or None) pairs -> DataPoints."""
    return [DataPoint(date, extractMetricValue(metric)) for date, metric in metrics]


def _insertion_point(sorted_values, bound):
    """scala.collection.Searching's binary search over an indexed sequence: the index found, or where to insert."""
    lo, hi = 0, len(sorted_values)
    while hi != lo:
        mid = lo + (hi - lo - 1) // 2
        if bound < sorted_values[mid]:
            hi = mid
        elif bound > sorted_values[mid]:
            lo = mid + 1
        else:
            return mid
    return lo


class AnomalyDetectionStrategy:
    """AnomalyDetectionStrategy.scala:20-32: detect(dataSeries, (start, end)) -> [(index, Anomaly)], end open."""

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        raise NotImplementedError


class AnomalyDetector:
    """AnomalyDetector.scala:29-102."""

    def __init__(self, strategy):
        self.strategy = strategy

    def isNewPointAnomalous(self, historicalDataPoints, newPoint):
        require(len(historicalDataPoints) > 0, "historicalDataPoints must not be empty!")
        points = sorted(historicalDataPoints, key=lambda p: p.time)
        first, last = points[0].time, points[-1].time
        require(last < newPoint.time,
                "Can't decide which range to use for anomaly detection. New data point with time %d is in history "
                "range (%d - %d)!" % (newPoint.time, first, last))
        found = self.detectAnomaliesInHistory(points + [newPoint], (newPoint.time, LONG_MAX))
        return DetectionResult(found.anomalies)

    def detectAnomaliesInHistory(self, dataSeries, searchInterval=(LONG_MIN, LONG_MAX)):
        start, end = searchInterval
        require(start <= end, "The first interval element has to be smaller or equal to the last.")
        points = sorted((p for p in dataSeries if p.metricValue is not None), key=lambda p: p.time)
        times = [p.time for p in points]
        bounds = (_insertion_point(times, start), _insertion_point(times, end))
        found = self.strategy.detect([p.metricValue for p in points], bounds)
        return DetectionResult([(times[i], anomaly) for i, anomaly in found])


class SimpleThresholdStrategy(AnomalyDetectionStrategy):
    """SimpleThresholdStrategy.scala:25-58."""

    def __init__(self, lowerBound=DOUBLE_MIN, upperBound=None):
        if upperBound is None:
            raise TypeError("SimpleThresholdStrategy: upperBound is required")
        self.lowerBound, self.upperBound = float(lowerBound), float(upperBound)
        require(self.lowerBound <= self.upperBound, "The lower bound must be smaller or equal to the upper bound.")

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        start, end = searchInterval
        require(start <= end, "The start of the interval can't be larger than the end.")
        out = []
        for i in range(max(start, 0), min(end, len(dataSeries))):
            v = dataSeries[i]
            if v < self.lowerBound or v > self.upperBound:
                out.append((i, Anomaly(v, 1.0, "[SimpleThresholdStrategy]: Value %s is not in bounds [%s, %s]"
                                       % (_d(v), _d(self.lowerBound), _d(self.upperBound)))))
        return out


class _BaseChangeStrategy(AnomalyDetectionStrategy):
    """BaseChangeStrategy.scala:29-103: anomalies in the order-th discrete difference of the series."""

    def __init__(self, maxRateDecrease=None, maxRateIncrease=None, order=1):
        self.maxRateDecrease, self.maxRateIncrease, self.order = maxRateDecrease, maxRateIncrease, order
        require(maxRateDecrease is not None or maxRateIncrease is not None,
                "At least one of the two limits (maxRateDecrease or maxRateIncrease) has to be specified.")
        require(self._low() <= self._high(),
                "The maximal rate of increase has to be bigger than the maximal rate of decrease.")
        require(order >= 0, "Order of derivative cannot be negative.")

    def _low(self):
        return DOUBLE_MIN if self.maxRateDecrease is None else self.maxRateDecrease

    def _high(self):
        return DOUBLE_MAX if self.maxRateIncrease is None else self.maxRateIncrease

    def diff(self, dataSeries, order):
        require(order >= 0, "Order of diff cannot be negative")
        values = list(dataSeries)
        while order > 0 and values:
            values = [right - left for left, right in zip(values[:-1], values[1:])]
            order -= 1
        return values

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        start, end = searchInterval
        require(start <= end, "The start of the interval cannot be larger than the end.")
        startPoint = max(start - self.order, 0)
        changes = self.diff(dataSeries[startPoint:end], self.order)
        low, high = self._low(), self._high()
        out = []
        for i, change in enumerate(changes):
            if change < low or change > high:
                at = i + startPoint + self.order
                out.append((at, Anomaly(dataSeries[at], 1.0,
                                        "[AbsoluteChangeStrategy]: Change of %s is not in bounds [%s, %s]. Order=%d"
                                        % (_d(change), _d(low), _d(high), self.order))))
        return out

    def __repr__(self):
        return "%s(%r,%r,%d)" % (type(self).__name__, self.maxRateDecrease, self.maxRateIncrease, self.order)


class AbsoluteChangeStrategy(_BaseChangeStrategy):
    """AbsoluteChangeStrategy.scala:33-36."""


class RateOfChangeStrategy(_BaseChangeStrategy):
    """RateOfChangeStrategy.scala:27-31: the deprecated name of AbsoluteChangeStrategy."""


class RelativeRateOfChangeStrategy(_BaseChangeStrategy):
    """RelativeRateOfChangeStrategy.scala:36-64: the ratio of a value to the one `order` steps before it."""

    def diff(self, dataSeries, order):
        require(order > 0, "Order of diff cannot be zero or negative")
        values = list(dataSeries)
        if not values:
            return values
        out = []
        for left, right in zip(values[:len(values) - order], values[order:]):
            try:
                out.append(right / left)
            except ZeroDivisionError:  # IEEE division, as the JVM's
                out.append(math.nan if right == 0 or math.isnan(right) else math.copysign(math.inf, right) *
                           math.copysign(1.0, left))
        return out


def meanAndVariance(values):
    """breeze.stats.meanAndVariance: Welford's running mean and the sample variance. (mean, variance, count)."""
    mu, s, n = 0.0, 0.0, 0
    for y in values:
        n += 1
        d = y - mu
        mu = mu + 1.0 / n * d
        s = s + (n - 1) * d / n * d
    return mu, (s / (n - 1) if n > 1 else 0.0), n


def _check_factors(lower, upper):
    require(lower is not None or upper is not None, "At least one factor has to be specified.")
    require((1.0 if lower is None else lower) >= 0 and (1.0 if upper is None else upper) >= 0,
            "Factors cannot be smaller than zero.")


def _factor(f):
    return DOUBLE_MAX if f is None else f


class BatchNormalStrategy(AnomalyDetectionStrategy):
    """BatchNormalStrategy.scala:33-95."""

    def __init__(self, lowerDeviationFactor=3.0, upperDeviationFactor=3.0, includeInterval=False):
        self.lowerDeviationFactor, self.upperDeviationFactor = lowerDeviationFactor, upperDeviationFactor
        self.includeInterval = includeInterval
        _check_factors(lowerDeviationFactor, upperDeviationFactor)

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        start, end = searchInterval
        require(start <= end, "The start of the interval can't be larger than the end.")
        require(len(dataSeries) > 0, "Data series is empty. Can't calculate mean/ stdDev.")
        require(self.includeInterval or end - start < len(dataSeries),
                "Excluding values in searchInterval from calculation but not enough values remain to calculate mean "
                "and stdDev.")
        basis = dataSeries if self.includeInterval else list(dataSeries[:max(start, 0)]) + list(dataSeries[end:])
        mean, variance, _ = meanAndVariance(basis)
        stdDev = math.sqrt(variance)
        upperBound = mean + _factor(self.upperDeviationFactor) * stdDev
        lowerBound = mean - _factor(self.lowerDeviationFactor) * stdDev
        out = []
        for i in range(max(start, 0), min(end, len(dataSeries))):
            v = dataSeries[i]
            if v > upperBound or v < lowerBound:
                out.append((i, Anomaly(v, 1.0, "[BatchNormalStrategy]: Value %s is not in bounds [%s, %s]."
                                       % (_d(v), _d(lowerBound), _d(upperBound)))))
        return out


class OnlineCalculationResult:
    def __init__(self, mean, stdDev, isAnomaly):
        self.mean, self.stdDev, self.isAnomaly = mean, stdDev, isAnomaly


class OnlineNormalStrategy(AnomalyDetectionStrategy):
    """OnlineNormalStrategy.scala:39-155."""

    def __init__(self, lowerDeviationFactor=3.0, upperDeviationFactor=3.0, ignoreStartPercentage=0.1,
                 ignoreAnomalies=True):
        self.lowerDeviationFactor, self.upperDeviationFactor = lowerDeviationFactor, upperDeviationFactor
        self.ignoreStartPercentage, self.ignoreAnomalies = ignoreStartPercentage, ignoreAnomalies
        _check_factors(lowerDeviationFactor, upperDeviationFactor)
        require(0 <= ignoreStartPercentage <= 1.0, "Percentage of start values to ignore must be in interval [0, 1].")

    def computeStatsAndAnomalies(self, dataSeries, searchInterval=(0, INT_MAX)):
        out = []
        currentMean = currentVariance = Sn = 0.0
        numValuesToSkip = len(dataSeries) * self.ignoreStartPercentage
        searchStart, searchEnd = searchInterval
        for i, value in enumerate(dataSeries):
            lastMean, lastVariance, lastSn = currentMean, currentVariance, Sn
            currentMean = value if i == 0 else lastMean + (1.0 / (i + 1)) * (value - lastMean)
            Sn += (value - lastMean) * (value - currentMean)
            currentVariance = Sn / (i + 1)
            stdDev = math.sqrt(currentVariance)
            upperBound = currentMean + _factor(self.upperDeviationFactor) * stdDev
            lowerBound = currentMean - _factor(self.lowerDeviationFactor) * stdDev
            if i < numValuesToSkip or i < searchStart or i >= searchEnd or lowerBound <= value <= upperBound:
                out.append(OnlineCalculationResult(currentMean, stdDev, False))
            else:
                if self.ignoreAnomalies:  # the anomaly leaves mean and variance as they were
                    currentMean, currentVariance, Sn = lastMean, lastVariance, lastSn
                out.append(OnlineCalculationResult(currentMean, stdDev, True))
        return out

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        start, end = searchInterval
        require(start <= end, "The start of the interval can't be larger than the end.")
        results = self.computeStatsAndAnomalies(dataSeries, searchInterval)
        out = []
        for i in range(max(start, 0), min(end, len(results))):
            r = results[i]
            if r.isAnomaly:
                lowerBound = r.mean - _factor(self.lowerDeviationFactor) * r.stdDev
                upperBound = r.mean + _factor(self.upperDeviationFactor) * r.stdDev
                out.append((i, Anomaly(dataSeries[i], 1.0, "[OnlineNormalStrategy]: Value %s is not in bounds [%s, %s]."
                                       % (_d(dataSeries[i]), _d(lowerBound), _d(upperBound)))))
        return out


def _sum(values):
    """Scala's Seq.sum: a left fold in series order (Python's sum() compensates the rounding of floats)."""
    total = 0.0
    for v in values:
        total += v
    return total


class ModelResults:
    def __init__(self, forecasts, level, trend, seasonality, residuals):
        self.forecasts, self.level, self.trend = forecasts, level, trend
        self.seasonality, self.residuals = seasonality, residuals


class HoltWinters(AnomalyDetectionStrategy):
    """seasonal/HoltWinters.scala:63-249: additive Holt-Winters, ETS(A, A). The three smoothing parameters minimise the
    residual sum of squares over [0, 1]^3 from (0.3, 0.1, 0.1); the reference does it with breeze's L-BFGS-B over a
    forward-difference gradient (step 1e-5), this port with scipy.optimize's L-BFGS-B and the same step. scipy is
    imported when a series is fitted, not with the package."""

    class SeriesSeasonality(enum.Enum):
        Weekly = "Weekly"
        Yearly = "Yearly"

    class MetricInterval(enum.Enum):
        Daily = "Daily"
        Monthly = "Monthly"

    def __init__(self, metricsInterval, seasonality):
        self.metricsInterval, self.seasonality = metricsInterval, seasonality
        periods = {(HoltWinters.SeriesSeasonality.Weekly, HoltWinters.MetricInterval.Daily): 7,
                   (HoltWinters.SeriesSeasonality.Yearly, HoltWinters.MetricInterval.Monthly): 12}
        if (seasonality, metricsInterval) not in periods:
            raise ValueError("HoltWinters: no periodicity for %s metrics with %s seasonality"
                             % (metricsInterval, seasonality))
        self.seriesPeriodicity = periods[(seasonality, metricsInterval)]

    @staticmethod
    def additiveHoltWinters(series, periodicity, numberOfPointsToForecast, alpha, beta, gamma):
        series = list(series)
        firstPeriodSum = _sum(series[:periodicity])
        secondPeriodSum = _sum(series[periodicity:2 * periodicity])
        level = [firstPeriodSum / float(periodicity)]
        trend = [(secondPeriodSum - firstPeriodSum) / (float(periodicity) * float(periodicity))]
        seasonality = [v - level[0] for v in series[:periodicity]]
        y = [level[0] + trend[0] + seasonality[0]]
        Y = list(series)
        for t in range(len(series) + numberOfPointsToForecast):
            if t >= len(series):
                Y.append(level[-1] + trend[-1] + seasonality[len(seasonality) - periodicity])
            level.append(alpha * (Y[t] - seasonality[t]) + (1 - alpha) * (level[t] + trend[t]))
            trend.append(beta * (level[t + 1] - level[t]) + (1 - beta) * trend[t])
            seasonality.append(gamma * (Y[t] - level[t] - trend[t]) + (1 - gamma) * seasonality[t])
            y.append(level[t + 1] + trend[t + 1] + seasonality[t + 1])
        residuals = [value - forecast for forecast, value in zip(y, series)]
        return ModelResults(Y[len(series):], level, trend, seasonality, residuals)

    def _modelSelectionFor(self, dataSeries, numberOfObservationsToForecast):
        try:
            from scipy.optimize import minimize
        except ImportError as e:
            raise ImportError("the HoltWinters anomaly detection strategy fits its smoothing parameters with "
                              "scipy.optimize, and scipy is not installed") from e

        def rss(x):
            fit = HoltWinters.additiveHoltWinters(dataSeries, self.seriesPeriodicity, numberOfObservationsToForecast,
                                                  float(x[0]), float(x[1]), float(x[2]))
            return _sum(r * r for r in fit.residuals)
        best = minimize(rss, [0.3, 0.1, 0.1], method="L-BFGS-B", bounds=[(0.0, 1.0)] * 3, options={"eps": 1e-5})
        return tuple(min(1.0, max(0.0, float(v))) for v in best.x)

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        require(len(dataSeries) > 0, "Provided data series is empty")
        start, end = searchInterval
        require(start < end, "Start must be before end")
        require(start >= 0 and end >= 0, "The search interval needs to be strictly positive")
        require(start >= self.seriesPeriodicity * 2, "Need at least two full cycles of data to estimate model")
        n = 1 if start >= len(dataSeries) else min(end, len(dataSeries)) - start
        training = list(dataSeries[:start])
        alpha, beta, gamma = self._modelSelectionFor(training, n)
        fit = HoltWinters.additiveHoltWinters(training, self.seriesPeriodicity, n, alpha, beta, gamma)
        _, variance, _ = meanAndVariance([abs(r) for r in fit.residuals])
        residualSD = math.sqrt(variance)
        if len(fit.forecasts) != n:
            raise ValueError("requirement failed")
        out = []
        for i, (value, forecast) in enumerate(zip(dataSeries[start:], fit.forecasts)):
            if abs(value - forecast) > 1.96 * residualSD:
                out.append((i + start, Anomaly(value, 1.0, "Forecasted %s for observed value %s"
                                               % (_d(forecast), _d(value)))))
        return out
