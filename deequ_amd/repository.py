"""Metrics repositories (M/repository/*.scala): the metrics of a run stored under a ResultKey, loaded back by key or
by a query over dates, tags and analyzers -- what `reuseExistingResultsForKey`, `saveOrAppendResult` and the anomaly
checks of a verification run read and write. The repository holds metrics, never table data: it lives on the host
side of the C-ABI. AnalysisResultSerde writes the reference's JSON wire format field for field, so a file of the
JVM FileSystemMetricsRepository loads here and a file written here is valid input for the reference's deserializer
(HDFS / S3 paths and the DataFrame outputs are out of scope: paths are local)."""
import json
import os
import re
import threading
import uuid

from . import analyzers as A
from .analyzers import _java_double_to_string
from .metrics import (DoubleMetric, HistogramMetric, KeyedDoubleMetric, Distribution, DistributionValue, Entity,
                      Success, Failure)
from .runners import AnalyzerContext


class ResultKey:
    """MetricsRepository.scala:51: what identifies one AnalysisResult. A value: equal and hashable by date and tags."""

    def __init__(self, dataSetDate, tags=None):
        self.dataSetDate = int(dataSetDate)
        self.tags = dict(tags or {})

    def _key(self):
        return self.dataSetDate, frozenset(self.tags.items())

    def __eq__(self, other):
        return isinstance(other, ResultKey) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "ResultKey(%d,%r)" % (self.dataSetDate, self.tags)


def _format_tag_name(tagName, rows):
    """AnalysisResult.formatTagColumnNameInJson (AnalysisResult.scala:123-136)."""
    name = re.sub(r"[^A-Za-z0-9_]", "", tagName).lower()
    if rows and name in rows[0]:
        name += "_2"
    return name


def _add_column(rows, name, value):
    """AnalysisResult.addColumnToSerializableResult (AnalysisResult.scala:94-109)."""
    if rows and name not in rows[0]:
        return [dict(r, **{name: value}) for r in rows]
    return rows


class AnalysisResult:
    """AnalysisResult.scala:25-137."""

    def __init__(self, resultKey, analyzerContext):
        self.resultKey, self.analyzerContext = resultKey, analyzerContext

    def __eq__(self, other):
        return isinstance(other, AnalysisResult) and self.resultKey == other.resultKey and \
            self.analyzerContext == other.analyzerContext

    def __repr__(self):
        return "AnalysisResult(%r,%r)" % (self.resultKey, self.analyzerContext.metricMap)

    @staticmethod
    def getSuccessMetricsAsJson(analysisResult, forAnalyzers=(), withTags=()):
        """The rows of AnalyzerContext.successMetricsAsJson plus `dataset_date` and one field per tag (of `withTags`
        when given)."""
        rows = json.loads(AnalyzerContext.successMetricsAsJson(analysisResult.analyzerContext, forAnalyzers))
        rows = _add_column(rows, "dataset_date", analysisResult.resultKey.dataSetDate)
        named = {}
        for tagName, tagValue in analysisResult.resultKey.tags.items():
            if not withTags or tagName in withTags:
                named[_format_tag_name(tagName, rows)] = tagValue
        for name, value in named.items():
            rows = _add_column(rows, name, value)
        return json.dumps(rows)


def _json_union(jsonOne, jsonTwo):
    """MetricsRepositoryMultipleResultsLoader.jsonUnion (:100-120): a field one side lacks is null there."""
    one, two = json.loads(jsonOne), json.loads(jsonTwo)
    columns = list(dict.fromkeys(list(one[0] if one else ()) + list(two[0] if two else ())))
    rows = []
    for row in two + one:
        row = dict(row)
        for c in columns:
            row.setdefault(c, None)
        rows.append(row)
    return json.dumps(rows)


class MetricsRepositoryMultipleResultsLoader:
    """MetricsRepositoryMultipleResultsLoader.scala:26-96, with the filters both reference stores apply in get()
    (InMemoryMetricsRepository.scala:119-135): `after` and `before` inclusive, tags by subset, `forAnalyzers` on
    each result's metric map."""

    def __init__(self, results):
        self._results = results  # () -> [AnalysisResult]
        self._tagValues = self._forAnalyzers = self._before = self._after = None

    def withTagValues(self, tagValues):
        self._tagValues = dict(tagValues)
        return self

    def forAnalyzers(self, analyzers):
        self._forAnalyzers = list(analyzers)
        return self

    def before(self, dateTime):
        self._before = dateTime
        return self

    def after(self, dateTime):
        self._after = dateTime
        return self

    def get(self):
        out = []
        for r in self._results():
            key = r.resultKey
            if self._after is not None and not self._after <= key.dataSetDate:
                continue
            if self._before is not None and not key.dataSetDate <= self._before:
                continue
            if self._tagValues is not None and not set(self._tagValues.items()) <= set(key.tags.items()):
                continue
            metrics = {a: m for a, m in r.analyzerContext.metricMap.items()
                       if self._forAnalyzers is None or a in self._forAnalyzers}
            out.append(AnalysisResult(key, AnalyzerContext(metrics)))
        return out

    def getSuccessMetricsAsJson(self, withTags=()):
        results = self.get()
        if not results:
            return AnalysisResult.getSuccessMetricsAsJson(AnalysisResult(ResultKey(0), AnalyzerContext.empty()))
        out = None
        for r in results:
            text = AnalysisResult.getSuccessMetricsAsJson(r, withTags=withTags)
            out = text if out is None else _json_union(out, text)
        return out


def _successful(analyzerContext):
    return AnalyzerContext({a: m for a, m in analyzerContext.metricMap.items() if m.value.isSuccess})


class MetricsRepository:
    """MetricsRepository.scala:25-43."""

    def save(self, resultKey, analyzerContext):
        raise NotImplementedError

    def loadByKey(self, resultKey):
        """The AnalyzerContext saved under exactly this key, or None."""
        raise NotImplementedError

    def load(self):
        raise NotImplementedError


class InMemoryMetricsRepository(MetricsRepository):
    """memory/InMemoryMetricsRepository.scala:28-63. The reference keeps a ConcurrentHashMap; runAsync runs save from
    helper threads here, so every access takes the lock."""

    def __init__(self):
        self._lock = threading.Lock()
        self._results = {}

    def save(self, resultKey, analyzerContext):
        result = AnalysisResult(resultKey, _successful(analyzerContext))
        with self._lock:
            self._results[resultKey] = result

    def loadByKey(self, resultKey):
        with self._lock:
            r = self._results.get(resultKey)
        return None if r is None else r.analyzerContext

    def _all(self):
        with self._lock:
            return list(self._results.values())

    def load(self):
        return MetricsRepositoryMultipleResultsLoader(self._all)


class FileSystemMetricsRepository(MetricsRepository):
    """fs/FileSystemMetricsRepository.scala:32-226 on a local path: every result in one JSON file
    (AnalysisResultSerde). A save reads the file, replaces the key's result and writes the whole file under a
    temporary name beside it, then renames it into place."""

    _lock = threading.Lock()  # one per process: two instances on one path do not interleave their read-modify-write

    def __init__(self, path):
        self.path = os.fspath(path)

    def _all(self):
        try:
            with open(self.path, encoding="utf-8") as f:
                text = f.read()
        except FileNotFoundError:
            return []
        return AnalysisResultSerde.deserialize(text)

    def save(self, resultKey, analyzerContext):
        new = AnalysisResult(resultKey, _successful(analyzerContext))
        with FileSystemMetricsRepository._lock:
            results = [r for r in self._all() if r.resultKey != resultKey] + [new]
            text = AnalysisResultSerde.serialize(results)
            parent = os.path.dirname(os.path.abspath(self.path))
            tmp = os.path.join(parent, "%s.json" % uuid.uuid4())
            try:
                with open(tmp, "x", encoding="utf-8") as f:
                    f.write(text)
                os.replace(tmp, self.path)
            except BaseException:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise

    def loadByKey(self, resultKey):
        for r in self._all():
            if r.resultKey == resultKey:
                return r.analyzerContext
        return None

    def load(self):
        return MetricsRepositoryMultipleResultsLoader(self._all)


# ---- AnalysisResultSerde (AnalysisResultSerde.scala:38-635) -------------------------------------------------------
def _where(obj, analyzer):
    if analyzer.where is not None:
        obj["where"] = analyzer.where
    return obj


def _column_where(name):
    def write(a):
        return _where({"analyzerName": name, "column": a.column}, a)
    return write


def _columns_where(name):
    def write(a):
        return _where({"analyzerName": name, "columns": list(a.columns)}, a)
    return write


def _quantile_text(q):
    return _java_double_to_string(float(q))


_WRITERS = {
    A.Size: lambda a: _where({"analyzerName": "Size"}, a),
    A.Completeness: _column_where("Completeness"),
    A.Compliance: lambda a: _where({"analyzerName": "Compliance"}, a) | {"instance": a.instance,
                                                                        "predicate": a.predicate},
    A.PatternMatch: lambda a: _where({"analyzerName": "PatternMatch", "column": a.column}, a) | {"pattern": a.pattern},
    A.Sum: _column_where("Sum"),
    A.Mean: _column_where("Mean"),
    A.Minimum: _column_where("Minimum"),
    A.Maximum: _column_where("Maximum"),
    A.CountDistinct: _columns_where("CountDistinct"),
    A.Distinctness: _columns_where("Distinctness"),
    A.Entropy: _column_where("Entropy"),
    A.MutualInformation: _columns_where("MutualInformation"),
    A.UniqueValueRatio: _columns_where("UniqueValueRatio"),
    A.Uniqueness: _columns_where("Uniqueness"),
    A.Histogram: lambda a: {"analyzerName": "Histogram", "column": a.column, "maxDetailBins": a.maxDetailBins},
    A.DataType: _column_where("DataType"),
    A.ApproxCountDistinct: _column_where("ApproxCountDistinct"),
    A.Correlation: lambda a: _where({"analyzerName": "Correlation", "firstColumn": a.firstColumn,
                                     "secondColumn": a.secondColumn}, a),
    A.StandardDeviation: _column_where("StandardDeviation"),
    A.ApproxQuantile: lambda a: _where({"analyzerName": "ApproxQuantile", "column": a.column, "quantile": a.quantile,
                                        "relativeError": a.relativeError}, a),
    A.ApproxQuantiles: lambda a: {"analyzerName": "ApproxQuantiles", "column": a.column,
                                  "quantiles": ",".join(_quantile_text(q) for q in a.quantiles),
                                  "relativeError": a.relativeError},
    A.MinLength: _column_where("MinLength"),
    A.MaxLength: _column_where("MaxLength"),
}


def _opt_where(o):
    return o.get("where")


_READERS = {
    "Size": lambda o: A.Size(_opt_where(o)),
    "Compliance": lambda o: A.Compliance(o["instance"], o["predicate"], _opt_where(o)),
    "PatternMatch": lambda o: A.PatternMatch(o["column"], o["pattern"], _opt_where(o)),
    "Histogram": lambda o: A.Histogram(o["column"], None, int(o["maxDetailBins"])),
    "Correlation": lambda o: A.Correlation(o["firstColumn"], o["secondColumn"], _opt_where(o)),
    "ApproxQuantile": lambda o: A.ApproxQuantile(o["column"], float(o["quantile"]), float(o["relativeError"]),
                                                 where=_opt_where(o)),
    "ApproxQuantiles": lambda o: A.ApproxQuantiles(o["column"], [float(q) for q in o["quantiles"].split(",")],
                                                   float(o["relativeError"])),
}
for _name in ("Completeness", "Sum", "Mean", "Minimum", "Maximum", "DataType", "ApproxCountDistinct",
              "StandardDeviation", "MinLength", "MaxLength", "Entropy"):
    _READERS[_name] = (lambda cls: lambda o: cls(o["column"], _opt_where(o)))(getattr(A, _name))
for _name in ("CountDistinct", "Distinctness", "MutualInformation", "UniqueValueRatio", "Uniqueness"):
    _READERS[_name] = (lambda cls: lambda o: cls(list(o["columns"]), _opt_where(o)))(getattr(A, _name))
del _name


class AnalysisResultSerde:
    """AnalysisResultSerde.scala:75-106: [AnalysisResult] <-> the reference's JSON. An absent `where` is left out, as
    gson leaves out the reference's null property; the `where` of the grouping analyzers and of ApproxQuantile (this
    project's extension) goes under the same field, so a file without one reads back to the plain analyzer."""

    @staticmethod
    def serialize(analysisResults):
        return json.dumps([AnalysisResultSerde._result(r) for r in analysisResults], indent=2)

    @staticmethod
    def deserialize(text):
        out = []
        for r in json.loads(text):
            key = ResultKey(int(r["resultKey"]["dataSetDate"]), r["resultKey"].get("tags") or {})
            metrics = {}
            for entry in r["analyzerContext"]["metricMap"]:
                metrics[AnalysisResultSerde.analyzer_from_json(entry["analyzer"])] = \
                    AnalysisResultSerde.metric_from_json(entry["metric"])
            out.append(AnalysisResult(key, AnalyzerContext(metrics)))
        return out

    @staticmethod
    def _result(r):
        entries = [{"analyzer": AnalysisResultSerde.analyzer_to_json(a), "metric": AnalysisResultSerde.metric_to_json(m)}
                   for a, m in r.analyzerContext.metricMap.items()]
        return {"resultKey": {"dataSetDate": r.resultKey.dataSetDate, "tags": dict(r.resultKey.tags)},
                "analyzerContext": {"metricMap": entries}}

    @staticmethod
    def analyzer_to_json(analyzer):
        if isinstance(analyzer, A.Histogram) and analyzer.binningUdf is not None:
            raise ValueError("Unable to serialize Histogram with binningUdf! (%r)" % (analyzer,))
        write = _WRITERS.get(type(analyzer))
        if write is None:
            raise ValueError("Unable to serialize analyzer %r." % (analyzer,))
        return write(analyzer)

    @staticmethod
    def analyzer_from_json(obj):
        read = _READERS.get(obj["analyzerName"])
        if read is None:
            raise ValueError("Unable to deserialize analyzer %s." % obj["analyzerName"])
        return read(obj)

    @staticmethod
    def metric_to_json(metric):
        if metric.value.isFailure:
            raise ValueError("Unable to serialize failed metrics.")
        if isinstance(metric, DoubleMetric):
            return {"metricName": "DoubleMetric", "entity": str(metric.entity), "instance": metric.instance,
                    "name": metric.name, "value": float(metric.value.get())}
        if isinstance(metric, HistogramMetric):
            dist = metric.value.get()
            values = {k: {"absolute": int(v.absolute), "ratio": float(v.ratio)} for k, v in dist.values.items()}
            return {"metricName": "HistogramMetric", "column": metric.column, "numberOfBins": int(dist.numberOfBins),
                    "value": {"numberOfBins": int(dist.numberOfBins), "values": values}}
        if isinstance(metric, KeyedDoubleMetric):
            return {"metricName": "KeyedDoubleMetric", "entity": str(metric.entity), "instance": metric.instance,
                    "name": metric.name, "value": {k: float(v) for k, v in metric.value.get().items()}}
        raise ValueError("Unable to serialize metrics %r." % (metric,))

    @staticmethod
    def metric_from_json(obj):
        kind = obj["metricName"]
        if kind == "DoubleMetric":
            return DoubleMetric(Entity(obj["entity"]), obj["name"], obj["instance"], Success(float(obj["value"])))
        if kind == "HistogramMetric":
            dist = obj["value"]
            values = {k: DistributionValue(int(v["absolute"]), float(v["ratio"])) for k, v in dist["values"].items()}
            return HistogramMetric(obj["column"], Success(Distribution(values, int(dist["numberOfBins"]))))
        if kind == "KeyedDoubleMetric":
            entity, name, instance = Entity(obj["entity"]), obj["name"], obj["instance"]
            if "value" in obj:
                return KeyedDoubleMetric(entity, name, instance,
                                         Success({k: float(v) for k, v in obj["value"].items()}))
            return KeyedDoubleMetric(entity, name, instance, Failure(ValueError("no value was stored")))
        raise ValueError("Unable to deserialize analyzer %s." % kind)
