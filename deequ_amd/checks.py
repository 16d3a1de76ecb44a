"""VerificationSuite / Check / Constraint — deequ's declarative layer over the analyzers
(M/VerificationSuite.scala:44-315, M/checks/Check.scala:60-1056, M/constraints/Constraint.scala,
M/constraints/AnalysisBasedConstraint.scala), as a thin host layer: a run collects every check's
required analyzers and hands them to ONE AnalysisRunner.doAnalysisRun (so all scan-shareable
metrics of all checks come from one fused dq_scan), then evaluates the assertions on the metrics.
VerificationResult.rowLevelResultsAsTable adds one pass / fail column per check to the data (rowlevel.py: the
per-row outcomes are computed and kept on the GPU).
A run may name a MetricsRepository (repository.py): metrics it holds are reused, the run's are saved after the checks
are evaluated, and an anomaly check (anomaly.py) judges a new metric against the history saved there.
KLL constraints are out of scope.
"""
import enum
import json

from . import analyzers as A
from .analyzers import _java_double_to_string
from .runners import AnalysisRunner, AnalyzerContext, RepositoryOptions


class CheckLevel(enum.Enum):
    Error = "Error"
    Warning = "Warning"


class CheckStatus(enum.IntEnum):
    Success = 0
    Warning = 1
    Error = 2


class ConstraintStatus(enum.Enum):
    Success = "Success"
    Failure = "Failure"


def is_one(v):
    """Check.IsOne (M/checks/Check.scala: `_ == 1.0`)."""
    return v == 1.0


def _fmt(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, float):
        return _java_double_to_string(v)
    return str(v)


class ConstraintResult:
    def __init__(self, constraint, status, message=None, metric=None):
        self.constraint, self.status, self.message, self.metric = constraint, status, message, metric

    def __repr__(self):
        return "ConstraintResult(%s,%s,%r)" % (self.constraint, self.status.value, self.message)


class AnalysisBasedConstraint:
    """M/constraints/AnalysisBasedConstraint.scala:33-110."""
    MissingAnalysis = "Missing Analysis, can't run the constraint!"
    ProblematicMetricPicker = "Can't retrieve the value to assert on"
    AssertionException = "Can't execute the assertion"

    def __init__(self, analyzer, assertion, value_picker=None, hint=None):
        self.analyzer, self.assertion, self.value_picker, self.hint = analyzer, assertion, value_picker, hint

    def evaluate(self, metric_map):
        metric = metric_map.get(self.analyzer)
        if metric is None:
            return ConstraintResult(self, ConstraintStatus.Failure, self.MissingAnalysis, None)
        if metric.value.isFailure:
            return ConstraintResult(self, ConstraintStatus.Failure, str(metric.value.failed), metric)
        try:
            value = self.value_picker(metric.value.get()) if self.value_picker else metric.value.get()
        except Exception as e:
            return ConstraintResult(self, ConstraintStatus.Failure, "%s: %s!" % (self.ProblematicMetricPicker, e),
                                    metric)
        try:
            ok = self.assertion(value)
        except Exception as e:
            return ConstraintResult(self, ConstraintStatus.Failure, "%s: %s!" % (self.AssertionException, e), metric)
        if ok:
            return ConstraintResult(self, ConstraintStatus.Success, None, metric)
        msg = "Value: %s does not meet the constraint requirement!" % _fmt(value)
        if self.hint:
            msg += " " + self.hint
        return ConstraintResult(self, ConstraintStatus.Failure, msg, metric)


class NamedConstraint:
    """M/constraints/Constraint.scala:50-62: the result's constraint is the named decorator."""

    def __init__(self, inner, name):
        self.inner, self.name = inner, name

    def evaluate(self, metric_map):
        r = self.inner.evaluate(metric_map)
        r.constraint = self
        return r

    def __repr__(self):
        return self.name


def _named(analyzer, assertion, name, picker=None, hint=None):
    return NamedConstraint(AnalysisBasedConstraint(analyzer, assertion, picker, hint), name)


def _ratio_types(ignore_unknown, key):
    """Constraint.ratioTypes (M/constraints/Constraint.scala:656-680)."""
    def pick(dist):
        if not ignore_unknown:
            v = dist.values.get(key)
            return 0.0 if v is None else v.ratio
        v = dist.values.get(key)
        count = 0 if v is None else v.absolute
        if count == 0:
            return 0.0
        total = sum(x.absolute for x in dist.values.values())
        unknown = dist.values.get("Unknown")
        return count / (total - (0 if unknown is None else unknown.absolute))
    return pick


class ConstrainableDataTypes(enum.Enum):
    Null = "Null"
    Fractional = "Fractional"
    Integral = "Integral"
    Boolean = "Boolean"
    String = "String"
    Numeric = "Numeric"


class CheckResult:
    def __init__(self, check, status, constraintResults):
        self.check, self.status, self.constraintResults = check, status, constraintResults


class Check:
    """M/checks/Check.scala:60-1056 (KLL constraints excluded)."""

    def __init__(self, level, description, constraints=None):
        self.level, self.description = level, description
        self.constraints = list(constraints or [])

    def __repr__(self):
        return "Check(%s,%s,%r)" % (self.level.value, self.description, self.constraints)

    def addConstraint(self, constraint):
        return Check(self.level, self.description, self.constraints + [constraint])

    def _filterable(self, create):
        return CheckWithLastConstraintFilterable(self.level, self.description,
                                                 self.constraints + [create(None)], create)

    # ---- size / completeness / uniqueness ---------------------------------------------------
    def hasSize(self, assertion, hint=None):
        def mk(where):
            size = A.Size(where)
            return _named(size, assertion, "SizeConstraint(%r)" % size, lambda v: int(v), hint)
        return self._filterable(mk)

    def isComplete(self, column, hint=None):
        return self.hasCompleteness(column, is_one, hint)

    def hasCompleteness(self, column, assertion, hint=None):
        def mk(where):
            c = A.Completeness(column, where)
            return _named(c, assertion, "CompletenessConstraint(%r)" % c, hint=hint)
        return self._filterable(mk)

    def isUnique(self, column, hint=None):
        return self.hasUniqueness([column], is_one, hint)

    def isPrimaryKey(self, column, *columns):
        return self.hasUniqueness([column] + list(columns), is_one)

    def hasUniqueness(self, columns, assertion, hint=None):
        def mk(where):
            u = A.Uniqueness([columns] if isinstance(columns, str) else list(columns), where)
            return _named(u, assertion, "UniquenessConstraint(%r)" % u, hint=hint)
        return self._filterable(mk)

    def doesDatasetMatch(self, otherDataset, keyColumnMappings, assertion, matchColumnMappings=None, hint=None):
        """Check.doesDatasetMatch of the later deequ releases: the share of rows that match
        `otherDataset` on the key mappings (and the match mappings) meets `assertion`."""
        from .comparison import DatasetMatchAnalyzer
        a = DatasetMatchAnalyzer(otherDataset, keyColumnMappings, assertion, matchColumnMappings)
        return self.addConstraint(_named(a, assertion, "DatasetMatchConstraint(%r)" % a, hint=hint))

    def hasDistinctness(self, columns, assertion, hint=None):
        def mk(where):
            d = A.Distinctness(list(columns), where)
            return _named(d, assertion, "DistinctnessConstraint(%r)" % d, hint=hint)
        return self._filterable(mk)

    def hasUniqueValueRatio(self, columns, assertion, hint=None):
        def mk(where):
            u = A.UniqueValueRatio(list(columns), where)
            return _named(u, assertion, "UniqueValueRatioConstraint(%r" % u, hint=hint)
        return self._filterable(mk)

    def hasNumberOfDistinctValues(self, column, assertion, binningUdf=None,
                                  maxBins=A.Histogram.MaximumAllowedDetailBins, hint=None):
        h = A.Histogram(column, binningUdf, maxBins)
        return self.addConstraint(_named(h, assertion, "HistogramBinConstraint(%r)" % h,
                                         lambda d: d.numberOfBins, hint))

    def hasHistogramValues(self, column, assertion, binningUdf=None,
                           maxBins=A.Histogram.MaximumAllowedDetailBins, hint=None):
        h = A.Histogram(column, binningUdf, maxBins)
        return self.addConstraint(_named(h, assertion, "HistogramConstraint(%r)" % h, hint=hint))

    # ---- anomaly detection ------------------------------------------------------------------
    def isNewestPointNonAnomalous(self, metricsRepository, anomalyDetectionStrategy, analyzer, withTagValues=None,
                                  afterDate=None, beforeDate=None, hint=None):
        """M/checks/Check.scala:345-365: the analyzer's new value is no anomaly against its history in the repository
        (the results under `withTagValues`, from `afterDate` to `beforeDate`, both inclusive)."""
        def assertion(currentMetricValue):
            return Check.isNewestPointNonAnomalousAssertion(metricsRepository, anomalyDetectionStrategy, analyzer,
                                                            withTagValues or {}, afterDate, beforeDate,
                                                            currentMetricValue)
        return self.addConstraint(_named(analyzer, assertion, "AnomalyConstraint(%r)" % analyzer, hint=hint))

    @staticmethod
    def isNewestPointNonAnomalousAssertion(metricsRepository, anomalyDetectionStrategy, analyzer, withTagValues,
                                           afterDate, beforeDate, currentMetricValue):
        """Check.isNewestPointNonAnomalous of the companion object (M/checks/Check.scala:998-1055)."""
        from .anomaly import AnomalyDetector, DataPoint, LONG_MAX, extractMetricValues, require
        loader = metricsRepository.load().withTagValues(withTagValues)
        if beforeDate is not None:
            loader = loader.before(beforeDate)
        if afterDate is not None:
            loader = loader.after(afterDate)
        analysisResults = loader.forAnalyzers([analyzer]).get()
        require(len(analysisResults) > 0, "There have to be previous results in the MetricsRepository!")
        # two results of one date are unusual: sorted by their tag values first (a stable sort), they come out of the
        # detector's sort by time in one order whatever the store returned
        ordered = sorted(analysisResults, key=lambda r: list(r.resultKey.tags.values()))
        historicalMetrics = [(r.resultKey.dataSetDate, next(iter(r.analyzerContext.metricMap.values()), None))
                             for r in ordered]
        testDateTime = max(r.resultKey.dataSetDate for r in analysisResults) + 1
        require(testDateTime != LONG_MAX, "Test DateTime cannot be Long.MaxValue, otherwise theAnomaly Detection, "
                "which works with an open upper interval bound, won't test anything")
        detected = AnomalyDetector(anomalyDetectionStrategy).isNewPointAnomalous(
            extractMetricValues(historicalMetrics), DataPoint(testDateTime, currentMetricValue))
        return not detected.anomalies

    # ---- information ------------------------------------------------------------------------
    def hasEntropy(self, column, assertion, hint=None):
        def mk(where):
            e = A.Entropy(column, where)
            return _named(e, assertion, "EntropyConstraint(%r)" % e, hint=hint)
        return self._filterable(mk)

    def hasMutualInformation(self, columnA, columnB, assertion, hint=None):
        def mk(where):
            m = A.MutualInformation([columnA, columnB], where)
            return _named(m, assertion, "MutualInformationConstraint(%r)" % m, hint=hint)
        return self._filterable(mk)

    def hasApproxQuantile(self, column, quantile, assertion, hint=None):
        def mk(where):
            q = A.ApproxQuantile(column, quantile, where=where)
            return _named(q, assertion, "ApproxQuantileConstraint(%r)" % q, hint=hint)
        return self._filterable(mk)

    # ---- per-column statistics (filterable) -------------------------------------------------
    def _stat(self, cls, label, column, assertion, hint):
        def mk(where):
            a = cls(column, where)
            return _named(a, assertion, "%s(%r)" % (label, a), hint=hint)
        return self._filterable(mk)

    def hasMinLength(self, column, assertion, hint=None):
        return self._stat(A.MinLength, "MinLengthConstraint", column, assertion, hint)

    def hasMaxLength(self, column, assertion, hint=None):
        return self._stat(A.MaxLength, "MaxLengthConstraint", column, assertion, hint)

    def hasMin(self, column, assertion, hint=None):
        return self._stat(A.Minimum, "MinimumConstraint", column, assertion, hint)

    def hasMax(self, column, assertion, hint=None):
        return self._stat(A.Maximum, "MaximumConstraint", column, assertion, hint)

    def hasMean(self, column, assertion, hint=None):
        return self._stat(A.Mean, "MeanConstraint", column, assertion, hint)

    def hasSum(self, column, assertion, hint=None):
        return self._stat(A.Sum, "SumConstraint", column, assertion, hint)

    def hasStandardDeviation(self, column, assertion, hint=None):
        return self._stat(A.StandardDeviation, "StandardDeviationConstraint", column, assertion, hint)

    def hasApproxCountDistinct(self, column, assertion, hint=None):
        return self._stat(A.ApproxCountDistinct, "ApproxCountDistinctConstraint", column, assertion, hint)

    def hasCorrelation(self, columnA, columnB, assertion, hint=None):
        def mk(where):
            c = A.Correlation(columnA, columnB, where)
            return _named(c, assertion, "CorrelationConstraint(%r)" % c, hint=hint)
        return self._filterable(mk)

    # ---- predicates -------------------------------------------------------------------------
    def satisfies(self, columnCondition, constraintName, assertion=is_one, hint=None):
        def mk(where):
            c = A.Compliance(constraintName, columnCondition, where)
            return _named(c, assertion, "ComplianceConstraint(%r)" % c, hint=hint)
        return self._filterable(mk)

    def hasPattern(self, column, pattern, assertion=is_one, name=None, hint=None):
        pat = pattern.pattern if hasattr(pattern, "pattern") else str(pattern)

        def mk(where):
            p = A.PatternMatch(column, pat, where)
            return _named(p, assertion, name or "PatternMatchConstraint(%s, %s)" % (column, pat), hint=hint)
        return self._filterable(mk)

    def containsCreditCardNumber(self, column, assertion=is_one, hint=None):
        return self.hasPattern(column, A.Patterns.CREDITCARD, assertion, "containsCreditCardNumber(%s)" % column,
                               hint)

    def containsEmail(self, column, assertion=is_one, hint=None):
        return self.hasPattern(column, A.Patterns.EMAIL, assertion, "containsEmail(%s)" % column, hint)

    def containsURL(self, column, assertion=is_one, hint=None):
        return self.hasPattern(column, A.Patterns.URL, assertion, "containsURL(%s)" % column, hint)

    def containsSocialSecurityNumber(self, column, assertion=is_one, hint=None):
        return self.hasPattern(column, A.Patterns.SOCIAL_SECURITY_NUMBER_US, assertion,
                               "containsSocialSecurityNumber(%s)" % column, hint)

    def hasDataType(self, column, dataType, assertion=is_one, hint=None):
        """Constraint.dataTypeConstraint (M/constraints/Constraint.scala:592-614)."""
        if dataType == ConstrainableDataTypes.Null:
            picker = _ratio_types(False, "Unknown")
        elif dataType == ConstrainableDataTypes.Numeric:
            f, i = _ratio_types(True, "Fractional"), _ratio_types(True, "Integral")

            def picker(d):
                return f(d) + i(d)
        else:
            picker = _ratio_types(True, dataType.value)
        d = A.DataType(column)
        return self.addConstraint(AnalysisBasedConstraint(d, assertion, picker, hint))

    def isNonNegative(self, column, assertion=is_one, hint=None):
        return self.satisfies("COALESCE(%s, 0.0) >= 0" % column, "%s is non-negative" % column, assertion, hint)

    def isPositive(self, column, assertion=is_one, hint=None):
        return self.satisfies("COALESCE(%s, 1.0) > 0" % column, "%s is positive" % column, assertion, hint)

    def isLessThan(self, columnA, columnB, assertion=is_one, hint=None):
        return self.satisfies("%s < %s" % (columnA, columnB), "%s is less than %s" % (columnA, columnB), assertion,
                              hint)

    def isLessThanOrEqualTo(self, columnA, columnB, assertion=is_one, hint=None):
        return self.satisfies("%s <= %s" % (columnA, columnB), "%s is less than or equal to %s" % (columnA, columnB),
                              assertion, hint)

    def isGreaterThan(self, columnA, columnB, assertion=is_one, hint=None):
        return self.satisfies("%s > %s" % (columnA, columnB), "%s is greater than %s" % (columnA, columnB),
                              assertion, hint)

    def isGreaterThanOrEqualTo(self, columnA, columnB, assertion=is_one, hint=None):
        return self.satisfies("%s >= %s" % (columnA, columnB),
                              "%s is greater than or equal to %s" % (columnA, columnB), assertion, hint)

    def isContainedIn(self, column, allowedValues=None, assertion=is_one, hint=None, lowerBound=None,
                      upperBound=None, includeLowerBound=True, includeUpperBound=True):
        """Both isContainedIn variants (M/checks/Check.scala:844-948): a value list, or a numeric interval."""
        if lowerBound is not None or upperBound is not None:
            lo, hi = float(lowerBound), float(upperBound)
            pred = "`%s` IS NULL OR (`%s` %s %s AND `%s` %s %s)" % (
                column, column, ">=" if includeLowerBound else ">", _java_double_to_string(lo), column,
                "<=" if includeUpperBound else "<", _java_double_to_string(hi))
            return self.satisfies(pred, "%s between %s and %s" % (column, _java_double_to_string(lo),
                                                                  _java_double_to_string(hi)), hint=hint)
        values = ",".join("'%s'" % v.replace("'", "''") for v in allowedValues)
        pred = "`%s` IS NULL OR `%s` IN (%s)" % (column, column, values)
        return self.satisfies(pred, "%s contained in %s" % (column, ",".join(allowedValues)), assertion, hint)

    # ---- evaluation -------------------------------------------------------------------------
    def evaluate(self, context):
        """Check.evaluate (M/checks/Check.scala:950-962)."""
        results = [c.evaluate(context.metricMap) for c in self.constraints]
        failed = any(r.status == ConstraintStatus.Failure for r in results)
        if failed:
            status = CheckStatus.Error if self.level == CheckLevel.Error else CheckStatus.Warning
        else:
            status = CheckStatus.Success
        return CheckResult(self, status, results)

    def requiredAnalyzers(self):
        out = []
        for c in self.constraints:
            inner = c.inner if isinstance(c, NamedConstraint) else c
            if isinstance(inner, AnalysisBasedConstraint) and inner.analyzer not in out:
                out.append(inner.analyzer)
        return out


class CheckWithLastConstraintFilterable(Check):
    """M/checks/CheckWithLastConstraintFilterable.scala: `.where(filter)` rebuilds the last constraint."""

    def __init__(self, level, description, constraints, create):
        super().__init__(level, description, constraints)
        self._create = create

    def where(self, filter_):
        return Check(self.level, self.description, self.constraints[:-1] + [self._create(filter_)])


class VerificationResult:
    """M/VerificationResult.scala: overall status, per-check results and all metrics."""

    def __init__(self, status, checkResults, metrics):
        self.status, self.checkResults, self.metrics = status, checkResults, metrics

    @staticmethod
    def successMetricsAsJson(result, forAnalyzers=()):
        return AnalyzerContext.successMetricsAsJson(AnalyzerContext(result.metrics), forAnalyzers)

    @staticmethod
    def checkResultsAsJson(result, forChecks=()):
        """M/VerificationResult.scala:73-115: one row per constraint result (`forChecks` is unused there too)."""
        rows = []
        for r in result.checkResults.values():
            for c in r.constraintResults:
                rows.append({"check": r.check.description, "check_level": r.check.level.value,
                             "check_status": r.status.name, "constraint": str(c.constraint),
                             "constraint_status": c.status.value, "constraint_message": c.message or ""})
        return json.dumps(rows)

    @staticmethod
    def rowLevelResultsAsTable(result, data, filteredRow="true", strict=False):
        """rowLevelResultsAsDataFrame of later deequ releases: `data` plus one BOOLEAN column per check of `result`
        that has a row-level constraint, named by the check's description; row i is the AND of those constraints'
        outcomes on row i. Returns a rowlevel.RowLevelResults (the table, per-check and per-constraint counts, and
        failedRowsTable / passedRowsTable). `filteredRow`: the outcome of a row a constraint's `where` leaves out,
        "true" (deequ's FilteredRowOutcome.TRUE) or "null". A constraint that cannot be evaluated per row is listed in
        `.skipped`, or raises with `strict`."""
        from .rowlevel import row_level_results
        return row_level_results(result, data, filteredRow, strict)


class VerificationRunBuilder:
    """M/VerificationRunBuilder.scala: onData(..).addCheck(..).addRequiredAnalyzer(..).run()."""

    def __init__(self, data):
        self.data = data
        self.checks = []
        self.requiredAnalyzers = []
        self._aggregateWith = None
        self._saveStatesWith = None
        self._repository = RepositoryOptions()
        self._check_results_path = None
        self._success_metrics_path = None
        self._overwrite = False

    def useRepository(self, metricsRepository):
        """The MetricsRepository (repository.py) of reuseExistingResultsForKey, saveOrAppendResult and
        addAnomalyCheck."""
        self._repository.metricsRepository = metricsRepository
        return self

    def reuseExistingResultsForKey(self, resultKey, failIfResultsMissing=False):
        self._repository.need_repository("reuseExistingResultsForKey")
        self._repository.reuseExistingResultsForKey = resultKey
        self._repository.failIfResultsForReusingMissing = bool(failIfResultsMissing)
        return self

    def saveOrAppendResult(self, resultKey):
        """The run's metrics are added to what the repository holds under `resultKey`, after the checks (an anomaly
        check sees the history without the run it judges)."""
        self._repository.need_repository("saveOrAppendResult")
        self._repository.saveOrAppendResultsWithKey = resultKey
        return self

    def addAnomalyCheck(self, anomalyDetectionStrategy, analyzer, anomalyCheckConfig=None):
        """M/VerificationRunBuilder.scala:227-243: a check that the analyzer's metric of this run is no anomaly
        against its history in the repository."""
        self._repository.need_repository("addAnomalyCheck")
        config = anomalyCheckConfig
        if config is None:
            config = AnomalyCheckConfig(CheckLevel.Warning, "Anomaly check for %r" % (analyzer,))
        self.checks.append(Check(config.level, config.description).isNewestPointNonAnomalous(
            self._repository.metricsRepository, anomalyDetectionStrategy, analyzer, config.withTagValues,
            config.afterDate, config.beforeDate))
        return self

    def saveCheckResultsJsonToPath(self, path):
        self._check_results_path = path
        return self

    def saveSuccessMetricsJsonToPath(self, path):
        self._success_metrics_path = path
        return self

    def overwritePreviousFiles(self, flag):
        self._overwrite = bool(flag)
        return self

    def addCheck(self, check):
        self.checks.append(check)
        return self

    def addChecks(self, checks):
        self.checks.extend(checks)
        return self

    def addRequiredAnalyzer(self, analyzer):
        self.requiredAnalyzers.append(analyzer)
        return self

    def addRequiredAnalyzers(self, analyzers):
        self.requiredAnalyzers.extend(analyzers)
        return self

    def aggregateWith(self, stateLoader):
        self._aggregateWith = stateLoader
        return self

    def saveStatesWith(self, statePersister):
        self._saveStatesWith = statePersister
        return self

    def run(self):
        return VerificationSuite.doVerificationRun(
            self.data, self.checks, self.requiredAnalyzers, self._aggregateWith, self._saveStatesWith,
            saveCheckResultsJsonToPath=self._check_results_path,
            saveSuccessMetricsJsonToPath=self._success_metrics_path, overwriteOutputFiles=self._overwrite,
            **self._repository.arguments())


class AnomalyCheckConfig:
    """M/VerificationRunBuilder.scala:336-341."""

    def __init__(self, level, description, withTagValues=None, afterDate=None, beforeDate=None):
        self.level, self.description = level, description
        self.withTagValues = dict(withTagValues or {})
        self.afterDate, self.beforeDate = afterDate, beforeDate


class VerificationSuite:
    """M/VerificationSuite.scala:44-315."""

    def onData(self, data):
        return VerificationRunBuilder(data)

    @staticmethod
    def doVerificationRun(data, checks, requiredAnalyzers=(), aggregateWith=None, saveStatesWith=None,
                          metricsRepository=None, reuseExistingResultsForKey=None,
                          failIfResultsForReusingMissing=False, saveOrAppendResultsWithKey=None,
                          saveCheckResultsJsonToPath=None, saveSuccessMetricsJsonToPath=None,
                          overwriteOutputFiles=False):
        """M/VerificationSuite.scala:107-144: one analysis run for every check's analyzers. The run's metrics go to
        the repository after the checks are evaluated (:121-139), so that an anomaly check reads the history
        without the point it judges. The JSON outputs take local paths."""
        analyzers = list(requiredAnalyzers) + [a for c in checks for a in c.requiredAnalyzers()]
        if metricsRepository is None:
            context = AnalysisRunner.doAnalysisRun(data, analyzers, aggregateWith, saveStatesWith)
        else:
            context = AnalysisRunner.doAnalysisRun(data, analyzers, aggregateWith, saveStatesWith,
                                                   metricsRepository=metricsRepository,
                                                   reuseExistingResultsForKey=reuseExistingResultsForKey,
                                                   failIfResultsForReusingMissing=failIfResultsForReusingMissing)
        result = VerificationSuite.evaluate(checks, context)
        AnalysisRunner.saveOrAppendResultsIfNecessary(AnalyzerContext(result.metrics), metricsRepository,
                                                      saveOrAppendResultsWithKey)
        if saveCheckResultsJsonToPath is not None or saveSuccessMetricsJsonToPath is not None:
            from .suggestions import _write_text
            if saveCheckResultsJsonToPath is not None:
                _write_text(saveCheckResultsJsonToPath, VerificationResult.checkResultsAsJson(result),
                            overwriteOutputFiles, False, "CHECK RESULTS")
            if saveSuccessMetricsJsonToPath is not None:
                _write_text(saveSuccessMetricsJsonToPath, VerificationResult.successMetricsAsJson(result),
                            overwriteOutputFiles, False, "SUCCESS METRICS")
        return result

    @staticmethod
    def evaluate(checks, context):
        results = {c: c.evaluate(context) for c in checks}
        status = max([r.status for r in results.values()], default=CheckStatus.Success)
        return VerificationResult(status, results, context.metricMap)
