"""ConstraintSuggestionRunner (M/suggestions/ConstraintSuggestionRunner.scala, ConstraintSuggestionRunBuilder.scala,
ConstraintSuggestion.scala, ConstraintSuggestionResult.scala, rules/*.scala) on the MI355X engine.

A run profiles the table with the 3-pass ColumnProfiler, applies the rules to every column profile and, when a
train / test split was asked for, evaluates the suggested constraints on the held-out rows with VerificationSuite. The
rules, the result and its JSON are a thin host layer; the split is the part that touches every row: one dq_split_rows
launch writes the TRAIN / TEST bitmaps and dq_gather_rows compacts every column under each ("Constraint
suggestion"). The metrics repository options (useRepository, reuseExistingResultsForKey, saveOrAppendResult) are not
part of this engine.
"""
import decimal
import json
import math
import os
import random

from . import native as N
from .analyzers import Histogram, _java_double_to_string
from .checks import Check, CheckLevel, ConstrainableDataTypes, VerificationSuite, is_one
from .profiles import ColumnProfiler, ColumnProfilerRunner, ColumnProfiles, DataTypeInstances, NumericColumnProfile
from .schema import _device_view, _gather, _to_host
from .table import ChunkedTable, Table

_U64 = (1 << 64) - 1
_TESTSET_RATIO_MESSAGE = "Testset ratio must be in ]0, 1["


# ---- train / test split -----------------------------------------------------------------------------------------------
def split_train_test(data, testsetRatio, seed=None):
    """(train, test, seed_used): every row goes to the test set independently with probability testsetRatio, decided
    by dq_split_rows from (seed, global row index, ratio) alone: a ChunkedTable and its concatenation split the same
    way, and a run is repeated by passing seed_used again. `seed` is a Java Long (taken modulo 2^64); None draws 63
    random bits. Host-resident tables are split on the device and come back host-resident."""
    if not (isinstance(testsetRatio, (int, float)) and 0 < testsetRatio < 1.0):
        raise ValueError(_TESTSET_RATIO_MESSAGE)
    if seed is None:
        seed = random.getrandbits(63)
    seed = int(seed)
    if isinstance(data, ChunkedTable):
        trains, tests, row0 = [], [], 0
        for chunk in data.chunks:
            tr, te = _split_table(chunk, testsetRatio, seed, row0)
            trains.append(tr)
            tests.append(te)
            row0 += chunk.nrows
        return ChunkedTable(trains), ChunkedTable(tests), seed
    train, test = _split_table(data, testsetRatio, seed, 0)
    return train, test, seed


def _split_table(data, ratio, seed, row0):
    import torch
    from . import engine
    ctx = engine.ctx()
    if ctx.multi:
        raise N.NativeError(-2, "split_train_test: multi-device contexts are not supported")
    dev = torch.device("cuda", engine.device())
    work, on_device = _device_view(data, engine.device())
    n = data.nrows
    nbitmap = max((n + 63) // 64, 1) * 8
    train_bits, test_bits = (torch.zeros(nbitmap, dtype=torch.uint8, device=dev) for _ in range(2))
    ntrain, ntest = ctx.split_rows(n, row0, seed & _U64, ratio, train_bits.data_ptr(), test_bits.data_ptr())
    names = list(work.columns)
    train = [_gather(ctx, torch, dev, work[c], n, train_bits, ntrain) for c in names]
    test = [_gather(ctx, torch, dev, work[c], n, test_bits, ntest) for c in names]
    if not on_device:
        train = [_to_host(c) for c in train]
        test = [_to_host(c) for c in test]
    return Table(train), Table(test)


# ---- formatting helpers -----------------------------------------------------------------------------------------------
def _jd(v):
    return _java_double_to_string(float(v))


def _round_down_2(x):
    """BigDecimal(x).setScale(2, RoundingMode.DOWN).toDouble: scala's BigDecimal(Double) reads Double.toString(x), so
    the decimal digits of the shortest representation are truncated (0.4 stays 0.4, 0.39999999999999997 gives 0.39)."""
    if math.isnan(x) or math.isinf(x):
        raise ValueError("NumberFormatException: %r has no BigDecimal" % x)
    d = decimal.Decimal(_java_double_to_string(x))
    return float(d.quantize(decimal.Decimal("0.01"), rounding=decimal.ROUND_DOWN))


def _lower_confidence_bound(p, n):
    z = 1.96
    if n == 0:
        raise ValueError("NumberFormatException: no records")
    return _round_down_2(p - z * math.sqrt(p * (1 - p) / n))


_JAVA_CTRL = {"\b": "\\b", "\n": "\\n", "\t": "\\t", "\f": "\\f", "\r": "\\r"}


def _escape_java(s):
    """commons-lang3 StringEscapeUtils.escapeJava: `"` and `\\` escaped, \\b \\n \\t \\f \\r by name, every other UTF-16
    code unit below 32 or above 0x7f as \\uXXXX (upper-case hex; a supplementary character as its surrogate pair)."""
    out = []
    for ch in s:
        cp = ord(ch)
        if ch == '"':
            out.append('\\"')
        elif ch == "\\":
            out.append("\\\\")
        elif ch in _JAVA_CTRL:
            out.append(_JAVA_CTRL[ch])
        elif cp < 32 or cp > 0x7F:
            if cp > 0xFFFF:
                cp -= 0x10000
                out.append("\\u%04X\\u%04X" % (0xD800 + (cp >> 10), 0xDC00 + (cp & 0x3FF)))
            else:
                out.append("\\u%04X" % cp)
        else:
            out.append(ch)
    return "".join(out)


def _by_popularity(items):
    """Histogram entries without the NULL bucket, by count descending, ties by key ascending."""
    return sorted(((k, v) for k, v in items if k != Histogram.NullFieldReplacement),
                  key=lambda kv: (-kv[1].absolute, kv[0]))


def _categories_sql(entries):
    return ", ".join("'%s'" % k.replace("'", "''") for k, _ in entries)


def _categories_code(entries):
    return ", ".join('"%s"' % _escape_java(k) for k, _ in entries)


def _unique_value_ratio(profile):
    """The share of histogram entries seen exactly once, or None without a String histogram / with an empty one
    (0 / 0 is NaN in the reference, which fails both thresholds)."""
    if profile.histogram is None or profile.dataType != DataTypeInstances.String:
        return None
    entries = profile.histogram.values
    if not entries:
        return None
    return sum(1 for v in entries.values() if v.absolute == 1) / len(entries)


def _last_constraint(check):
    return check.constraints[-1]


def _check():
    return Check(CheckLevel.Warning, "suggestion")


class ConstraintSuggestion:
    """M/suggestions/ConstraintSuggestion.scala:25-32."""

    def __init__(self, constraint, columnName, currentValue, description, suggestingRule, codeForConstraint):
        self.constraint, self.columnName, self.currentValue = constraint, columnName, currentValue
        self.description, self.suggestingRule, self.codeForConstraint = description, suggestingRule, codeForConstraint

    def __repr__(self):
        return "ConstraintSuggestion(%r,%s,%s,%s,%r,%s)" % (self.constraint, self.columnName, self.currentValue,
                                                           self.description, self.suggestingRule,
                                                           self.codeForConstraint)


# ---- rules ------------------------------------------------------------------------------------------------------------
class ConstraintRule:
    """M/suggestions/rules/ConstraintRule.scala: decides from a column profile whether to suggest a constraint, and
    builds the suggestion. The constraints come from the Check DSL, so they are named and evaluated as the same
    constraint written by hand."""
    ruleDescription = ""

    def shouldBeApplied(self, profile, numRecords):
        raise NotImplementedError

    def candidate(self, profile, numRecords):
        raise NotImplementedError

    def __repr__(self):
        return "%s()" % type(self).__name__

    def __eq__(self, other):
        return type(self) is type(other) and repr(self) == repr(other)

    def __hash__(self):
        return hash(repr(self))


class CompleteIfCompleteRule(ConstraintRule):
    """rules/CompleteIfCompleteRule.scala."""
    ruleDescription = "If a column is complete in the sample, we suggest a NOT NULL constraint"

    def shouldBeApplied(self, profile, numRecords):
        return profile.completeness == 1.0

    def candidate(self, profile, numRecords):
        constraint = _last_constraint(_check().isComplete(profile.column))
        return ConstraintSuggestion(constraint, profile.column, "Completeness: " + _jd(profile.completeness),
                                    "'%s' is not null" % profile.column, self, '.isComplete("%s")' % profile.column)


class RetainCompletenessRule(ConstraintRule):
    """rules/RetainCompletenessRule.scala: the completeness as a binomial variable; the lower end of its 95 %
    interval, cut to two decimals, is the suggested bound."""
    ruleDescription = ("If a column is incomplete in the sample, we model its completeness as a binomial variable, "
                       "estimate a confidence interval and use this to define a lower bound for the completeness")

    def shouldBeApplied(self, profile, numRecords):
        return 0.2 < profile.completeness < 1.0

    def candidate(self, profile, numRecords):
        target = _lower_confidence_bound(profile.completeness, numRecords)
        constraint = _last_constraint(_check().hasCompleteness(profile.column, lambda v: v >= target))
        bound_in_percent = int((1.0 - target) * 100)
        code = '.hasCompleteness("%s", _ >= %s, Some("It should be above %s!"))' % (profile.column, _jd(target),
                                                                                   _jd(target))
        return ConstraintSuggestion(constraint, profile.column, "Completeness: " + _jd(profile.completeness),
                                    "'%s' has less than %d%% missing values" % (profile.column, bound_in_percent),
                                    self, code)


class RetainTypeRule(ConstraintRule):
    """rules/RetainTypeRule.scala."""
    ruleDescription = "If we detect a non-string type, we suggest a type constraint"
    _TESTABLE = (DataTypeInstances.Integral, DataTypeInstances.Fractional, DataTypeInstances.Boolean)

    def shouldBeApplied(self, profile, numRecords):
        return bool(profile.isDataTypeInferred) and profile.dataType in self._TESTABLE

    def candidate(self, profile, numRecords):
        if profile.dataType not in self._TESTABLE:
            raise ValueError("MatchError: %s" % profile.dataType)
        constraint = _last_constraint(_check().hasDataType(profile.column, ConstrainableDataTypes[profile.dataType]))
        return ConstraintSuggestion(constraint, profile.column, "DataType: %s" % profile.dataType,
                                    "'%s' has type %s" % (profile.column, profile.dataType), self,
                                    '.hasDataType("%s", ConstrainableDataTypes.%s)' % (profile.column,
                                                                                       profile.dataType))


class CategoricalRangeRule(ConstraintRule):
    """rules/CategoricalRangeRule.scala.

    Divergence: among categories with equal counts the reference lists them in the order of the JVM's hash map; here
    the order of the IN list is count descending, then key ascending."""
    ruleDescription = "If we see a categorical range for a column, we suggest an IS IN (...) constraint"

    def shouldBeApplied(self, profile, numRecords):
        ratio = _unique_value_ratio(profile)
        return ratio is not None and ratio <= 0.1

    def candidate(self, profile, numRecords):
        entries = _by_popularity(profile.histogram.values.items())
        sql = _categories_sql(entries)
        description = "'%s' has value range %s" % (profile.column, sql)
        condition = "`%s` IN (%s)" % (profile.column, sql)
        constraint = _last_constraint(_check().satisfies(condition, description, is_one))
        return ConstraintSuggestion(constraint, profile.column, "Compliance: 1", description, self,
                                    '.isContainedIn("%s", Array(%s))' % (profile.column, _categories_code(entries)))


class FractionalCategoricalRangeRule(ConstraintRule):
    """rules/FractionalCategoricalRangeRule.scala: the most frequent categories that cover targetDataCoverageFraction
    of the rows, and the lower end of the 95 % interval of their coverage as the compliance bound.

    Divergence: among categories with equal ratios the reference admits them in the order of the JVM's hash map; here
    categories are admitted by ratio descending, then count descending, then key ascending, and listed by count
    descending, then key ascending. So which of two tied categories makes it into the range, and the order of the IN
    list, are defined here and arbitrary there."""
    ruleDescription = ("If we see a categorical range for most values in a column, we suggest an IS IN (...) "
                       "constraint that should hold for most values")

    def __init__(self, targetDataCoverageFraction=0.9):
        self.targetDataCoverageFraction = float(targetDataCoverageFraction)

    def __repr__(self):
        return "FractionalCategoricalRangeRule(%s)" % _jd(self.targetDataCoverageFraction)

    def _top_categories(self, profile):
        ordered = sorted(profile.histogram.values.items(), key=lambda kv: (-kv[1].ratio, -kv[1].absolute, kv[0]))
        coverage, top = 0.0, []
        for k, v in ordered:
            if coverage < self.targetDataCoverageFraction:
                coverage += v.ratio
                top.append((k, v))
        return top

    def shouldBeApplied(self, profile, numRecords):
        ratio = _unique_value_ratio(profile)
        if ratio is None:
            return False
        return ratio <= 0.4 and sum(v.ratio for _, v in self._top_categories(profile)) < 1

    def candidate(self, profile, numRecords):
        top = self._top_categories(profile)
        ratio_sums = sum(v.ratio for _, v in top)
        entries = _by_popularity(top)
        sql = _categories_sql(entries)
        target = _lower_confidence_bound(ratio_sums, numRecords)
        description = "'%s' has value range %s for at least %s%% of values" % (profile.column, sql, _jd(target * 100))
        condition = "`%s` IN (%s)" % (profile.column, sql)
        hint = "It should be above %s!" % _jd(target)
        constraint = _last_constraint(_check().satisfies(condition, description, lambda v: v >= target, hint))
        code = '.isContainedIn("%s", Array(%s), _ >= %s, Some("%s"))' % (profile.column, _categories_code(entries),
                                                                        _jd(target), hint)
        return ConstraintSuggestion(constraint, profile.column, "Compliance: " + _jd(ratio_sums), description, self,
                                    code)


class NonNegativeNumbersRule(ConstraintRule):
    """rules/NonNegativeNumbersRule.scala (the predicate names the column unquoted, as the reference does)."""
    ruleDescription = "If we see only non-negative numbers in a column, we suggest a corresponding constraint"

    def shouldBeApplied(self, profile, numRecords):
        return isinstance(profile, NumericColumnProfile) and profile.minimum is not None and profile.minimum >= 0.0

    def candidate(self, profile, numRecords):
        description = "'%s' has no negative values" % profile.column
        constraint = _last_constraint(_check().satisfies("%s >= 0" % profile.column, description, is_one))
        if isinstance(profile, NumericColumnProfile) and profile.minimum is not None:
            minimum = _jd(profile.minimum)
        else:
            minimum = "Error while calculating minimum!"
        return ConstraintSuggestion(constraint, profile.column, "Minimum: " + minimum, description, self,
                                    '.isNonNegative("%s")' % profile.column)


class UniqueIfApproximatelyUniqueRule(ConstraintRule):
    """rules/UniqueIfApproximatelyUniqueRule.scala (not one of Rules.DEFAULT)."""
    ruleDescription = ("If the ratio of approximate num distinct values in a column is close to the number of records "
                       "(within the error of the HLL sketch), we suggest a UNIQUE constraint")

    @staticmethod
    def _approximate_distinctness(profile, numRecords):
        n = float(profile.approximateNumDistinctValues)
        if numRecords == 0:
            return float("nan") if n == 0 else math.copysign(float("inf"), n)
        return n / numRecords

    def shouldBeApplied(self, profile, numRecords):
        d = self._approximate_distinctness(profile, numRecords)
        return profile.completeness == 1.0 and abs(1.0 - d) <= 0.08

    def candidate(self, profile, numRecords):
        constraint = _last_constraint(_check().hasUniqueness([profile.column], is_one))
        d = self._approximate_distinctness(profile, numRecords)
        return ConstraintSuggestion(constraint, profile.column, "ApproxDistinctness: " + _jd(d),
                                    "'%s' is unique" % profile.column, self, '.isUnique("%s")' % profile.column)


class Rules:
    """ConstraintSuggestionRunner.scala:30-36."""
    DEFAULT = (CompleteIfCompleteRule(), RetainCompletenessRule(), RetainTypeRule(), CategoricalRangeRule(),
               FractionalCategoricalRangeRule(), NonNegativeNumbersRule())


# ---- JSON -------------------------------------------------------------------------------------------------------------
class ConstraintSuggestions:
    """ConstraintSuggestion.scala:34-115. Gson's pretty printing is not reproduced byte for byte: parity is on the
    parsed document."""
    _FIELD = "constraint_suggestions"

    @staticmethod
    def _shared(s):
        return {"constraint_name": repr(s.constraint), "column_name": s.columnName, "current_value": s.currentValue,
                "description": s.description, "suggesting_rule": repr(s.suggestingRule),
                "rule_description": s.suggestingRule.ruleDescription, "code_for_constraint": s.codeForConstraint}

    @staticmethod
    def toJson(constraintSuggestions):
        return json.dumps({ConstraintSuggestions._FIELD: [ConstraintSuggestions._shared(s)
                                                          for s in constraintSuggestions]}, indent=2)

    @staticmethod
    def evaluationResultsToJson(constraintSuggestions, result):
        """Every suggestion with the status of its constraint in the first check of `result` ("Unknown" where the
        check has no result for it, or `result` is None)."""
        statuses = []
        if result is not None:
            for check_result in result.checkResults.values():
                statuses = [r.status.value for r in check_result.constraintResults]
                break
        out = []
        for i, s in enumerate(constraintSuggestions):
            j = ConstraintSuggestions._shared(s)
            j["constraint_result_on_test_set"] = statuses[i] if i < len(statuses) else "Unknown"
            out.append(j)
        return json.dumps({ConstraintSuggestions._FIELD: out}, indent=2)


class ConstraintSuggestionResult:
    """ConstraintSuggestionResult.scala, plus testsetSplitRandomSeed: the seed the split used (None without a split),
    so a run with a drawn seed can be repeated."""

    def __init__(self, columnProfiles, numRecordsUsedForProfiling, constraintSuggestions, verificationResult=None,
                 testsetSplitRandomSeed=None):
        self.columnProfiles = columnProfiles
        self.numRecordsUsedForProfiling = numRecordsUsedForProfiling
        self.constraintSuggestions = constraintSuggestions
        self.verificationResult = verificationResult
        self.testsetSplitRandomSeed = testsetSplitRandomSeed

    def _all_suggestions(self):
        return [s for group in self.constraintSuggestions.values() for s in group]

    @staticmethod
    def getColumnProfilesAsJson(result):
        return ColumnProfiles.toJson(list(result.columnProfiles.values()))

    @staticmethod
    def getConstraintSuggestionsAsJson(result):
        return ConstraintSuggestions.toJson(result._all_suggestions())

    @staticmethod
    def getEvaluationResultsAsJson(result):
        return ConstraintSuggestions.evaluationResultsToJson(result._all_suggestions(), result.verificationResult)


# ---- runner -----------------------------------------------------------------------------------------------------------
def _write_text(path, text, overwrite, printStatusUpdates, what):
    if printStatusUpdates:
        print("### WRITING %s TO %s" % (what, path))
    if os.path.exists(path) and not overwrite:
        raise FileExistsError("%s exists: overwritePreviousFiles(True) replaces it" % path)
    with open(path, "w") as f:
        f.write(text)
        f.write("\n")


class ConstraintSuggestionRunBuilder:
    """ConstraintSuggestionRunBuilder.scala (the file outputs take local paths; no repository options)."""

    def __init__(self, data):
        self.data = data
        self._rules = []
        self._print = False
        self._testset_ratio = None
        self._testset_seed = None
        self._threshold = ColumnProfiler.DEFAULT_CARDINALITY_THRESHOLD
        self._restrict = None
        self._kll = None
        self._predefined = {}
        self._profiles_path = self._suggestions_path = self._evaluation_path = None
        self._overwrite = False

    def addConstraintRule(self, constraintRule):
        self._rules.append(constraintRule)
        return self

    def addConstraintRules(self, constraintRules):
        self._rules.extend(constraintRules)
        return self

    def printStatusUpdates(self, flag):
        self._print = bool(flag)
        return self

    def cacheInputs(self, flag):  # Spark caching has no analogue: inputs stay resident in HBM
        return self

    def useTrainTestSplitWithTestsetRatio(self, testsetRatio, seed=None):
        """Suggest from 1 - testsetRatio of the rows and evaluate the suggestions on the rest; `seed` (a Java Long)
        makes the split repeatable, None draws one (reported as the result's testsetSplitRandomSeed)."""
        self._testset_ratio = testsetRatio
        self._testset_seed = seed
        return self

    def withLowCardinalityHistogramThreshold(self, threshold):
        self._threshold = int(threshold)
        return self

    def restrictToColumns(self, columns):
        self._restrict = list(columns)
        return self

    def setKLLParameters(self, kllParameters):
        self._kll = kllParameters
        return self

    def setPredefinedTypes(self, dataTypes):
        self._predefined = dict(dataTypes)
        return self

    def saveColumnProfilesJsonToPath(self, path):
        self._profiles_path = path
        return self

    def saveConstraintSuggestionsJsonToPath(self, path):
        self._suggestions_path = path
        return self

    def saveEvaluationResultsJsonToPath(self, path):
        self._evaluation_path = path
        return self

    def overwritePreviousFiles(self, flag):
        self._overwrite = bool(flag)
        return self

    def run(self):
        """ConstraintSuggestionRunner.run (ConstraintSuggestionRunner.scala:63-136)."""
        ratio = self._testset_ratio
        if ratio is not None and not (isinstance(ratio, (int, float)) and 0 < ratio < 1.0):
            raise ValueError(_TESTSET_RATIO_MESSAGE)
        training, test, seed = self.data, None, None
        if ratio is not None:
            training, test, seed = split_train_test(self.data, ratio, self._testset_seed)

        profiles, suggestions = ConstraintSuggestionRunner.profileAndSuggest(
            training, self._rules, self._restrict, self._threshold, self._print, self._kll, self._predefined)
        if self._profiles_path is not None:
            _write_text(self._profiles_path, ColumnProfiles.toJson(list(profiles.profiles.values())), self._overwrite,
                        self._print, "COLUMN PROFILES")
        if self._suggestions_path is not None:
            _write_text(self._suggestions_path, ConstraintSuggestions.toJson(suggestions), self._overwrite,
                        self._print, "CONSTRAINTS")

        verification = None
        if test is not None:
            if self._print:
                print("### RUNNING EVALUATION")
            generated = Check(CheckLevel.Warning, "generated constraints", [s.constraint for s in suggestions])
            verification = VerificationSuite().onData(test).addCheck(generated).run()
            if self._evaluation_path is not None:
                _write_text(self._evaluation_path,
                            ConstraintSuggestions.evaluationResultsToJson(suggestions, verification), self._overwrite,
                            self._print, "EVALUATION RESULTS")

        by_column = {}
        for s in suggestions:
            by_column.setdefault(s.columnName, []).append(s)
        return ConstraintSuggestionResult(profiles.profiles, profiles.numRecords, by_column, verification, seed)


class ConstraintSuggestionRunner:
    """ConstraintSuggestionRunner.scala:57-341."""

    def onData(self, data):
        return ConstraintSuggestionRunBuilder(data)

    @staticmethod
    def applyRules(constraintRules, profiles, columns):
        """Every rule that applies to a column's profile, in column order then rule order (:211-226)."""
        out = []
        for column in columns:
            profile = profiles.profiles[column]
            out += [r.candidate(profile, profiles.numRecords) for r in constraintRules
                    if r.shouldBeApplied(profile, profiles.numRecords)]
        return out

    @staticmethod
    def profileAndSuggest(trainingData, constraintRules, restrictToColumns=None,
                          lowCardinalityHistogramThreshold=ColumnProfiler.DEFAULT_CARDINALITY_THRESHOLD,
                          printStatusUpdates=False, kllParameters=None, predefinedTypes=None):
        """(:161-209): the profiler run with the builder's options, then the rules on the relevant columns in schema
        order."""
        builder = ColumnProfilerRunner().onData(trainingData).printStatusUpdates(printStatusUpdates) \
            .withLowCardinalityHistogramThreshold(lowCardinalityHistogramThreshold)
        if restrictToColumns is not None:
            builder = builder.restrictToColumns(restrictToColumns)
        builder = builder.setKLLParameters(kllParameters).setPredefinedTypes(predefinedTypes or {})
        profiles = builder.run()
        relevant = [f for f in trainingData.fieldNames if restrictToColumns is None or f in restrictToColumns]
        return profiles, ConstraintSuggestionRunner.applyRules(constraintRules, profiles, relevant)
