"""Cross-table checks: referential integrity and dataset match, as the later deequ releases ship them
(com.amazon.deequ.comparison.ReferentialIntegrity / DataSynchronization, DatasetMatchAnalyzer, Check.doesDatasetMatch).

Both are a hash semi-join. The build side is the project's frequency table over the reference table's key columns
(engine.frequencies); the probe streams the primary table's key columns through it (dq_freq_probe: one launch per
primary table or chunk). A primary row matches iff some reference row has `P.p_i = R.r_i` TRUE for every column pair
under SQL '=': a NULL component on either side never matches.
"""
from . import engine
from . import native as N
from .analyzers import Analyzer, Preconditions, metricFromFailure, metricFromValue, emptyStateException
from .checks import is_one
from .metrics import Entity, MetricCalculationRuntimeException, NoSuchColumnException, UnsupportedOnDevice
from .states import DoubleValuedState
from .table import ChunkedTable, Column, DictColumn, Table

_INTEGRAL = (N.TYPE_BYTE, N.TYPE_SHORT, N.TYPE_INT, N.TYPE_LONG)


class ComparisonResult:
    def __eq__(self, other):
        return type(self) is type(other) and self.__dict__ == other.__dict__

    def __hash__(self):
        return hash((type(self).__name__,) + tuple(self.__dict__.values()))


class ComparisonSucceeded(ComparisonResult):
    def __init__(self, ratio=0.0):
        self.ratio = float(ratio)

    def __repr__(self):
        return "ComparisonSucceeded(%r)" % self.ratio


class ComparisonFailed(ComparisonResult):
    def __init__(self, errorMessage, ratio=0.0):
        self.errorMessage, self.ratio = errorMessage, float(ratio)

    def __repr__(self):
        return "ComparisonFailed(%s,%r)" % (self.errorMessage, self.ratio)


class DatasetMatchState(DoubleValuedState):
    """Matching rows and rows of the primary table; two partitions of it against one reference add up."""

    def __init__(self, matchedDataCount, totalDataCount):
        self.matchedDataCount, self.totalDataCount = int(matchedDataCount), int(totalDataCount)

    def sum(self, other):
        return DatasetMatchState(self.matchedDataCount + other.matchedDataCount,
                                 self.totalDataCount + other.totalDataCount)

    def metricValue(self):
        return float("nan") if self.totalDataCount == 0 else self.matchedDataCount / self.totalDataCount

    def __eq__(self, o):
        if not isinstance(o, DatasetMatchState):
            return NotImplemented
        return (o.matchedDataCount, o.totalDataCount) == (self.matchedDataCount, self.totalDataCount)

    def __hash__(self):
        return hash((self.matchedDataCount, self.totalDataCount))

    def __repr__(self):
        return "DatasetMatchState(%d,%d)" % (self.matchedDataCount, self.totalDataCount)


# ---- validation: no GPU, no context -------------------------------------------------------------------------------
def _as_list(columns):
    return [columns] if isinstance(columns, str) else list(columns)


def _pairs(mapping):
    """A {primary column: reference column} mapping (or a list of pairs) as two lists."""
    items = list(mapping.items()) if hasattr(mapping, "items") else [tuple(p) for p in (mapping or [])]
    return [p for p, _ in items], [r for _, r in items]


def missing_column(primary, pcols, reference, rcols):
    """The message naming the first mapped column that a side does not have, or None."""
    for side, table, cols in (("primary", primary, pcols), ("reference", reference, rcols)):
        for c in cols:
            if c not in table:
                return "Input data does not include column %s! (the %s dataset)" % (c, side)
    return None


def pair_refusal(pname, pcol, rname, rcol):
    """Why the probe does not compare this column pair, or None when it does."""
    for name, col in ((pname, pcol), (rname, rcol)):
        if col.spark_type in (N.TYPE_FLOAT, N.TYPE_DOUBLE, N.TYPE_DECIMAL128):
            return ("column %s is %s: '=' over floating and wide-decimal cells is not the frequency table's equality"
                    % (name, col.type_name))
    if pcol.spark_type in _INTEGRAL and rcol.spark_type in _INTEGRAL:
        return None
    if pcol.spark_type != rcol.spark_type:
        return "column %s is %s but %s is %s" % (pname, pcol.type_name, rname, rcol.type_name)
    if pcol.spark_type == N.TYPE_DECIMAL and pcol.decimal_scale != rcol.decimal_scale:
        return "column %s is %s but %s is %s: decimal keys need one scale" % (pname, pcol.type_name, rname,
                                                                            rcol.type_name)
    return None


def first_refusal(primary, pcols, reference, rcols):
    for p, r in zip(pcols, rcols):
        why = pair_refusal(p, primary[p], r, reference[r])
        if why is not None:
            return why
    return None


def _validate(primary, pcols, reference, rcols):
    """The ComparisonFailed message of a call that needs no GPU to be refused, or None."""
    if not pcols or len(pcols) != len(rcols):
        return "The number of primary and reference columns must be equal and at least one (%d, %d)" % (len(pcols),
                                                                                                        len(rcols))
    return missing_column(primary, pcols, reference, rcols) or first_refusal(primary, pcols, reference, rcols)


# ---- the device side ------------------------------------------------------------------------------------------------
def _require_single(reference):
    if isinstance(reference, ChunkedTable):
        raise UnsupportedOnDevice("the reference dataset of a cross-table check must be one Table, not a ChunkedTable")
    if getattr(engine.ctx(), "multi", False):
        raise UnsupportedOnDevice("cross-table checks need a single-device context")


def _key_view(table, columns):
    """The named columns as a Table (each once); a kept dictionary column is read decoded."""
    return Table([table[c].decoded() if isinstance(table[c], DictColumn) else table[c] for c in dict.fromkeys(columns)])


def _chunks(primary):
    return primary.chunks if isinstance(primary, ChunkedTable) else [primary]


def _build(table, columns):
    """The frequency table of `columns` of `table` under the grouping's own (null-safe) semantics."""
    if isinstance(table, ChunkedTable):
        table = ChunkedTable([_key_view(ch, columns) for ch in table.chunks]).concat(list(dict.fromkeys(columns)))
    return engine.frequencies(_key_view(table, columns), list(columns))


def _groups_and_rows(ft, nrows):
    """(#groups, #rows) under GROUP BY: NULL is a key value. The build leaves out the rows whose key columns are all
    NULL (nrows - numRows of them): they are one more group."""
    return ft.num_groups + (1 if nrows > ft.num_rows else 0), nrows


def _probe(ref_table, primary, pcols, want_outcome=False):
    """One dq_freq_probe per chunk of `primary`: (matched rows, [outcome bytes tensor per chunk])."""
    matched, outcomes = 0, []
    for chunk in _chunks(primary):
        m, _, out = ref_table.probe(_key_view(chunk, pcols), pcols, want_outcome=want_outcome)
        matched += m
        outcomes.append(out)
    return matched, outcomes


def _with_outcome(primary, outcomes, name):
    """`primary` plus one BOOLEAN column of the probe's outcome bytes: in HBM for a device-resident table, on the host
    for a host table; a ChunkedTable chunk by chunk."""
    out = []
    for chunk, cells in zip(_chunks(primary), outcomes):
        n = chunk.nrows
        if all(c.device is not None for c in chunk.columns.values()):
            col = Column(name, N.TYPE_BOOLEAN, None, None, length=n)
            col.device = {"values": cells}
        else:
            col = Column(name, N.TYPE_BOOLEAN, cells[:n].cpu().numpy(), None, length=n)
        out.append(Table(list(chunk.columns.values()) + [col]))
    return ChunkedTable(out) if isinstance(primary, ChunkedTable) else out[0]


def _result(ratio, assertion):
    if assertion(ratio):
        return ComparisonSucceeded(ratio)
    return ComparisonFailed("Value: %s does not meet the constraint requirement." % ratio, ratio)


class ReferentialIntegrity:
    """com.amazon.deequ.comparison.ReferentialIntegrity: (|P| - count(P LEFT ANTI JOIN R ON p = r)) / |P|."""

    @staticmethod
    def subsetCheck(primary, primaryColumns, reference, referenceColumns, assertion=is_one):
        pcols, rcols = _as_list(primaryColumns), _as_list(referenceColumns)
        why = _validate(primary, pcols, reference, rcols)
        if why is None and primary.nrows == 0:
            why = "The primary dataset is empty: no ratio to assert on"
        if why is not None:
            return ComparisonFailed(why)
        _require_single(reference)
        matched, _ = _probe(_build(reference, rcols), primary, pcols)
        return _result(matched / primary.nrows, assertion)

    @staticmethod
    def subsetCheckRowLevel(primary, primaryColumns, reference, referenceColumns, outcomeColumnName="outcome"):
        """The primary table plus one BOOLEAN column: the row's key is among the reference's (a project extension)."""
        pcols, rcols = _as_list(primaryColumns), _as_list(referenceColumns)
        why = _validate(primary, pcols, reference, rcols)
        if why is not None:
            return ComparisonFailed(why)
        _require_single(reference)
        _, outcomes = _probe(_build(reference, rcols), primary, pcols, want_outcome=True)
        return _with_outcome(primary, outcomes, outcomeColumnName)


def _match(primary, reference, keys, comps, want_outcome=False):
    """DataSynchronization's join: (failure message or None, matched rows, outcomes). The key columns must be unique
    on both sides; the join is then over the key pairs plus the compare pairs, and its row count is `matched`."""
    (pk, rk), (pc, rc) = keys, comps
    ref_keys = _build(reference, rk)
    g2, n2 = _groups_and_rows(ref_keys, reference.nrows)
    g1, n1 = _groups_and_rows(_build(primary, pk), primary.nrows)
    if g1 != n1 or g2 != n2:
        return ("The selected columns are not comparable due to duplicates present in the dataset. Comparison keys "
                "must be unique, but in Dataframe 1, there are %d unique records and %d rows, and in Dataframe 2, "
                "there are %d unique records and %d rows, based on the combination of keys {%s} in Dataframe 1 and "
                "{%s} in Dataframe 2" % (g1, n1, g2, n2, ", ".join(pk), ", ".join(rk))), 0, None
    ref_all = _build(reference, rk + rc) if rc else ref_keys
    matched, outcomes = _probe(ref_all, primary, pk + pc, want_outcome)
    return None, matched, outcomes


class DataSynchronization:
    """com.amazon.deequ.comparison.DataSynchronization: do two datasets match row by row on a key?"""

    @staticmethod
    def _prepare(ds1, ds2, colKeyMap, compCols):
        keys, comps = _pairs(colKeyMap), _pairs(compCols)
        return keys, comps, _validate(ds1, keys[0] + comps[0], ds2, keys[1] + comps[1])

    @staticmethod
    def columnMatch(ds1, ds2, colKeyMap, compCols=None, assertion=is_one):
        keys, comps, why = DataSynchronization._prepare(ds1, ds2, colKeyMap, compCols)
        if why is None and ds1.nrows == 0:
            why = "The primary dataset is empty: no ratio to assert on"
        if why is not None:
            return ComparisonFailed(why)
        _require_single(ds2)
        why, matched, _ = _match(ds1, ds2, keys, comps)
        if why is not None:
            return ComparisonFailed(why)
        return _result(matched / ds1.nrows, assertion)

    @staticmethod
    def columnMatchRowLevel(ds1, ds2, colKeyMap, compCols=None, outcomeColumnName="outcome"):
        keys, comps, why = DataSynchronization._prepare(ds1, ds2, colKeyMap, compCols)
        if why is not None:
            return ComparisonFailed(why)
        _require_single(ds2)
        why, _, outcomes = _match(ds1, ds2, keys, comps, want_outcome=True)
        if why is not None:
            return ComparisonFailed(why)
        return _with_outcome(ds1, outcomes, outcomeColumnName)


class DatasetMatchAnalyzer(Analyzer):
    """DatasetMatchAnalyzer(dfToCompare, columnMappings, assertion, matchColumnMappings): the share of the data's rows
    that match `dfToCompare` on the key mappings (plus the match mappings), DataSynchronization.columnMatch as a metric.
    Equality is by the identity of `dfToCompare` and the mappings, as Histogram compares its UDF."""
    name = "DatasetMatch"
    entity = Entity.Dataset

    def __init__(self, dfToCompare, columnMappings, assertion=is_one, matchColumnMappings=None):
        self.dfToCompare, self.assertion = dfToCompare, assertion
        self.columnMappings = dict(columnMappings)
        self.matchColumnMappings = dict(matchColumnMappings) if matchColumnMappings else None

    def _key(self):
        return (type(self).__name__, id(self.dfToCompare), tuple(self.columnMappings.items()),
                tuple(self.matchColumnMappings.items()) if self.matchColumnMappings else None)

    def __repr__(self):
        def show(m):
            return "Map(%s)" % ", ".join("%s -> %s" % kv for kv in m.items())
        return "DatasetMatchAnalyzer(%s,%s)" % (show(self.columnMappings), "Some(%s)" % show(self.matchColumnMappings)
                                                if self.matchColumnMappings else "None")

    @property
    def instance(self):
        return ",".join(self.columnMappings)

    def _mapped(self):
        keys, comps = _pairs(self.columnMappings), _pairs(self.matchColumnMappings)
        return keys, comps

    def preconditions(self):
        keys, comps = self._mapped()

        def mappings_given(_):
            if not keys[0]:
                raise MetricCalculationRuntimeException("DatasetMatch needs at least one key column mapping")

        def reference_has_columns(_):
            for c in keys[1] + comps[1]:
                if c not in self.dfToCompare:
                    raise NoSuchColumnException("Input data does not include column %s! (the dataset to compare)" % c)
        return [mappings_given] + [Preconditions.hasColumn(c) for c in keys[0] + comps[0]] + [reference_has_columns]

    def computeStateFrom(self, data):
        keys, comps = self._mapped()
        why = first_refusal(data, keys[0] + comps[0], self.dfToCompare, keys[1] + comps[1])
        if why is not None:
            raise UnsupportedOnDevice("DatasetMatch: " + why)
        _require_single(self.dfToCompare)
        why, matched, _ = _match(data, self.dfToCompare, keys, comps)
        if why is not None:
            raise MetricCalculationRuntimeException(why)
        return DatasetMatchState(matched, data.nrows)

    def computeMetricFrom(self, state):
        if state is None:
            return metricFromFailure(emptyStateException(self), self.name, self.instance, self.entity)
        return metricFromValue(state.metricValue(), self.name, self.instance, self.entity)

    def toFailureMetric(self, exception):
        return metricFromFailure(exception, self.name, self.instance, self.entity)
