"""Row-level results: one BOOLEAN pass / fail column per Check, computed on the GPU.

`VerificationResult.rowLevelResultsAsTable(result, data)` -- rowLevelResultsAsDataFrame of later deequ releases --
returns the input plus one column per check: row i of a check's column is the AND of the outcomes of the check's
row-level constraints on row i. Every piece is a per-row bitmap on the device already (a predicate's TRUE bitmap, a
column's validity, one probe of the frequency table per row); `plan_row_level` maps the constraints of the checks onto
such terms on the host, and the driver hands them to dq_row_outcomes, whose single kernel launch writes every check's
column, its pass bitmap and the counts next to the table in HBM. The failed / passed rows are device compactions by
those bitmaps (dq_gather_rows), not a round trip through the host.
"""
import numpy as np

from . import analyzers as A
from . import native as N
from .metrics import UnsupportedOnDevice
from .table import ChunkedTable, Column, DictColumn, Table

FILTERED_ROW_OUTCOMES = ("true", "null")
UNIQUENESS_ANALYZERS = (A.Uniqueness, A.UniqueValueRatio)


class RowTerm:
    """One row-level constraint as the kernel sees it. `kind`: N.ROW_NOT_NULL (`column`), N.ROW_PREDICATE
    (`predicate`: index into the plan's batch.preds) or N.ROW_BITS (`columns`: the uniqueness keys; `where_text`: the
    filter their frequency table is built under). `where`: predicate index of the filter, -1 = none (ROW_BITS: -1, the
    filter is in the table's rows)."""

    def __init__(self, check, description, constraint, analyzer, kind, column=None, predicate=-1, where=-1,
                 columns=None, where_text=None):
        self.check, self.description, self.constraint, self.analyzer = check, description, constraint, analyzer
        self.kind, self.column, self.predicate, self.where = kind, column, predicate, where
        self.columns, self.where_text = columns, where_text

    def __repr__(self):
        return "RowTerm(%s, %r, kind=%d)" % (self.description, self.analyzer, self.kind)


class RowLevelPlan:
    """`descriptions`: the checks that get a column (those with a row-level constraint), in order; `terms`: RowTerm
    with `check` an index into them; `skipped`: (check description, constraint, reason); `batch`: the ScanBatch whose
    `preds` the terms index (each distinct predicate text compiled once)."""

    def __init__(self, descriptions, terms, skipped, batch):
        self.descriptions, self.terms, self.skipped, self.batch = descriptions, terms, skipped, batch


def _analyzer_of(constraint):
    inner = getattr(constraint, "inner", constraint)
    return getattr(inner, "analyzer", None)


def _is_row_level(analyzer):
    return isinstance(analyzer, (A.Completeness, A.Compliance, A.PatternMatch) + UNIQUENESS_ANALYZERS)


def check_names(checks, data):
    """Two checks of one description, or a description that is a column of `data`: ValueError before any GPU work."""
    seen = set()
    for c in checks:
        if c.description in seen:
            raise ValueError("two checks are described as %r: a check's row-level column is named by its description"
                             % c.description)
        seen.add(c.description)
        if c.description in data:
            raise ValueError("check description %r is a column of the data" % c.description)


def plan_row_level(checks, data, metrics, strict=False, chunked=False):
    """The row-level terms of `checks` over `data` (a Table; only its column names and types are read): pure host code.
    A constraint is recognised by its analyzer (Completeness, Compliance, PatternMatch, Uniqueness, UniqueValueRatio);
    its assertion plays no part. Every other analyzer has no row-level form and is ignored. A term that cannot be
    evaluated -- its metric in `metrics` is a Failure, its predicate or regex does not compile (or reads a DECIMAL128
    column), or it is a uniqueness term of a `chunked` table -- goes to `skipped`, or raises with `strict`."""
    from .runners import ScanBatch
    batch = ScanBatch(data)
    descriptions, terms, skipped = [], [], []

    def skip(check, constraint, reason, cause=None):
        if strict:
            raise UnsupportedOnDevice("check %r: %r has no row-level result: %s" % (check.description, constraint, reason)) \
                from cause
        skipped.append((check.description, constraint, reason))

    for check in checks:
        index = None
        for constraint in check.constraints:
            a = _analyzer_of(constraint)
            if not _is_row_level(a):
                continue
            if index is None:
                index = len(descriptions)
                descriptions.append(check.description)
            metric = metrics.get(a) if metrics is not None else None
            if metric is not None and metric.value.isFailure:
                skip(check, constraint, "its metric failed: %s" % (metric.value.failed,))
                continue
            common = dict(check=index, description=check.description, constraint=constraint, analyzer=a)
            if isinstance(a, UNIQUENESS_ANALYZERS):
                if chunked:
                    skip(check, constraint, "uniqueness over a ChunkedTable: a group spans chunks")
                    continue
                missing = [c for c in a.columns if c not in data]
                if missing or not a.columns:
                    skip(check, constraint, "no column %s" % (missing[0] if missing else "given"))
                    continue
                terms.append(RowTerm(kind=N.ROW_BITS, columns=list(a.columns), where_text=a.where, **common))
                continue
            try:
                where = batch.predicate(a.where) if a.where is not None else -1
                if isinstance(a, A.Completeness):
                    if a.column not in data:
                        raise KeyError("no column %s" % a.column)
                    term = RowTerm(kind=N.ROW_NOT_NULL, column=a.column, where=where, **common)
                elif isinstance(a, A.PatternMatch):
                    col = data[a.column] if a.column in data else None
                    if col is not None and col.spark_type == N.TYPE_TIMESTAMP and getattr(col, "tz", None) not in A.UTC_ZONES:
                        raise UnsupportedOnDevice("PatternMatch over TIMESTAMP column %s outside a UTC session time zone"
                                                  % a.column)
                    term = RowTerm(kind=N.ROW_PREDICATE, predicate=batch.regex_predicate(a.column, a.pattern_),
                                   where=where, **common)
                else:
                    term = RowTerm(kind=N.ROW_PREDICATE, predicate=batch.predicate(a.predicate), where=where, **common)
            except Exception as e:  # the compilers' own exceptions: syntax, unknown column, regex, DECIMAL128
                skip(check, constraint, "%s: %s" % (type(e).__name__, e), e)
                continue
            terms.append(term)
    return RowLevelPlan(descriptions, terms, skipped, batch)


class RowLevelResults:
    """What rowLevelResultsAsTable returns.

    table          the data's columns plus one BOOLEAN column per check with a row-level constraint (a ChunkedTable for
                   a ChunkedTable); on the device for a device table, on the host for a host table
    checkColumns   {check description: column name}
    passedRows / failedRows / nullRows   {check description: rows whose outcome is TRUE / FALSE / NULL}
    termCounts     [(check description, constraint, matched, considered)] per evaluated constraint
    skipped        [(check description, constraint, reason)]: constraints left out of their check's AND
    """

    def __init__(self, table, checkColumns, passedRows, failedRows, nullRows, termCounts, skipped, parts=None):
        self.table, self.checkColumns = table, checkColumns
        self.passedRows, self.failedRows, self.nullRows = passedRows, failedRows, nullRows
        self.termCounts, self.skipped = termCounts, skipped
        self._parts = parts  # per chunk results of a ChunkedTable
        self._work = self._bits = self._nrows = self._on_device = self._device = None

    def _select(self, check, failed):
        """(device bitmap, set bits): rows FALSE under `check` (any check for None), or TRUE (under every check)."""
        import torch
        names = list(self.checkColumns) if check is None else [check]
        for n in names:
            if n not in self._bits:
                raise KeyError("no row-level column for check %r" % n)
        n = self._nrows
        sel = None
        for name in names:
            passed, validity = self._bits[name]
            if failed:  # FALSE: not TRUE and, under filteredRow="null", not NULL
                b = ~passed if validity is None else validity & ~passed
                sel = b if sel is None else sel | b
            else:
                sel = passed if sel is None else sel & passed
        if sel is None:  # no check columns: nothing failed, everything passed
            sel = torch.full((max((n + 63) // 64, 1) * 8,), 0 if failed else 255, dtype=torch.uint8,
                             device=torch.device("cuda", self._device))
        sel = sel.clone()
        if failed or not names:  # `~` and the fill set the bits past nrows: clear them
            sel[(n + 7) // 8:] = 0
            if n & 7:
                sel[n >> 3] &= (1 << (n & 7)) - 1
        return sel, int(_POPCOUNT8.to(sel.device)[sel.long()].sum().item())

    def _rows(self, check, failed):
        import torch
        from . import engine
        from .schema import _gather, _to_host
        if self._parts is not None:
            return ChunkedTable([p._rows(check, failed) for p in self._parts])
        ctx = engine.ctx()
        dev = torch.device("cuda", self._device)
        sel, nsel = self._select(check, failed)
        cols = [_gather(ctx, torch, dev, c.decoded() if isinstance(c, DictColumn) else c, self._nrows, sel, nsel)
                for c in self._work.columns.values()]
        return Table(cols if self._on_device else [_to_host(c) for c in cols])

    def failedRowsTable(self, check=None):
        """The data's rows whose outcome under `check` (a description; None: under any check) is FALSE, compacted on
        the device."""
        return self._rows(check, True)

    def passedRowsTable(self, check=None):
        """The data's rows whose outcome under `check` (None: under every check) is TRUE."""
        return self._rows(check, False)


_POPCOUNT8 = None


def _init_popcount():
    global _POPCOUNT8
    if _POPCOUNT8 is None:
        import torch
        _POPCOUNT8 = torch.from_numpy(np.array([bin(i).count("1") for i in range(256)], dtype=np.int64))


def _uniqueness_bits(ctx, torch, dev, work, columns, where):
    """dq_freq_row_bits over the frequency table of `columns` of `work` under `where`, built as
    FrequencyBasedAnalyzer.computeStateFrom builds it: (unique bitmap, participating bitmap) in HBM."""
    from . import engine
    columns = list(dict.fromkeys(columns))
    view = engine.FilterCache().view(work, where, columns) if where is not None else work
    # a dictionary-encoded key is read decoded: the table must be built over the table's own rows to be probed by row
    keys = Table([view[c].decoded() if isinstance(view[c], DictColumn) else view[c] for c in columns])
    table = A.computeFrequencies(keys, columns).frequencies
    nbytes = max((work.nrows + 63) // 64, 1) * 8
    unique = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    part = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ctx.freq_row_bits(table.handle, unique.data_ptr(), part.data_ptr(), work.nrows)
    return unique, part


def _run_table(checks, data, metrics, null_mode, strict, chunked=False):
    import torch
    from . import engine
    from .schema import _device_view, _to_host
    ctx = engine.ctx()
    if getattr(ctx, "multi", False):
        raise UnsupportedOnDevice("row-level results need a single-device context")
    _init_popcount()
    device = engine.device()
    dev = torch.device("cuda", device)
    work, on_device = _device_view(data, device)
    plan = plan_row_level(checks, work, metrics, strict, chunked)
    batch, n = plan.batch, work.nrows
    skipped = list(plan.skipped)

    # the uniqueness terms' bitmaps, one table per distinct (keys, where)
    bits, terms = {}, []
    for t in plan.terms:
        if t.kind == N.ROW_BITS:
            key = (tuple(t.columns), t.where_text)
            if key not in bits:
                try:
                    bits[key] = _uniqueness_bits(ctx, torch, dev, work, t.columns, t.where_text)
                except Exception as e:  # e.g. a table without a slot table to probe (DQ_ERR_UNSUPPORTED), wide decimals
                    bits[key] = e
            if isinstance(bits[key], Exception):
                if strict:
                    raise UnsupportedOnDevice("check %r: %r has no row-level result: %s"
                                              % (t.description, t.constraint, bits[key])) from bits[key]
                skipped.append((t.description, t.constraint, "%s: %s" % (type(bits[key]).__name__, bits[key])))
                continue
        terms.append(t)

    ndesc = len(plan.descriptions)
    nwords = max((n + 63) // 64, 1)
    outs = []
    for _ in range(ndesc):
        passed = torch.zeros(nwords * 8, dtype=torch.uint8, device=dev)
        values = torch.zeros(max((n + 15) // 16, 1) * 16, dtype=torch.uint8, device=dev)
        validity = torch.zeros(nwords * 8, dtype=torch.uint8, device=dev) if null_mode else None
        outs.append((passed, values, validity))
    check_counts = [(0, 0)] * ndesc
    term_counts = []

    # native calls of at most ROW_MAX_CHECKS checks and ROW_MAX_TERMS terms, split by check
    by_check = [[t for t in terms if t.check == c] for c in range(ndesc)]
    for ts in by_check:
        if len(ts) > N.ROW_MAX_TERMS:
            raise UnsupportedOnDevice("check %r has %d row-level constraints, at most %d" % (ts[0].description, len(ts),
                                                                                          N.ROW_MAX_TERMS))
    at = 0
    while at < ndesc:
        end, nt = at, 0
        while end < ndesc and end - at < N.ROW_MAX_CHECKS and nt + len(by_check[end]) <= N.ROW_MAX_TERMS:
            nt += len(by_check[end])
            end += 1
        group = [t for c in range(at, end) for t in by_check[c]]
        used = sorted({p for t in group for p in (t.predicate, t.where) if p >= 0})
        remap = {p: i for i, p in enumerate(used)}
        decoded = set().union(*[batch._pred_columns(p) for p in used]) if used else set()
        cols = batch.native_columns(decoded)
        nterms = []
        for t in group:
            nt_ = N.DqRowTerm()
            nt_.kind, nt_.check = t.kind, t.check - at
            nt_.index, nt_.where = -1, -1
            if t.kind == N.ROW_BITS:
                unique, part = bits[(tuple(t.columns), t.where_text)]
                nt_.pass_bits, nt_.considered_bits = unique.data_ptr(), part.data_ptr()
            else:
                nt_.index = batch.col_index[t.column] if t.kind == N.ROW_NOT_NULL else remap[t.predicate]
                nt_.where = remap[t.where] if t.where >= 0 else -1
            nterms.append(nt_)
        nchecks = []
        for passed, values, validity in outs[at:end]:
            ck = N.DqRowCheck()
            ck.pass_bits, ck.values = passed.data_ptr(), values.data_ptr()
            ck.validity = validity.data_ptr() if validity is not None else None
            nchecks.append(ck)
        tc, cc = ctx.row_outcomes(cols, n, [batch.preds[p].to_native() for p in used], nterms, nchecks,
                                  N.ROW_FILTERED_NULL if null_mode else 0)
        term_counts.extend((t.description, t.constraint, m, k) for t, (m, k) in zip(group, tc))
        check_counts[at:end] = cc
        at = end

    check_cols, res_bits = [], {}
    passed_rows, failed_rows, null_rows = {}, {}, {}
    for desc, (passed, values, validity), (ntrue, nnull) in zip(plan.descriptions, outs, check_counts):
        col = Column(desc, N.TYPE_BOOLEAN, None, None, length=n)
        col.device = {"values": values}
        if validity is not None:
            col.device["validity"] = validity
        check_cols.append(col)
        res_bits[desc] = (passed, validity)
        passed_rows[desc], null_rows[desc], failed_rows[desc] = ntrue, nnull, n - ntrue - nnull
    if on_device:
        table = Table(list(data.columns.values()) + check_cols)
    else:
        table = Table(list(data.columns.values()) + [_to_host(c) for c in check_cols])
    res = RowLevelResults(table, {d: d for d in plan.descriptions}, passed_rows, failed_rows, null_rows, term_counts,
                          skipped)
    res._work, res._bits, res._nrows, res._on_device, res._device = work, res_bits, n, on_device, device
    return res


def row_level_results(result, data, filteredRow="true", strict=False):
    """VerificationResult.rowLevelResultsAsTable (see checks.py)."""
    if filteredRow not in FILTERED_ROW_OUTCOMES:
        raise ValueError("filteredRow must be 'true' or 'null', not %r" % (filteredRow,))
    checks = list(result.checkResults)
    check_names(checks, data)
    null_mode = filteredRow == "null"
    if not isinstance(data, ChunkedTable):
        return _run_table(checks, data, result.metrics, null_mode, strict)
    parts = [_run_table(checks, chunk, result.metrics, null_mode, strict, chunked=True) for chunk in data.chunks]
    first = parts[0]

    def total(attr):
        return {d: sum(getattr(p, attr)[d] for p in parts) for d in first.checkColumns}
    counts = [(d, c, sum(p.termCounts[i][2] for p in parts), sum(p.termCounts[i][3] for p in parts))
              for i, (d, c, _, _) in enumerate(first.termCounts)]
    return RowLevelResults(ChunkedTable([p.table for p in parts]), dict(first.checkColumns), total("passedRows"),
                           total("failedRows"), total("nullRows"), counts, list(first.skipped), parts=parts)
