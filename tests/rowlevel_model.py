"""numpy restatement of the row-level contract: terms -> per-check value / validity arrays and counts.

A term is (check index, `holds`, `considered`), two bool arrays over the rows: `considered` = the rows the term looks
at (its `where` is TRUE; for a uniqueness term also: some key is not NULL), `holds` = what must be true of a
considered row for it to pass. The term builders below take their inputs from the oracle: `O.predicate_masks` for the
TRUE rows of a predicate or filter, `O.compile_java_regex` over `O.spark_cast_to_string` for a pattern, `O.frequencies`
for the group counts. Nothing here calls the product's kernels or its term planner.
"""
import numpy as np

import oracle as O
from deequ_amd.table import Column, Table, pack_validity, unpack_validity


def where_true(table, where):
    return np.ones(table.nrows, dtype=bool) if where is None else O.predicate_masks(table, where)[0].copy()


def term_not_null(check, table, column, where=None):
    c = table[column]
    return check, unpack_validity(c.validity, c.length), where_true(table, where)


def term_predicate(check, table, predicate, where=None):
    return check, O.predicate_masks(table, predicate)[0].copy(), where_true(table, where)


def term_pattern(check, table, column, pattern, where=None):
    """PatternMatch: the first find() match of the cell's string form is non-empty; a NULL cell fails."""
    c = table[column]
    rx = O.compile_java_regex(pattern)
    valid = unpack_validity(c.validity, c.length)
    holds = np.zeros(c.length, dtype=bool)
    for i in np.flatnonzero(valid):
        m = rx.search(O.spark_cast_to_string(c, int(i)))
        holds[i] = m is not None and m.group(0) != ""
    return check, holds, where_true(table, where)


def group_counts(table, columns, where=None):
    """Per row: the count of its group among the rows on which `where` is TRUE (0: the row takes no part -- the filter
    is not TRUE there, or every key is NULL). Groups and counts are O.frequencies' over the kept rows."""
    keep = where_true(table, where)
    cols = []
    for name in columns:
        c = table[name]
        valid = unpack_validity(c.validity, c.length) & keep
        nc = Column(c.name, c.spark_type, c.values, pack_validity(valid), c.offsets, c.decimal_precision, c.decimal_scale,
                    length=c.length)
        cols.append(nc)
    kept = Table(cols)
    freq, _ = O.frequencies(kept, list(columns))
    cells = [O._pylist(kept[c]) for c in columns]
    out = np.zeros(table.nrows, dtype=np.int64)
    for i in range(table.nrows):
        out[i] = freq.get(tuple(O._group_key(c[i]) for c in cells), 0)
    return out


def term_unique(check, table, columns, where=None):
    counts = group_counts(table, columns, where)
    return check, counts == 1, counts > 0


class Outcome:
    """One check: `value` (bool per row; False where the outcome is FALSE or NULL), `validity` (None under
    filteredRow="true"), and the row counts."""

    def __init__(self, value, validity):
        self.value, self.validity = value, validity
        self.true_rows = int(value.sum())
        self.null_rows = 0 if validity is None else int((~validity).sum())
        self.false_rows = len(value) - self.true_rows - self.null_rows


def fold(terms, nchecks, nrows, null_mode):
    """([(matched, considered)] per term, [Outcome] per check). filteredRow="true": a row a term does not consider
    passes it. "null": it is NULL there, and the check follows the three-valued AND -- FALSE if any term is FALSE, else
    NULL if any term is NULL, else TRUE."""
    counts = []
    fail = [np.zeros(nrows, dtype=bool) for _ in range(nchecks)]
    nul = [np.zeros(nrows, dtype=bool) for _ in range(nchecks)]
    for check, holds, considered in terms:
        counts.append((int((holds & considered).sum()), int(considered.sum())))
        fail[check] |= ~holds & considered
        nul[check] |= ~considered
    out = []
    for c in range(nchecks):
        if null_mode:
            out.append(Outcome(~fail[c] & ~nul[c], fail[c] | ~nul[c]))
        else:
            out.append(Outcome(~fail[c], None))
    return counts, out
