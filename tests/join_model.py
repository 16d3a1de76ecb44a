"""The model of the cross-table checks in plain Python: what the semi-join probe and the comparison
functions must compute, from the definition alone. Rows are tuples of Python values, None is NULL, integers of any
width are Python ints and so compare by value, strings compare as str (equal text is equal UTF-8)."""
from collections import Counter


def rows_of(data, columns):
    """{column: list} -> the key tuples of `columns`, row by row."""
    n = len(data[columns[0]]) if columns else 0
    return [tuple(data[c][i] for c in columns) for i in range(n)]


def hits(primary_rows, reference_rows):
    """Per primary row: some reference row equals it under SQL '=' in every component. A tuple with a None never
    matches and is never matched."""
    keys = {r for r in reference_rows if None not in r}
    return [None not in p and p in keys for p in primary_rows]


def matched(primary_rows, reference_rows):
    return sum(hits(primary_rows, reference_rows))


def groups_and_rows(rows):
    """(#groups, #rows) under GROUP BY: None is a key value, an all-None key is a group."""
    return len(Counter(rows)), len(rows)


def keys_unique(rows):
    g, n = groups_and_rows(rows)
    return g == n


def bitmap(flags):
    """LSB-first bitmap bytes of a list of bools, padded with zero bits to whole 8-byte words."""
    out = bytearray(((len(flags) + 63) // 64) * 8)
    for i, f in enumerate(flags):
        if f:
            out[i >> 3] |= 1 << (i & 7)
    return bytes(out)
