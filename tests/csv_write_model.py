"""A plain model of Table.to_csv's file, independent of the package's writers: the cell text is
oracle.spark_cast_to_string, the rest is the quoting rule restated. No GPU, no native code: the host path is compared
with it in test_csv_write.py, the device path in test_gpu_csv_write.py.

  record  = cell ("," cell)* LF          every record, the last included, ends with LF
  cell    = nothing for NULL, else the cast text; a STRING cell's bytes as they are
  quoting = STRING cells (and header names) only: in quotes, every quote doubled, iff the cell holds , " LF CR or is empty
"""
import oracle as O


def quoted(b):
    if b == b"" or b"," in b or b'"' in b or b"\n" in b or b"\r" in b:
        return b'"' + b.replace(b'"', b'""') + b'"'
    return b


def is_null(col, i):
    return col.validity is not None and not (int(col.validity[i >> 3]) >> (i & 7)) & 1


def cell_text(col, i):
    """The unquoted bytes of cell i, None for NULL."""
    if is_null(col, i):
        return None
    if col.spark_type == O.T_STRING:
        return bytes(col.values[int(col.offsets[i]):int(col.offsets[i + 1])])
    return O.spark_cast_to_string(col, i).encode("ascii")


def cell(col, i):
    text = cell_text(col, i)
    if text is None:
        return b""
    return quoted(text) if col.spark_type == O.T_STRING else text


def header(names):
    return b",".join(quoted(n.encode("utf-8")) for n in names) + b"\n"


def body(table):
    cols = list(table.columns.values())
    return b"".join(b",".join(cell(c, i) for c in cols) + b"\n" for i in range(table.nrows))


def file_bytes(table, with_header=True):
    return (header(table.fieldNames) if with_header else b"") + body(table)


def law_cells(table):
    """What from_csv(infer_schema=False) must give back, per column: the cell text, None where the cell was NULL or the
    empty string."""
    out = []
    for c in table.columns.values():
        texts = [cell_text(c, i) for i in range(table.nrows)]
        out.append([None if t is None or t == b"" else t for t in texts])
    return out
