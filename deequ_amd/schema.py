"""Row-level schema validation (schema/RowLevelSchemaValidator.scala:25-282) on the GPU.

`RowLevelSchemaValidator.validate(data, schema)` checks every row of a table of STRING columns against a
`RowLevelSchema` (nullability, length bounds, a regex, cast(int), cast(decimal(p,s)), unix_timestamp(mask)) and splits
it into the cast valid rows and the untouched invalid rows. Spark does this in three passes over a persisted CNF
column; here one kernel launch (dq_schema_validate) reads the bytes once, writes the verdict bitmaps and the cast
values, and dq_gather_rows compacts each column ("Row-level schema validation").
"""
import ctypes

import numpy as np

from . import native as N
from .regex import compile_regex
from .table import NUMPY_OF, ChunkedTable, Column, Table

_INT32_MIN, _INT32_MAX = -(1 << 31), (1 << 31) - 1

# compiled mask (dq_schema_parse.h SchemaMaskOp): {0, byte} literal, {1..6} the fields
MASK_LITERAL = 0
MASK_FIELDS = {"yyyy": 1, "MM": 2, "dd": 3, "HH": 4, "mm": 5, "ss": 6}


def compile_mask(mask):
    """A SimpleDateFormat mask over the fields yyyy MM dd HH mm ss (each at most once, any two separated by at least
    one literal: a non-letter ASCII character or 'quoted text', '' = a quote) -> the byte program the parsers walk.
    Anything else raises ValueError."""
    if not isinstance(mask, str):
        raise ValueError("timestamp mask must be a string")
    prog = bytearray()
    seen = set()
    prev_field = False
    i, n = 0, len(mask)
    while i < n:
        c = mask[i]
        if c == "'":
            if i + 1 < n and mask[i + 1] == "'":  # '' outside a quote: one quote character
                prog += bytes([MASK_LITERAL, ord("'")])
                i += 2
                prev_field = False
                continue
            i += 1
            text = []
            while True:
                if i >= n:
                    raise ValueError("timestamp mask %r: unterminated quote" % mask)
                if mask[i] == "'":
                    if i + 1 < n and mask[i + 1] == "'":
                        text.append("'")
                        i += 2
                        continue
                    i += 1
                    break
                text.append(mask[i])
                i += 1
            for b in "".join(text).encode("utf-8"):
                prog += bytes([MASK_LITERAL, b])
            if text:
                prev_field = False
            continue
        if c.isascii() and c.isalpha():
            j = i
            while j < n and mask[j] == c:
                j += 1
            run = mask[i:j]
            if run not in MASK_FIELDS:
                raise ValueError("timestamp mask %r: unsupported pattern letters %r (supported: yyyy MM dd HH mm ss)"
                                 % (mask, run))
            if run in seen:
                raise ValueError("timestamp mask %r: field %s appears twice" % (mask, run))
            if prev_field:
                raise ValueError("timestamp mask %r: fields must be separated by a literal" % mask)
            seen.add(run)
            prog.append(MASK_FIELDS[run])
            prev_field = True
            i = j
            continue
        if not c.isascii():
            raise ValueError("timestamp mask %r: non-ASCII literal %r must be quoted" % (mask, c))
        prog += bytes([MASK_LITERAL, ord(c)])
        prev_field = False
        i += 1
    return bytes(prog)


class ColumnDefinition:
    kind = None

    def __init__(self, name, isNullable=True):
        self.name = name
        self.isNullable = bool(isNullable)

    def program(self):
        return b""


class StringColumnDefinition(ColumnDefinition):
    kind = N.SCHEMA_STRING

    def __init__(self, name, isNullable=True, minLength=None, maxLength=None, matches=None):
        super().__init__(name, isNullable)
        self.minLength, self.maxLength, self.matches = minLength, maxLength, matches
        self._image = compile_regex(matches).to_bytes() if matches is not None else b""  # RegexUnsupported propagates

    def program(self):
        return self._image


class IntColumnDefinition(ColumnDefinition):
    kind = N.SCHEMA_INT

    def __init__(self, name, isNullable=True, minValue=None, maxValue=None):
        super().__init__(name, isNullable)
        for what, v in (("minValue", minValue), ("maxValue", maxValue)):
            if v is not None and not _INT32_MIN <= int(v) <= _INT32_MAX:
                raise ValueError("column %s: %s %r does not fit an int" % (name, what, v))
        self.minValue, self.maxValue = minValue, maxValue


class DecimalColumnDefinition(ColumnDefinition):
    kind = N.SCHEMA_DECIMAL

    def __init__(self, name, precision, scale, isNullable=True):
        super().__init__(name, isNullable)
        if not 0 <= int(scale) <= int(precision) <= 18:
            raise ValueError("column %s: decimal(%r,%r) needs 0 <= scale <= precision <= 18 (int64 unscaled values)"
                             % (name, precision, scale))
        self.precision, self.scale = int(precision), int(scale)


class TimestampColumnDefinition(ColumnDefinition):
    kind = N.SCHEMA_TIMESTAMP

    def __init__(self, name, mask, isNullable=True):
        super().__init__(name, isNullable)
        self.mask = mask
        self._program = compile_mask(mask)

    def program(self):
        return self._program


class RowLevelSchema:
    """Immutable: every with* call returns a new schema with the definition appended."""

    def __init__(self, columnDefinitions=()):
        self.columnDefinitions = tuple(columnDefinitions)

    def _with(self, d):
        return RowLevelSchema(self.columnDefinitions + (d,))

    def withStringColumn(self, name, isNullable=True, minLength=None, maxLength=None, matches=None):
        return self._with(StringColumnDefinition(name, isNullable, minLength, maxLength, matches))

    def withIntColumn(self, name, isNullable=True, minValue=None, maxValue=None):
        return self._with(IntColumnDefinition(name, isNullable, minValue, maxValue))

    def withDecimalColumn(self, name, precision, scale, isNullable=True):
        return self._with(DecimalColumnDefinition(name, precision, scale, isNullable))

    def withTimestampColumn(self, name, mask, isNullable=True):
        return self._with(TimestampColumnDefinition(name, mask, isNullable))


class RowLevelSchemaValidationResult:
    def __init__(self, validRows, numValidRows, invalidRows, numInvalidRows, numUnknownRows=0, numAmbiguousRows=0):
        self.validRows, self.numValidRows = validRows, numValidRows
        self.invalidRows, self.numInvalidRows = invalidRows, numInvalidRows
        self.numUnknownRows = numUnknownRows      # verdict NULL: in neither output (reference :246)
        self.numAmbiguousRows = numAmbiguousRows  # ambiguous="invalid": rows with a cell cast to NULL by that policy


def check_schema(data, schema):
    """Every schema column exists and is STRING: ValueError before any GPU work."""
    for d in schema.columnDefinitions:
        if d.name not in data:
            raise ValueError("schema column %r is not in the table" % d.name)
        if data[d.name].spark_type != N.TYPE_STRING:
            raise ValueError("schema column %r is %s: the validator takes STRING columns" % (d.name, data[d.name].type_name))


def _device_view(table, device):
    """The table in HBM: itself when every column is resident, else a device copy of its host buffers."""
    if all(c.device is not None for c in table.columns.values()):
        return table, True
    cols = []
    for c in table.columns.values():
        nc = Column(c.name, c.spark_type, c.values, c.validity, c.offsets, c.decimal_precision, c.decimal_scale,
                    length=c.length)
        nc.tz = c.tz
        cols.append(nc)
    return Table(cols).to_device(device), False


def _to_host(col):
    """A device-only column as a host column."""
    d = col.device
    n = col.length
    validity = d["validity"].cpu().numpy() if d.get("validity") is not None else None
    if col.spark_type == N.TYPE_STRING:
        offsets = d["offsets"].cpu().numpy().astype(np.int32)
        values = d["values"][:int(offsets[n]) if n else 0].cpu().numpy()
        out = Column(col.name, col.spark_type, values, validity, offsets, length=n)
    else:
        dt = np.dtype(NUMPY_OF[col.spark_type])
        values = d["values"].cpu().numpy().view(np.uint8)[:n * dt.itemsize].view(dt).copy()
        out = Column(col.name, col.spark_type, values, validity, decimal_precision=col.decimal_precision,
                     decimal_scale=col.decimal_scale, length=n)
    out.tz = col.tz
    return out


def _gather(ctx, torch, dev, col, nrows, select, nsel):
    """dq_gather_rows of one device column into torch-allocated buffers."""
    out = Column(col.name, col.spark_type, None, None, decimal_precision=col.decimal_precision,
                 decimal_scale=col.decimal_scale, length=nsel)
    out.tz = col.tz
    native = col.native()
    has_validity = col.device.get("validity") is not None
    validity = torch.zeros(max((nsel + 63) // 64, 1) * 8, dtype=torch.uint8, device=dev) if has_validity else None
    vptr = validity.data_ptr() if has_validity else None
    if col.spark_type == N.TYPE_STRING:
        offsets = torch.zeros(nsel + 1, dtype=torch.int32, device=dev)
        nbytes = ctx.gather_rows(native, nrows, select.data_ptr(), nsel, None, vptr, offsets.data_ptr())
        values = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
        ctx.gather_rows(native, nrows, select.data_ptr(), nsel, values.data_ptr(), None, offsets.data_ptr())
        out.device = {"values": values, "offsets": offsets}
    else:
        width = np.dtype(NUMPY_OF[col.spark_type]).itemsize
        values = torch.zeros(max(nsel, 1) * width, dtype=torch.uint8, device=dev)
        ctx.gather_rows(native, nrows, select.data_ptr(), nsel, values.data_ptr(), vptr)
        out.device = {"values": values}
    if has_validity:
        out.device["validity"] = validity
    return out


class RowLevelSchemaValidator:
    @staticmethod
    def validate(data, schema, ambiguous="error"):
        """RowLevelSchemaValidator.validate (:183-206). `ambiguous`: "error" raises NativeError (DQ_ERR_UNSUPPORTED)
        when a decimal / timestamp cell's JVM parse is not reproduced here (the three classes); "invalid"
        casts such cells to NULL and reports the rows as numAmbiguousRows."""
        if ambiguous not in ("error", "invalid"):
            raise ValueError("ambiguous must be 'error' or 'invalid'")
        check_schema(data, schema)
        if isinstance(data, ChunkedTable):
            parts = [RowLevelSchemaValidator._validate_table(t, schema, ambiguous) for t in data.chunks]
            return RowLevelSchemaValidationResult(
                ChunkedTable([p.validRows for p in parts]), sum(p.numValidRows for p in parts),
                ChunkedTable([p.invalidRows for p in parts]), sum(p.numInvalidRows for p in parts),
                sum(p.numUnknownRows for p in parts), sum(p.numAmbiguousRows for p in parts))
        return RowLevelSchemaValidator._validate_table(data, schema, ambiguous)

    @staticmethod
    def _validate_table(data, schema, ambiguous):
        import torch
        from . import engine
        ctx = engine.ctx()
        if ctx.multi:
            raise N.NativeError(-2, "RowLevelSchemaValidator: multi-device contexts are not supported")
        dev = torch.device("cuda", engine.device())
        work, on_device = _device_view(data, engine.device())
        n = data.nrows
        names = list(work.columns)
        nbitmap = max((n + 63) // 64, 1) * 8
        true_bits, false_bits, amb_bits = (torch.zeros(nbitmap, dtype=torch.uint8, device=dev) for _ in range(3))
        defs, casts, keep = [], {}, []
        for d in schema.columnDefinitions:
            sc = N.DqSchemaColumn()
            sc.kind = d.kind
            sc.column = names.index(d.name)
            sc.nullable = 1 if d.isNullable else 0
            prog = d.program()
            if prog:
                buf = ctypes.create_string_buffer(prog, len(prog))
                keep.append(buf)
                sc.program = ctypes.addressof(buf)
                sc.program_len = len(prog)
            if d.kind == N.SCHEMA_STRING:
                lo, hi = d.minLength, d.maxLength
            elif d.kind == N.SCHEMA_INT:
                lo, hi = d.minValue, d.maxValue
            else:
                lo = hi = None
            if lo is not None:
                sc.has_min, sc.min_value = 1, int(lo)
            if hi is not None:
                sc.has_max, sc.max_value = 1, int(hi)
            if d.kind != N.SCHEMA_STRING:
                if d.kind == N.SCHEMA_INT:
                    t, dtype = N.TYPE_INT, torch.int32
                elif d.kind == N.SCHEMA_DECIMAL:
                    t, dtype = N.TYPE_DECIMAL, torch.int64
                    sc.precision, sc.scale = d.precision, d.scale
                else:
                    t, dtype = N.TYPE_TIMESTAMP, torch.int64
                vals = torch.zeros(max(n, 1), dtype=dtype, device=dev)
                mask = torch.zeros(nbitmap, dtype=torch.uint8, device=dev)
                sc.cast_values, sc.cast_validity = vals.data_ptr(), mask.data_ptr()
                cast = Column(d.name, t, None, None, length=n,
                              decimal_precision=d.precision if d.kind == N.SCHEMA_DECIMAL else 0,
                              decimal_scale=d.scale if d.kind == N.SCHEMA_DECIMAL else 0)
                cast.device = {"values": vals, "validity": mask}
                casts[d.name] = cast  # a column defined twice keeps its last definition's cast (a Map in the reference)
            defs.append(sc)
        flags = N.SCHEMA_AMBIGUOUS_NULL if ambiguous == "invalid" else 0
        rc, res = ctx.schema_validate([work[c].native() for c in names], n, defs, flags, true_bits.data_ptr(),
                                      false_bits.data_ptr(), amb_bits.data_ptr())
        if rc != N.DQ_OK:
            if rc == -2 and res.num_ambiguous:
                raise N.NativeError(rc, "RowLevelSchemaValidator: %d rows hold a cell whose JVM parse is ambiguous, "
                                        "first in column %r; ambiguous='invalid' casts such cells to NULL"
                                    % (res.num_ambiguous, names[res.first_ambiguous_column]))
            ctx.check(rc, "dq_schema_validate")
        nv, ni = int(res.num_valid), int(res.num_invalid)
        valid = [_gather(ctx, torch, dev, casts.get(c, work[c]), n, true_bits, nv) for c in names]
        invalid = [_gather(ctx, torch, dev, work[c], n, false_bits, ni) for c in names]
        if not on_device:
            valid = [_to_host(c) for c in valid]
            invalid = [_to_host(c) for c in invalid]
        return RowLevelSchemaValidationResult(Table(valid), nv, Table(invalid), ni, int(res.num_unknown),
                                              int(res.num_ambiguous))
