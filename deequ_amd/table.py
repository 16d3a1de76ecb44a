"""Columnar batches in the layout the C-ABI takes (Arrow-style buffers + the Spark physical type).

This stands where deequ takes a Spark DataFrame (`AnalysisRunner.onData(df)`,
R/AnalysisRunner.scala:51-53). A Table holds named columns; each column is a values buffer,
an LSB-first validity bitmap (None = no nulls) and, for strings, int32 offsets into UTF-8 data.
`Table.to_device()` moves the buffers into HBM (torch is used only as the device allocator) so
repeated runs read device-resident data, as the benchmark does.
"""
import csv
import math
import os
import re
from collections import OrderedDict

import numpy as np

from . import native as N

SPARK_TYPE_NAMES = {
    N.TYPE_BOOLEAN: "BooleanType", N.TYPE_BYTE: "ByteType", N.TYPE_SHORT: "ShortType",
    N.TYPE_INT: "IntegerType", N.TYPE_LONG: "LongType", N.TYPE_FLOAT: "FloatType",
    N.TYPE_DOUBLE: "DoubleType", N.TYPE_STRING: "StringType", N.TYPE_DATE: "DateType",
    N.TYPE_TIMESTAMP: "TimestampType", N.TYPE_DECIMAL: "DecimalType",
}
WIDE_DECIMAL_NAME = "DecimalType"  # TYPE_DECIMAL128 shares Spark's type name: the precision tells them apart
# One DECIMAL128 cell: the 16-byte little-endian two's-complement unscaled value, Arrow's decimal128 cell.
DEC128_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<i8")])
_NAME_TO_TYPE = {v.lower().replace("type", ""): k for k, v in SPARK_TYPE_NAMES.items()}
_NAME_TO_TYPE.update({"int": N.TYPE_INT, "bigint": N.TYPE_LONG, "bool": N.TYPE_BOOLEAN, "str": N.TYPE_STRING,
                      "float64": N.TYPE_DOUBLE, "float32": N.TYPE_FLOAT, "int64": N.TYPE_LONG,
                      "int32": N.TYPE_INT, "int16": N.TYPE_SHORT, "int8": N.TYPE_BYTE})

NUMPY_OF = {N.TYPE_BOOLEAN: np.uint8, N.TYPE_BYTE: np.int8, N.TYPE_SHORT: np.int16, N.TYPE_INT: np.int32,
            N.TYPE_LONG: np.int64, N.TYPE_FLOAT: np.float32, N.TYPE_DOUBLE: np.float64, N.TYPE_DATE: np.int32,
            N.TYPE_TIMESTAMP: np.int64, N.TYPE_DECIMAL: np.int64, N.TYPE_DECIMAL128: DEC128_DTYPE}

NUMERIC_TYPES = (N.TYPE_BYTE, N.TYPE_SHORT, N.TYPE_INT, N.TYPE_LONG, N.TYPE_FLOAT, N.TYPE_DOUBLE, N.TYPE_DECIMAL,
                 N.TYPE_DECIMAL128)
_DECIMAL_PS = re.compile(r"^\s*decimal(?:type)?\s*\(\s*(\d+)\s*,\s*(\d+)\s*\)\s*$", re.I)


def decimal_precision_scale(name):
    """(precision, scale) of a type string with explicit "(p,s)", e.g. "decimal(38,18)"; None otherwise."""
    m = _DECIMAL_PS.match(name) if isinstance(name, str) else None
    return (int(m.group(1)), int(m.group(2))) if m else None


def dec128_cells(unscaled):
    """Python ints -> DEC128_DTYPE cells (two's complement); a value outside 128 bits raises OverflowError."""
    out = np.zeros(len(unscaled), dtype=DEC128_DTYPE)
    if len(unscaled):
        out[:] = np.frombuffer(b"".join(int(v).to_bytes(16, "little", signed=True) for v in unscaled), dtype=DEC128_DTYPE)
    return out


def dec128_int(cell):
    """One DEC128_DTYPE cell -> its unscaled Python int."""
    return (int(cell["hi"]) << 64) | int(cell["lo"])


def spark_type_of(name_or_code):
    if isinstance(name_or_code, int):
        return name_or_code
    key = str(name_or_code).lower().replace("type", "")
    key = re.sub(r"\(.*\)", "", key)
    if key not in _NAME_TO_TYPE:
        raise ValueError("unknown Spark type %r" % name_or_code)
    return _NAME_TO_TYPE[key]


def pack_validity(mask):
    """bool mask (True = non-null) -> Arrow LSB-first bitmap (uint8), padded to 8-byte multiples."""
    mask = np.asarray(mask, dtype=bool)
    bits = np.packbits(mask, bitorder="little")
    pad = (-len(bits)) % 8
    if pad:
        bits = np.concatenate([bits, np.zeros(pad, dtype=np.uint8)])
    return bits


def unpack_validity(bitmap, n):
    if bitmap is None:
        return np.ones(n, dtype=bool)
    return np.unpackbits(np.asarray(bitmap, dtype=np.uint8), bitorder="little", count=n).astype(bool)


class Column:
    """One column: Spark type, values, optional validity bitmap, optional string offsets."""

    def __init__(self, name, spark_type, values, validity=None, offsets=None, decimal_precision=0,
                 decimal_scale=0, length=None):
        self.name = name
        self.spark_type = spark_type_of(spark_type)
        self.values = values
        self.validity = validity
        self.offsets = offsets
        self.decimal_precision = decimal_precision
        self.decimal_scale = decimal_scale
        if length is None:
            length = len(offsets) - 1 if self.spark_type == N.TYPE_STRING else len(values)
        self.length = int(length)
        self.device = None  # dict of torch tensors once resident in HBM
        self.tz = None  # TIMESTAMP: the Arrow column's time zone (None = naive, read as the UTC session zone)

    @property
    def type_name(self):
        if self.spark_type == N.TYPE_DECIMAL128:
            return "%s(%d,%d)" % (WIDE_DECIMAL_NAME, self.decimal_precision, self.decimal_scale)
        n = SPARK_TYPE_NAMES[self.spark_type]
        if self.spark_type == N.TYPE_DECIMAL:
            return "DecimalType(%d,%d)" % (self.decimal_precision, self.decimal_scale)
        return n

    def is_numeric(self):
        return self.spark_type in NUMERIC_TYPES

    def is_wide_decimal(self):
        return self.spark_type == N.TYPE_DECIMAL128

    def null_mask(self):
        return ~unpack_validity(self.validity, self.length)

    def to_pylist(self):
        """Python values with None for nulls (host-side formatting only, e.g. Histogram keys)."""
        valid = unpack_validity(self.validity, self.length)
        out = []
        for i in range(self.length):
            out.append(self.value_at(i) if valid[i] else None)
        return out

    def valid_at(self, i):
        """Row i is non-NULL (reads one validity byte from HBM for a device-only column)."""
        if self.validity is not None:
            return bool((self.validity[i >> 3] >> (i & 7)) & 1)
        if self.values is None and self.device is not None and self.device.get("validity") is not None:
            return bool((int(self.device["validity"][i >> 3].item()) >> (i & 7)) & 1)
        return True

    def value_at(self, i):
        if self.values is None and self.device is not None:
            return self._device_value_at(i)
        if self.spark_type == N.TYPE_STRING:
            o = self.offsets
            return bytes(self.values[o[i]:o[i + 1]]).decode("utf-8")
        return self._decode_cell(self.values[i])

    def _device_value_at(self, i):
        """One cell of a device-only column (top-N keys, representatives of a few groups: tiny copies)."""
        d = self.device
        if self.spark_type == N.TYPE_STRING:
            o = d["offsets"][i:i + 2].cpu().numpy()
            return bytes(d["values"][int(o[0]):int(o[1])].cpu().numpy()).decode("utf-8")
        t = d["values"]
        dt = np.dtype(NUMPY_OF[self.spark_type])
        if str(t.dtype) == "torch.uint8" and dt.itemsize > 1:
            v = t.reshape(-1)[i * dt.itemsize:(i + 1) * dt.itemsize].cpu().numpy().view(dt)[0]
        else:
            v = t[i:i + 1].cpu().numpy().astype(dt)[0]
        return self._decode_cell(v)

    def cells_at(self, rows):
        """The cells of `rows` (None for NULL) in one go: for a device-only column, one gather per buffer and one copy
        back each (the representatives of a table's groups), instead of a device round trip per row."""
        rows = np.asarray(rows, dtype=np.int64)
        if len(rows) == 0:
            return []
        if not (self.values is None and self.device is not None):
            return [self.value_at(int(r)) if self.valid_at(int(r)) else None for r in rows]
        import torch
        d = self.device
        dev = d["values"].device
        idx = torch.from_numpy(rows).to(dev)
        if d.get("validity") is not None:
            vb = d["validity"][idx >> 3].cpu().numpy()
            valid = ((vb >> (rows & 7).astype(np.uint8)) & 1).astype(bool)
        else:
            valid = np.ones(len(rows), dtype=bool)
        if self.spark_type == N.TYPE_STRING:
            off = d["offsets"]
            lo = off[idx].to(torch.int64)
            hi = off[idx + 1].to(torch.int64)
            lens = (hi - lo).cpu().numpy()
            total = int(lens.sum())
            if total:
                starts = np.repeat(lo.cpu().numpy() - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
                pos = torch.from_numpy(starts + np.arange(total, dtype=np.int64)).to(dev)
                data = d["values"][pos].cpu().numpy().tobytes()
            else:
                data = b""
            out, at = [], 0
            for ok, n in zip(valid, lens):
                out.append(data[at:at + int(n)].decode("utf-8") if ok else None)
                at += int(n)
            return out
        t = d["values"]
        dt = np.dtype(NUMPY_OF[self.spark_type])
        if str(t.dtype) == "torch.uint8" and dt.itemsize > 1:
            pos = (idx[:, None] * dt.itemsize + torch.arange(dt.itemsize, device=dev)[None, :]).reshape(-1)
            vals = t.reshape(-1)[pos].cpu().numpy().view(dt)
        else:
            vals = t[idx].cpu().numpy().astype(dt)
        return [self._decode_cell(v) if ok else None for v, ok in zip(vals, valid)]

    def _decode_cell(self, v):
        if self.spark_type == N.TYPE_BOOLEAN:
            return bool(v)
        if self.spark_type in (N.TYPE_FLOAT, N.TYPE_DOUBLE):
            return float(v)
        if self.spark_type == N.TYPE_DECIMAL:
            return int(v) / (10 ** self.decimal_scale)
        if self.spark_type == N.TYPE_DECIMAL128:
            from decimal import Context, Decimal
            return Decimal(dec128_int(v)).scaleb(-self.decimal_scale, context=Context(prec=60))  # exact: <= 39 digits
        return int(v)

    def native(self):
        """DqColumn for the C-ABI (device pointers when resident in HBM)."""
        c = N.DqColumn()
        c.spark_type = self.spark_type
        c.length = self.length
        c.decimal_precision = self.decimal_precision
        c.decimal_scale = self.decimal_scale
        if self.device is not None:
            c.flags = N.COL_DEVICE | (N.COL_OFFSETS64 if getattr(self, "offsets64", False) else 0)
            c.values = self.device["values"].data_ptr() if self.device.get("values") is not None else None
            c.validity = self.device["validity"].data_ptr() if self.device.get("validity") is not None else None
            c.offsets = self.device["offsets"].data_ptr() if self.device.get("offsets") is not None else None
        else:
            c.flags = N.COL_OFFSETS64 if getattr(self, "offsets64", False) else 0
            c.values = self.values.ctypes.data if self.values is not None and len(self.values) else None
            c.validity = self.validity.ctypes.data if self.validity is not None else None
            c.offsets = self.offsets.ctypes.data if self.offsets is not None else None
        return c

    def native_parts(self):
        """The column as consecutive row ranges for the ABIs that take parts (dq_quantile_summaries)."""
        return [self.native()]


class PartedColumn(Column):
    """A column of a ChunkedTable seen as its chunks' columns in row order, read where they lie (no concatenation):
    only the ABIs that take parts accept it (dq_quantile_summaries)."""

    def __init__(self, parts):
        first = parts[0]
        super().__init__(first.name, first.spark_type, None, None, decimal_precision=first.decimal_precision,
                         decimal_scale=first.decimal_scale, length=sum(p.length for p in parts))
        self.parts = list(parts)
        self.tz = first.tz

    def native(self):
        raise TypeError("column %s is held as %d chunks: only a per-part ABI reads it" % (self.name, len(self.parts)))

    def native_parts(self):
        return [p.native() for p in self.parts]

    def _locate(self, i):
        """(part, row inside it) of row i of the concatenation."""
        for p in self.parts:
            if i < p.length:
                return p, i
            i -= p.length
        raise IndexError(i)

    def valid_at(self, i):
        p, j = self._locate(int(i))
        return p.valid_at(j)

    def value_at(self, i):
        p, j = self._locate(int(i))
        return p.value_at(j)

    def cells_at(self, rows):
        """The cells of `rows` (indices into the concatenation): one batched gather per part."""
        rows = np.asarray(rows, dtype=np.int64)
        out = [None] * len(rows)
        base = 0
        for p in self.parts:
            sel = np.flatnonzero((rows >= base) & (rows < base + p.length))
            if len(sel):
                for k, v in zip(sel.tolist(), p.cells_at(rows[sel] - base)):
                    out[k] = v
            base += p.length
        return out


class _DecodedBuffers:
    """The device buffers of a DictColumn as a plain STRING column's `device` dict: present (so `col.device is not
    None` costs nothing) but decoded, on the device, only when a buffer is asked for."""

    def __init__(self, col):
        self._col = col

    def _d(self):
        return self._col.decoded().device

    def __getitem__(self, key):
        return self._d()[key]

    def get(self, key, default=None):
        return self._d().get(key, default)

    def __contains__(self, key):
        return key in self._d()

    def keys(self):
        return self._d().keys()

    def items(self):
        return self._d().items()


class DictColumn(Column):
    """A STRING column held dictionary-encoded (Arrow `dictionary<values=string, indices=int32>`): int32 `indices`
    into `dictionary`, a plain STRING Column of n_dict entries that may hold duplicates, unused entries, the empty
    string and NULL entries. A row is NULL iff its validity bit is clear: the rows that point at a NULL entry are
    folded into the bitmap at ingest, and the index of a NULL row is 0. The indices and the dictionary always have
    host buffers (the dictionary is small); `to_device` adds the HBM copies the native paths read (dq_dict_scan,
    dq_dict_counts). Every consumer that does not know the class sees a plain STRING column: `values`, `offsets`,
    `device` and `native()` are those of `decoded()`, built on first use (on the device for a device column)."""

    def __init__(self, name, indices, validity, dictionary, length=None):
        self.name = name
        self.spark_type = N.TYPE_STRING
        # None (with `length`): a column ingested on the device (from_arrow(device=...)), whose indices and validity
        # live in dict_device only; its cells are read through decoded()
        self.indices = None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
        self.validity = validity
        self.dictionary = dictionary
        self.decimal_precision = 0
        self.decimal_scale = 0
        self.length = len(self.indices) if indices is not None else int(length)
        self.dict_device = None  # torch tensors once resident: indices, validity, dict_values, dict_offsets, dict_validity
        self.tz = None
        self._decoded = None

    @property
    def n_dict(self):
        return self.dictionary.length

    # ---- the plain-column view -------------------------------------------------------------------
    @property
    def values(self):
        return None if self.dict_device is not None else self.decoded().values  # a device column decodes in HBM only

    @property
    def offsets(self):
        return None if self.dict_device is not None else self.decoded().offsets

    @property
    def device(self):
        return _DecodedBuffers(self) if self.dict_device is not None else None

    def native(self):
        return self.decoded().native()

    def decoded(self):
        """The column as a plain STRING Column (cached): host buffers for a host column; for a device column a
        device-only column gathered in HBM (dq_dict_decode), sharing this column's validity bitmap."""
        if self._decoded is None:
            self._decoded = self._decode_device() if self.dict_device is not None else self._decode_host()
        return self._decoded

    def _decode_host(self):
        d = self.dictionary
        doff = np.asarray(d.offsets, dtype=np.int64)
        if self.length == 0 or d.length == 0:
            return Column(self.name, N.TYPE_STRING, np.zeros(0, np.uint8), self.validity,
                          np.zeros(self.length + 1, np.int32), length=self.length)
        idx = self.indices.astype(np.int64)
        lens = doff[idx + 1] - doff[idx]
        lens[~unpack_validity(self.validity, self.length)] = 0
        offs = np.zeros(self.length + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        if offs[-1] >= 2 ** 31:
            raise ValueError("column %s: the decoded strings hold %d bytes, past the int32 offsets of one column (2^31)"
                             % (self.name, int(offs[-1])))
        src = np.repeat(doff[idx] - offs[:-1], lens) + np.arange(int(offs[-1]), dtype=np.int64)
        data = np.asarray(d.values, dtype=np.uint8)[src]
        return Column(self.name, N.TYPE_STRING, data, self.validity, offs.astype(np.int32), length=self.length)

    def _decode_device(self):
        import torch
        from . import engine
        dd = self.dict_device
        dev = dd["indices"].device
        offsets = torch.empty(self.length + 1, dtype=torch.int32, device=dev)
        ctx = engine.ctx()
        total = ctx.dict_decode(self.native_dict(), offsets.data_ptr(), None)
        values = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        ctx.dict_decode(self.native_dict(), offsets.data_ptr(), values.data_ptr())
        col = Column(self.name, N.TYPE_STRING, None, None, length=self.length)
        col.device = {"values": values, "offsets": offsets}
        if dd.get("validity") is not None:
            col.device["validity"] = dd["validity"]
        return col

    # ---- cells -------------------------------------------------------------------------------------
    def valid_at(self, i):
        if self.indices is None:
            return self.decoded().valid_at(i)
        return True if self.validity is None else bool((self.validity[i >> 3] >> (i & 7)) & 1)

    def value_at(self, i):
        if self.indices is None:
            return self.decoded().value_at(i)
        return self.dictionary.value_at(int(self.indices[i]))

    def cells_at(self, rows):
        if self.indices is None:
            return self.decoded().cells_at(rows)
        return [self.value_at(int(r)) if self.valid_at(int(r)) else None for r in np.asarray(rows, dtype=np.int64)]

    def to_pylist(self):
        if self.indices is None:
            return self.decoded().cells_at(np.arange(self.length))
        entries = self.dictionary.to_pylist()
        valid = unpack_validity(self.validity, self.length)
        return [entries[i] if v else None for i, v in zip(self.indices.tolist(), valid.tolist())]

    def to_arrow(self):
        import pyarrow as pa
        return column_to_arrow(self, pa)

    # ---- device ------------------------------------------------------------------------------------
    def to_device(self, device=0):
        """Copy the indices, the validity bitmap and the dictionary into HBM. The device dictionary holds one entry
        more than `dictionary`: entry n_dict is NULL and stands for the NULL rows when a predicate is evaluated once
        per entry (dq_dict_scan)."""
        import torch
        dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
        if self.indices is None:
            raise TypeError("column %s was ingested on the device and has no host buffers to copy" % self.name)
        dd = {"indices": torch.from_numpy(self.indices).to(dev)}
        if self.validity is not None:
            dd["validity"] = torch.from_numpy(pack_validity(unpack_validity(self.validity, self.length))).to(dev)
        dd.update(_dictionary_device(self.dictionary, dev, torch))
        self.dict_device = dd
        self._decoded = None
        return self

    def native_dict(self):
        """DqDictColumn over the device buffers (the C-ABI's dq_dict_column)."""
        dd = self.dict_device
        if dd is None:
            raise TypeError("column %s: the dictionary paths read device-resident columns (to_device())" % self.name)
        c = N.DqDictColumn()
        c.flags = N.COL_DEVICE
        c.length = self.length
        c.indices = dd["indices"].data_ptr()
        c.validity = dd["validity"].data_ptr() if dd.get("validity") is not None else None
        c.dictionary.spark_type = N.TYPE_STRING
        c.dictionary.flags = N.COL_DEVICE
        c.dictionary.length = self.n_dict + 1
        c.dictionary.values = dd["dict_values"].data_ptr()
        c.dictionary.offsets = dd["dict_offsets"].data_ptr()
        c.dictionary.validity = dd["dict_validity"].data_ptr()
        return c

    def indices_native(self):
        """The indices as an INT column: how the fused scan is handed a kept column that none of its ops reads."""
        c = N.DqColumn()
        c.spark_type = N.TYPE_INT
        c.flags = N.COL_DEVICE
        c.length = self.length
        c.values = self.dict_device["indices"].data_ptr()
        c.validity = self.dict_device["validity"].data_ptr() if self.dict_device.get("validity") is not None else None
        return c


def _dictionary_device(d, dev, torch):
    """The entries of a dictionary (a host STRING column) as the device buffers of DictColumn.dict_device, with the
    extra NULL entry n_dict."""
    nd = d.length
    offs = np.asarray(d.offsets, dtype=np.int32)[:nd + 1] if nd else np.zeros(1, np.int32)
    nbytes = int(offs[-1])
    dd = {"dict_values": torch.from_numpy(
        np.concatenate([np.asarray(d.values, dtype=np.uint8)[:nbytes], np.zeros(16, np.uint8)])).to(dev)}
    dd["dict_offsets"] = torch.from_numpy(np.concatenate([offs, offs[-1:]]).astype(np.int32)).to(dev)
    dvalid = np.concatenate([unpack_validity(d.validity, nd), np.zeros(1, dtype=bool)])
    dd["dict_validity"] = torch.from_numpy(pack_validity(dvalid)).to(dev)
    return dd


def _dict_column_from_arrow(name, arr, pa):
    """dictionary<values=string|large_string, indices=intN|uintN> -> DictColumn: the indices widened to int32 (a
    cast, never a decode), NULL entries folded into the validity bitmap, an index outside the dictionary on a valid
    row rejected."""
    n = len(arr)
    entries = arr.dictionary
    if pa.types.is_large_string(entries.type):
        entries = entries.cast(pa.string())
    dictionary = _column_from_arrow(name, entries, pa)
    nd = dictionary.length
    ind = arr.indices
    valid = ~np.asarray(ind.is_null()) if ind.null_count else np.ones(n, dtype=bool)
    idx = np.asarray(ind.fill_null(0) if ind.null_count else ind).astype(np.int64)
    bad = valid & ((idx < 0) | (idx >= nd))
    if bad.any():
        r = int(np.flatnonzero(bad)[0])
        raise ValueError("column %s: row %d has dictionary index %d outside [0, %d)" % (name, r, int(idx[r]), nd))
    idx[~valid] = 0
    if dictionary.validity is not None and n:
        valid &= unpack_validity(dictionary.validity, nd)[idx] if nd else False
        idx[~valid] = 0
    return DictColumn(name, idx.astype(np.int32), None if valid.all() else pack_validity(valid), dictionary)


def _wide_column_from_pylist(name, precision, scale, items):
    """decimal.Decimal / int / str cells -> a DECIMAL128 column of decimal(precision, scale); a cell that does not fit
    (more fraction digits than the scale, or more than `precision` digits) raises ValueError."""
    import decimal
    if not (19 <= precision <= 38 and 0 <= scale <= precision):
        raise ValueError("column %s: decimal(%d,%d) is not a wide decimal (19 <= p <= 38, 0 <= s <= p)"
                         % (name, precision, scale))
    unscaled, mask = [], []
    with decimal.localcontext() as c:
        c.prec = 100
        for x in items:
            mask.append(x is not None)
            if x is None:
                unscaled.append(0)
                continue
            if isinstance(x, float):
                raise ValueError("column %s: a float cell (%r) is not an exact decimal; pass Decimal, int or str"
                                 % (name, x))
            try:
                d = decimal.Decimal(x)
            except decimal.InvalidOperation:
                raise ValueError("column %s: %r is not a decimal" % (name, x))
            u = d.scaleb(scale)
            if not d.is_finite() or u != u.to_integral_value() or abs(int(u)) >= 10 ** precision:
                raise ValueError("column %s: %r does not fit decimal(%d,%d)" % (name, x, precision, scale))
            unscaled.append(int(u))
    mask = np.array(mask, dtype=bool)
    return Column(name, N.TYPE_DECIMAL128, dec128_cells(unscaled), None if mask.all() else pack_validity(mask),
                  decimal_precision=precision, decimal_scale=scale)


def _column_from_pylist(name, spark_type, items):
    ps = decimal_precision_scale(spark_type)
    if ps is not None and ps[0] > 18:
        return _wide_column_from_pylist(name, ps[0], ps[1], items)
    t = spark_type_of(spark_type)
    n = len(items)
    mask = np.array([x is not None and not (isinstance(x, float) and math.isnan(x) and t == N.TYPE_STRING)
                     for x in items], dtype=bool)
    validity = None if mask.all() else pack_validity(mask)
    if t == N.TYPE_STRING:
        enc = [("" if x is None else str(x)).encode("utf-8") for x in items]
        offsets = np.zeros(n + 1, dtype=np.int32)
        if n:
            offsets[1:] = np.cumsum([len(b) for b in enc])
        data = np.frombuffer(b"".join(enc), dtype=np.uint8).copy() if n else np.zeros(0, dtype=np.uint8)
        return Column(name, t, data, validity, offsets, length=n)
    if t == N.TYPE_DECIMAL:
        from decimal import Decimal
        vals = [Decimal(str(x)) if x is not None else Decimal(0) for x in items]
        scale = max([max(0, -v.as_tuple().exponent) for v in vals] + [0])
        unscaled = np.array([int(v.scaleb(scale)) for v in vals], dtype=np.int64)
        prec = max([len(str(abs(int(u)))) for u in unscaled] + [1])
        return Column(name, t, unscaled, validity, decimal_precision=max(prec, scale + 1), decimal_scale=scale)
    dtype = NUMPY_OF[t]
    fill = 0
    vals = np.array([fill if x is None else x for x in items], dtype=dtype)
    return Column(name, t, vals, validity)


def _arrow_validity(arr, n):
    if arr.null_count == 0:
        return None
    bits = np.frombuffer(arr.buffers()[0], dtype=np.uint8)
    mask = np.unpackbits(bits, bitorder="little", count=arr.offset + n)[arr.offset:].astype(bool)
    return pack_validity(mask)


def _kept_dictionary(t, pa):
    """The Arrow type is one that `dictionaries="keep"` holds encoded: a dictionary of strings."""
    return pa.types.is_dictionary(t) and (pa.types.is_string(t.value_type) or pa.types.is_large_string(t.value_type))


def _string_column_from_arrow(name, arr, validity):
    """A pa.string() array -> a host STRING column over its buffers."""
    n = len(arr)
    bufs = arr.buffers()
    offs = np.frombuffer(bufs[1], dtype=np.int32)[arr.offset:arr.offset + n + 1]
    data = np.frombuffer(bufs[2], dtype=np.uint8) if bufs[2] is not None else np.zeros(0, np.uint8)
    base = int(offs[0]) if n else 0
    end = int(offs[-1]) if n else 0
    return Column(name, N.TYPE_STRING, data[base:end], validity, (offs - base).astype(np.int32), length=n)


def _column_from_arrow(name, arr, pa, wide_decimals=False, dictionaries="decode"):
    t, n = arr.type, len(arr)
    if dictionaries == "keep" and _kept_dictionary(t, pa):
        return _dict_column_from_arrow(name, arr, pa)
    validity = _arrow_validity(arr, n)
    if pa.types.is_dictionary(t):
        return _column_from_arrow(name, arr.dictionary_decode(), pa, wide_decimals)
    if pa.types.is_large_string(t):
        arr, t = arr.cast(pa.string()), pa.string()
    if pa.types.is_string(t):
        return _string_column_from_arrow(name, arr, validity)
    if pa.types.is_boolean(t):
        bits = np.frombuffer(arr.buffers()[1], dtype=np.uint8)
        vals = np.unpackbits(bits, bitorder="little", count=arr.offset + n)[arr.offset:].astype(np.uint8)
        return Column(name, N.TYPE_BOOLEAN, vals, validity)
    if pa.types.is_decimal(t):
        if t.precision > 18 and wide_decimals and pa.types.is_decimal128(t):
            # the Arrow cells are the DECIMAL128 layout: taken as they are (NULL slots zeroed, as the int64 path does)
            cells = np.frombuffer(arr.buffers()[1], dtype=DEC128_DTYPE)[arr.offset:arr.offset + n]
            if validity is not None:
                cells = cells.copy()
                cells[~unpack_validity(validity, n)] = np.zeros((), dtype=DEC128_DTYPE)
            return Column(name, N.TYPE_DECIMAL128, cells, validity, decimal_precision=t.precision,
                          decimal_scale=t.scale)
        if t.precision > 18:
            raise ValueError("column %s: DecimalType(%d,%d) exceeds the 64-bit unscaled range (wide_decimals=True "
                             "loads it as a 128-bit decimal column)" % (name, t.precision, t.scale))
        # decimal128 cells are 16-byte little-endian two's complement; precision <= 18 fits the low 8 bytes
        cells = np.frombuffer(arr.buffers()[1], dtype=np.int64)[2 * arr.offset:2 * (arr.offset + n)]
        unscaled = np.ascontiguousarray(cells[0::2])
        if validity is not None:
            unscaled = np.where(unpack_validity(validity, n), unscaled, 0)
        return Column(name, N.TYPE_DECIMAL, unscaled, validity, decimal_precision=t.precision,
                      decimal_scale=t.scale)
    if pa.types.is_timestamp(t):
        us = arr.cast(pa.timestamp("us", tz=t.tz), safe=False) if t.unit != "us" else arr
        vals = np.frombuffer(us.buffers()[1], dtype=np.int64)[us.offset:us.offset + n]
        col = Column(name, N.TYPE_TIMESTAMP, vals, validity)
        col.tz = t.tz
        return col
    spark = {pa.int8(): N.TYPE_BYTE, pa.int16(): N.TYPE_SHORT, pa.int32(): N.TYPE_INT, pa.int64(): N.TYPE_LONG,
             pa.float32(): N.TYPE_FLOAT, pa.float64(): N.TYPE_DOUBLE, pa.date32(): N.TYPE_DATE}.get(t)
    if spark is None:
        raise ValueError("column %s: Arrow type %s has no Spark counterpart here" % (name, t))
    vals = np.frombuffer(arr.buffers()[1], dtype=NUMPY_OF[spark])[arr.offset:arr.offset + n]
    return Column(name, spark, vals, validity)


def column_to_arrow(col, pa):
    """A host column -> pyarrow array of its Spark type (inverse of _column_from_arrow), from the buffers."""
    n = col.length
    valid = unpack_validity(col.validity, n)
    mask = None if valid.all() else ~valid
    vbuf = None if mask is None else pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
    t = col.spark_type
    if isinstance(col, DictColumn):  # round-trips as a dictionary array (the entries as they are)
        ind = pa.array(col.indices[:n], type=pa.int32(), mask=mask)
        return pa.DictionaryArray.from_arrays(ind, column_to_arrow(col.dictionary, pa))
    if t == N.TYPE_STRING:
        off = np.ascontiguousarray(np.asarray(col.offsets, dtype=np.int32)[:n + 1])
        data = np.ascontiguousarray(np.asarray(col.values, dtype=np.uint8)[:int(off[-1]) if n else 0])
        return pa.Array.from_buffers(pa.string(), n, [vbuf, pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes())],
                                     null_count=-1)
    if t == N.TYPE_BOOLEAN:
        return pa.array(np.asarray(col.values)[:n] != 0, mask=mask)
    if t == N.TYPE_DATE:
        return pa.array(np.asarray(col.values, dtype=np.int32)[:n], type=pa.int32(), mask=mask).cast(pa.date32())
    if t == N.TYPE_TIMESTAMP:
        return pa.array(np.asarray(col.values, dtype=np.int64)[:n], type=pa.int64(), mask=mask).cast(pa.timestamp("us"))
    if t == N.TYPE_DECIMAL128:
        cells = np.ascontiguousarray(np.asarray(col.values, dtype=DEC128_DTYPE)[:n])
        return pa.Array.from_buffers(pa.decimal128(col.decimal_precision, col.decimal_scale), n,
                                     [vbuf, pa.py_buffer(cells.tobytes())], null_count=-1)
    if t == N.TYPE_DECIMAL:
        u = np.asarray(col.values, dtype=np.int64)[:n]
        cells = np.empty(2 * n, dtype=np.int64)
        cells[0::2] = u
        cells[1::2] = np.where(u < 0, -1, 0)
        return pa.Array.from_buffers(pa.decimal128(max(col.decimal_precision, 1), col.decimal_scale), n,
                                     [vbuf, pa.py_buffer(cells.tobytes())], null_count=-1)
    return pa.array(np.asarray(col.values, dtype=NUMPY_OF[t])[:n], mask=mask)


# ---- CSV output: the host path (the definition of Table.to_csv) -----------------------------------------
def _java_float_text(x, is_float):
    """Double.toString / Float.toString: the shortest digits that round-trip, plain for 1e-3 <= |x| < 1e7."""
    x = np.float32(x) if is_float else float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    if x == 0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    mant, exp = np.format_float_scientific(x, unique=True, trim="0").split("e")  # d.ddd, at least one fraction digit
    sign, mant = ("-", mant[1:]) if mant[0] == "-" else ("", mant)
    e = int(exp)
    if not (np.float32(1e-3) if is_float else 1e-3) <= abs(x) < 1e7:
        return "%s%sE%d" % (sign, mant, e)
    digits = mant.replace(".", "")
    if e < 0:
        return sign + "0." + "0" * (-e - 1) + (digits.rstrip("0") or "0")
    digits = digits.ljust(e + 2, "0")
    return sign + digits[:e + 1] + "." + digits[e + 1:]


def _java_civil(days):
    """(year of era, month, day) of a day number in java.util.GregorianCalendar: Gregorian from 1582-10-15 (Julian Day
    2299161), Julian before (E. G. Richards' day-number conversion; every // floors)."""
    j = days + 2440588
    f = j + 1401
    if j >= 2299161:
        f += (4 * j + 274277) // 146097 * 3 // 4 - 38
    e = 4 * f + 3
    h = 5 * (e % 1461 // 4) + 2
    day, month = h % 153 // 5 + 1, (h // 153 + 2) % 12 + 1
    year = e // 1461 - 4716 + (14 - month) // 12
    return (year if year >= 1 else 1 - year), month, day


def _date_text(days):
    return "%04d-%02d-%02d" % _java_civil(days)


def _timestamp_text(micros):
    secs, frac = divmod(micros, 1000000)
    days, sod = divmod(secs, 86400)
    text = "%s %02d:%02d:%02d" % (_date_text(days), sod // 3600, sod // 60 % 60, sod % 60)
    return text + (".%06d" % frac).rstrip("0") if frac else text


def _decimal_text(unscaled, scale):
    """BigDecimal.toString of unscaled * 10^-scale (scale >= 0): scientific when the adjusted exponent is below -6."""
    sign, digits = ("-" if unscaled < 0 else ""), str(abs(unscaled))
    adjusted = len(digits) - 1 - scale
    if scale == 0:
        return sign + digits
    if adjusted >= -6:
        digits = digits.rjust(scale + 1, "0")
        return sign + digits[:-scale] + "." + digits[-scale:]
    return sign + digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "E%d" % adjusted


def _csv_cell_bytes(col, i):
    """The bytes of the non-NULL cell i of a host column in a CSV file: Spark 2.2's Cast(x AS STRING); a STRING cell
    in quotes, every quote doubled, iff it holds ',', '"', LF or CR or is empty."""
    t = col.spark_type
    if t == N.TYPE_STRING:
        return _csv_quoted(bytes(col.values[col.offsets[i]:col.offsets[i + 1]]))
    v = col.values[i]
    if t == N.TYPE_BOOLEAN:
        text = "true" if v else "false"
    elif t in (N.TYPE_FLOAT, N.TYPE_DOUBLE):
        text = _java_float_text(v, t == N.TYPE_FLOAT)
    elif t == N.TYPE_DECIMAL:
        text = _decimal_text(int(v), col.decimal_scale)
    elif t == N.TYPE_DATE:
        text = _date_text(int(v))
    elif t == N.TYPE_TIMESTAMP:
        text = _timestamp_text(int(v))
    else:
        text = str(int(v))
    return text.encode("ascii")


def _csv_quoted(b):
    if b == b"" or any(c in b for c in b',"\n\r'):
        return b'"' + b.replace(b'"', b'""') + b'"'
    return b


def _csv_header(names):
    return b",".join(_csv_quoted(n.encode("utf-8")) for n in names) + b"\n"


def _csv_refuse_wide(table):
    for c in table.columns.values():
        if c.spark_type == N.TYPE_DECIMAL128:
            raise ValueError("column %s: %s has no CSV text yet (a 128-bit BigDecimal.toString is a later step); cast or "
                             "drop the column" % (c.name, c.type_name))


def _csv_body_host(table):
    cols = [c.decoded() if isinstance(c, DictColumn) else c for c in table.columns.values()]
    valid = [unpack_validity(c.validity, c.length) for c in cols]
    return b"".join(b",".join(_csv_cell_bytes(c, i) if v[i] else b"" for c, v in zip(cols, valid)) + b"\n"
                    for i in range(table.nrows))


def _csv_body_device(table):
    """The CSV body of a device-resident table as a device uint8 tensor (csv_write.hip through Context.csv_write)."""
    from . import engine
    cols = list(table.columns.values())
    missing = [c.name for c in cols if c.device is None]
    if missing:
        raise ValueError("to_csv of a device table: column %s has no device buffers (to_device() first)" % missing[0])
    first = cols[0].device["values"] if cols[0].device.get("values") is not None else cols[0].device["offsets"]
    dev = first.device
    ctx = engine.ctx()
    if not ctx.multi and ctx.device != dev.index:
        ctx = N.context(dev.index)
    return ctx.csv_write([c.native() for c in cols], table.nrows, dev)


def _is_device_table(table):
    return any(c.device is not None for c in table.columns.values())


def _csv_body(table):
    """bytes (host table) or a device uint8 tensor (device table)."""
    _csv_refuse_wide(table)
    if not table.columns:
        raise ValueError("to_csv: a table without columns has no records")
    return _csv_body_device(table) if _is_device_table(table) else _csv_body_host(table)


def _csv_write_file(path, names, header, bodies):
    """The header, then every body (bytes, or a device tensor that is downloaded once), into `path`; the bytes written."""
    total = 0
    with open(path, "wb") as f:
        if header:
            total += f.write(_csv_header(names))
        for b in bodies:
            if not isinstance(b, bytes):
                b = b.cpu().numpy()
            total += f.write(b)
    return total


def _column_to_host(c):
    """A device-resident column as a host column: every buffer downloaded once (the inverse of to_device)."""
    if isinstance(c, DictColumn):
        dd = c.dict_device
        validity = dd["validity"].cpu().numpy() if dd.get("validity") is not None else None
        return DictColumn(c.name, dd["indices"].cpu().numpy(), validity, c.dictionary)
    d, n = c.device, c.length
    validity = d["validity"].reshape(-1).cpu().numpy().view(np.uint8) if d.get("validity") is not None else None
    if c.spark_type == N.TYPE_STRING:
        offsets = d["offsets"].cpu().numpy()
        end = int(offsets[n]) if len(offsets) > n else 0
        out = Column(c.name, c.spark_type, d["values"][:end].cpu().numpy(), validity, offsets, length=n)
        if getattr(c, "offsets64", False):
            out.offsets64 = True
    else:
        dt = np.dtype(NUMPY_OF[c.spark_type])
        raw = d["values"].reshape(-1).cpu().numpy().view(np.uint8)[:n * dt.itemsize]
        out = Column(c.name, c.spark_type, raw.view(dt), validity, decimal_precision=c.decimal_precision,
                     decimal_scale=c.decimal_scale, length=n)
    out.tz = c.tz
    return out


def _table_to_arrow(table):
    import pyarrow as pa
    host = table.to_host()
    arrays = []
    for c in host.columns.values():
        a = column_to_arrow(c, pa)
        if c.spark_type == N.TYPE_TIMESTAMP and c.tz is not None:
            a = a.cast(pa.timestamp("us", tz=c.tz))
        arrays.append(a)
    return pa.Table.from_arrays(arrays, names=list(host.columns))


class Table:
    """Named columns of equal length (the DataFrame stand-in of the drop-in API)."""

    def __init__(self, columns):
        self.columns = OrderedDict()
        n = None
        for c in columns:
            if n is not None and c.length != n:
                raise ValueError("column %s has %d rows, expected %d" % (c.name, c.length, n))
            n = c.length
            self.columns[c.name] = c
        self.nrows = n or 0

    # ---- constructors ---------------------------------------------------------------------------
    @classmethod
    def from_rows(cls, rows, names, types=None):
        """Like Spark's `Seq((..),(..)).toDF(names...)`: None is null; types default from values."""
        cols = []
        for j, name in enumerate(names):
            items = [r[j] for r in rows]
            t = types[j] if types else _infer_py_type(items)
            cols.append(_column_from_pylist(name, t, items))
        return cls(cols)

    @classmethod
    def from_pydict(cls, data, types=None):
        cols = []
        for name, items in data.items():
            t = (types or {}).get(name) or _infer_py_type(list(items))
            cols.append(_column_from_pylist(name, t, list(items)))
        return cls(cols)

    @classmethod
    def from_arrays(cls, arrays, types=None, validity=None):
        """numpy arrays (fixed width) -> columns; `validity`: name -> bool mask."""
        cols = []
        for name, arr in arrays.items():
            arr = np.ascontiguousarray(arr)
            t = (types or {}).get(name)
            if t is None:
                t = {np.dtype(np.float64): N.TYPE_DOUBLE, np.dtype(np.float32): N.TYPE_FLOAT,
                     np.dtype(np.int64): N.TYPE_LONG, np.dtype(np.int32): N.TYPE_INT,
                     np.dtype(np.int16): N.TYPE_SHORT, np.dtype(np.int8): N.TYPE_BYTE,
                     np.dtype(np.bool_): N.TYPE_BOOLEAN}[arr.dtype]
            t = spark_type_of(t)
            vals = arr.astype(NUMPY_OF[t]) if t != N.TYPE_BOOLEAN else arr.astype(np.uint8)
            vm = (validity or {}).get(name)
            cols.append(Column(name, t, vals, pack_validity(vm) if vm is not None else None))
        return cls(cols)

    @classmethod
    def from_csv(cls, path, header=True, infer_schema=True, device=None):
        """CSV -> Table with Spark 2.2 CSV `inferSchema` typing (empty field = null). `device=d`: the file's bytes are
        uploaded once and tokenized, typed and parsed on GPU d into a device-resident Table (`_from_csv_device`): the
        same names, types, validity and cells as the host path, or a ValueError for input the host path reads
        leniently."""
        if device is not None:
            return _from_csv_device(cls, path, header, infer_schema, device)
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        names = rows[0] if header else ["_c%d" % i for i in range(len(rows[0]))]
        body = rows[1:] if header else rows
        cols = []
        for j, name in enumerate(names):
            raw = [(r[j] if j < len(r) else "") for r in body]
            items = [None if x == "" else x for x in raw]
            t = _csv_infer(items) if infer_schema else N.TYPE_STRING
            if t == N.TYPE_STRING:
                cols.append(_column_from_pylist(name, t, items))
            elif t == N.TYPE_DOUBLE:
                cols.append(_column_from_pylist(name, t, [None if x is None else float(x) for x in items]))
            elif t == N.TYPE_BOOLEAN:
                cols.append(_column_from_pylist(name, t, [None if x is None else x.lower() == "true" for x in items]))
            else:
                cols.append(_column_from_pylist(name, t, [None if x is None else int(x) for x in items]))
        return cls(cols)

    @classmethod
    def from_arrow(cls, table, wide_decimals=False, dictionaries="decode", device=None, chunk_rows=None):
        """pyarrow.Table (a Spark DataFrame collected through Arrow, or a parquet read) -> Table.
        Fixed-width values and UTF-8 offsets/data are taken from the Arrow buffers without a
        per-row pass; validity bitmaps are realigned to bit 0 and padded; booleans are widened to one
        byte per row, timestamps normalised to Spark's microseconds, decimals (precision <= 18) to
        unscaled longs. decimal128(p > 18, s) columns raise unless `wide_decimals`: then they load as 128-bit
        decimal columns (DQ_TYPE_DECIMAL128, the Arrow cells as they are), which the fused scan and the cast accept;
        every other analyzer over such a column fails alone.
        `dictionaries`: "decode" (default) rebuilds every row of a dictionary-encoded column on the host; "keep" holds
        dictionary<string> columns encoded (DictColumn: int32 indices + the dictionary; chunks with different
        dictionaries are unified), which device-resident tables scan and group without decoding. Dictionaries of
        other value types decode either way.
        `device=d`: the Arrow buffers are uploaded as they are and brought into the column layout on GPU d
        (`_from_arrow_device`, ingest.hip): a device-resident Table equal to `from_arrow(table).to_device(d)`, or that
        path's error, without a host pass over the rows. With `chunk_rows=k` a table of more than k rows comes back
        as a ChunkedTable of device tables of k rows, which is how a string column of 2^31 bytes and more loads."""
        if device is not None:
            return _from_arrow_device(cls, table, wide_decimals, dictionaries, device, chunk_rows)
        if chunk_rows is not None:
            raise ValueError("chunk_rows cuts a device-resident table into chunks: it needs device=")
        import pyarrow as pa
        if dictionaries not in ("decode", "keep"):
            raise ValueError("dictionaries must be 'decode' or 'keep', not %r" % (dictionaries,))
        cols = []
        for name, chunked in zip(table.column_names, table.columns):
            if dictionaries == "keep" and chunked.num_chunks > 1 and _kept_dictionary(chunked.type, pa):
                chunked = chunked.unify_dictionaries()
            arr = chunked.combine_chunks() if chunked.num_chunks != 1 else chunked.chunk(0)
            if isinstance(arr, pa.ChunkedArray):  # a column without chunks
                arr = arr.chunk(0) if arr.num_chunks == 1 else pa.array([], type=chunked.type)
            cols.append(_column_from_arrow(name, arr, pa, wide_decimals, dictionaries))
        return cls(cols)

    @classmethod
    def from_parquet(cls, path, columns=None, wide_decimals=False, dictionaries="decode", device=None, chunk_rows=None):
        """Parquet file or directory -> Table (through pyarrow, then `from_arrow`). dictionaries="keep" reads the
        string columns dictionary-encoded (`read_dictionary`) and holds them so. `device` and `chunk_rows` are
        `from_arrow`'s: pyarrow reads the file as before, the table it gives is ingested on the device."""
        import pyarrow as pa
        import pyarrow.parquet as pq
        if device is None and chunk_rows is not None:
            raise ValueError("chunk_rows cuts a device-resident table into chunks: it needs device=")
        if dictionaries == "keep":
            schema = pq.ParquetDataset(path).schema
            strings = [f.name for f in schema if (pa.types.is_string(f.type) or pa.types.is_large_string(f.type) or
                                                  _kept_dictionary(f.type, pa)) and
                       (columns is None or f.name in columns)]
            return cls.from_arrow(pq.read_table(path, columns=columns, read_dictionary=strings),
                                  wide_decimals=wide_decimals, dictionaries="keep", device=device, chunk_rows=chunk_rows)
        return cls.from_arrow(pq.read_table(path, columns=columns), wide_decimals=wide_decimals,
                              dictionaries=dictionaries, device=device, chunk_rows=chunk_rows)

    # ---- schema / access ------------------------------------------------------------------------
    @property
    def schema(self):
        return OrderedDict((n, c.type_name) for n, c in self.columns.items())

    @property
    def fieldNames(self):
        return list(self.columns)

    def __getitem__(self, name):
        return self.columns[name]

    def __contains__(self, name):
        return name in self.columns

    def count(self):
        return self.nrows

    def select_rows(self, mask):
        """Host-side row subset (test helper: builds partitions like parallelize(rows, numSlices))."""
        mask = np.asarray(mask, dtype=bool)
        out = []
        for c in self.columns.values():
            valid = unpack_validity(c.validity, c.length)[mask]
            if c.spark_type == N.TYPE_STRING:
                items = [c.value_at(i) for i in np.nonzero(mask)[0]]
                items = [x if v else None for x, v in zip(items, valid)]
                out.append(_column_from_pylist(c.name, c.spark_type, items))
            else:
                vals = c.values[mask]
                nc = Column(c.name, c.spark_type, np.ascontiguousarray(vals),
                            None if valid.all() else pack_validity(valid), decimal_precision=c.decimal_precision,
                            decimal_scale=c.decimal_scale)
                out.append(nc)
        return Table(out)

    def to_device(self, device=0):
        """Copy every buffer into HBM (torch tensors as the allocator); runs then read device memory."""
        import torch
        dev = torch.device("cuda", device)
        for c in self.columns.values():
            if isinstance(c, DictColumn):
                c.to_device(dev)
                continue
            d = {}
            if c.spark_type == N.TYPE_STRING:
                d["values"] = torch.from_numpy(np.concatenate([c.values, np.zeros(16, np.uint8)])).to(dev)
                d["offsets"] = torch.from_numpy(c.offsets.astype(np.int32)).to(dev)
            else:
                d["values"] = torch.from_numpy(np.ascontiguousarray(c.values).view(np.uint8).reshape(-1).copy()).to(dev)
            if c.validity is not None:
                d["validity"] = torch.from_numpy(pack_validity(unpack_validity(c.validity, c.length))).to(dev)
            c.device = d
        return self

    def to_host(self):
        """The inverse of `to_device`, buffer for buffer: a new host Table whose values, validity words, int32 offsets,
        dictionary indices and entries are the device buffers downloaded once each (a column without a bitmap stays
        without one). A host table returns itself."""
        if not _is_device_table(self):
            return self
        return Table([_column_to_host(c) if c.device is not None else c for c in self.columns.values()])

    def to_arrow(self):
        """The table as a pyarrow.Table (`column_to_arrow` per column over the buffers; a device table is downloaded
        once, `to_host`): no per-row Python. `Table.from_arrow(t.to_arrow(), wide_decimals=True, dictionaries="keep")`
        gives back the buffers of `t`."""
        return _table_to_arrow(self)

    def to_parquet(self, path):
        """`pyarrow.parquet.write_table` of `to_arrow()`."""
        import pyarrow.parquet as pq
        pq.write_table(self.to_arrow(), path)

    def to_csv(self, path, header=True):
        """Write the table as CSV: ',' delimiter, '"' quote, doubled-quote escape, LF after every
        record; a cell is Spark 2.2's Cast(x AS STRING), NULL is zero bytes, a STRING cell is quoted iff it holds ',',
        '"', LF or CR or is empty. A host table is written by the host path (`_csv_body_host`: the definition), a
        device-resident table by csv_write.hip, byte for byte the same file. DECIMAL128 columns and device bodies of
        2^31 bytes and more raise ValueError. Returns the bytes written."""
        return _csv_write_file(path, self.fieldNames, header, [_csv_body(self)])


class ChunkedTable:
    """A table held as consecutive row chunks (Arrow record batches) of one schema: the shape of a DataFrame's
    partitions, and how a shard whose string bytes exceed one column's int32 offsets (2^31 bytes) is held.
    AnalysisRunner runs every chunk and merges the chunk states with the reference's semigroup merges
    (runOnAggregatedStates, R/AnalysisRunner.scala:385-460) — the per-partition aggregation Spark performs inside
    one `agg`; ColumnProfiler runs its three passes the same way."""

    def __init__(self, chunks):
        chunks = list(chunks)
        if not chunks:
            raise ValueError("a ChunkedTable needs at least one chunk")
        schema = chunks[0].schema
        for t in chunks[1:]:
            if t.schema != schema:
                raise ValueError("chunks of a ChunkedTable must share one schema")
        self.chunks = chunks
        self.nrows = sum(t.nrows for t in chunks)

    @property
    def schema(self):
        return self.chunks[0].schema

    @property
    def fieldNames(self):
        return self.chunks[0].fieldNames

    def __getitem__(self, name):
        """The first chunk's column: type and metadata only (values live in every chunk)."""
        return self.chunks[0][name]

    def __contains__(self, name):
        return name in self.chunks[0]

    def count(self):
        return self.nrows

    def to_arrow(self):
        """The chunks' `Table.to_arrow()` tables concatenated."""
        import pyarrow as pa
        return pa.concat_tables([t.to_arrow() for t in self.chunks])

    def to_csv(self, path, header=True):
        """The header once, then every chunk's body appended (`Table.to_csv`): the file of the concatenated table.
        Each chunk's body is below 2^31 bytes on the device; the file may be larger. Returns the bytes written."""
        return _csv_write_file(path, self.fieldNames, header, (_csv_body(t) for t in self.chunks))

    def concat(self, names):
        """The named columns of every chunk as one Table, concatenated where the chunks live (HBM when every chunk is
        device-resident, else host memory): a string column's offsets become int64 (Arrow large_string,
        DQ_COL_OFFSETS64) so its bytes may pass 2^31. The grouping builds take it whole, so a grouping over the shard
        is one frequency table (not per-chunk tables merged through host memory)."""
        on_device = all(all(c[n].device is not None for n in names) for c in self.chunks)
        cols = [(_concat_device if on_device else _concat_host)([c[n] for c in self.chunks]) for n in names]
        if on_device and cols:
            import torch
            # the copies run on this thread's torch stream of the columns' device, the builds that read them on the
            # context's own stream
            torch.cuda.current_stream(cols[0].device["values"].device).synchronize()
        return Table(cols)

    def parted(self, names):
        """The named columns as PartedColumns over the chunks (no copy): the ApproxQuantile summaries of the shard
        read every chunk in one dq_quantile_summaries call."""
        return Table([PartedColumn([c[n] for c in self.chunks]) for n in names])

    def grouping_view(self, names):
        """The key columns of a grouping over the whole shard: read in place as two parts (dq_frequencies_parts) when
        the shard is two device chunks and a key is a string (the general build, no HBM concatenation and no host
        synchronisation), else concatenated (a fixed-width single key keeps the fast build over one column).
        DQ_GROUP_CONCAT=1 always concatenates."""
        import os
        cols = [self.chunks[0][n] for n in names]
        if len(names) == 1 and all(isinstance(ch[names[0]], DictColumn) and ch[names[0]].dict_device is not None
                                   for ch in self.chunks):
            return self.parted(names)  # dictionary-encoded chunks: counted per chunk, their entries built once
        if len(self.chunks) == 2 and not os.environ.get("DQ_GROUP_CONCAT") and \
                any(c.spark_type == N.TYPE_STRING for c in cols) and \
                all(ch[n].device is not None and not getattr(ch[n], "offsets64", False)
                    for ch in self.chunks for n in names):
            return self.parted(names)
        return self.concat(names)


def _infer_py_type(items):
    nn = [x for x in items if x is not None]
    if not nn:
        return N.TYPE_STRING
    if all(isinstance(x, bool) for x in nn):
        return N.TYPE_BOOLEAN
    if all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in nn):
        return N.TYPE_INT if all(-2 ** 31 <= int(x) < 2 ** 31 for x in nn) else N.TYPE_LONG
    if all(isinstance(x, (int, float, np.integer, np.floating)) for x in nn):
        return N.TYPE_DOUBLE
    return N.TYPE_STRING


_INT_RE = re.compile(r"^[+-]?\d+$")


def _csv_infer(items):
    """Spark 2.2 CSVInferSchema per column: Integer -> Long -> Decimal(p,0) -> Double -> Boolean -> String."""
    rank = {None: 0, N.TYPE_INT: 1, N.TYPE_LONG: 2, N.TYPE_DOUBLE: 4, N.TYPE_BOOLEAN: 5, N.TYPE_STRING: 6}
    cur = None
    for x in items:
        if x is None:
            continue
        t = _csv_field_type(x)
        if cur is None:
            cur = t
        elif t != cur:
            if {t, cur} <= {N.TYPE_INT, N.TYPE_LONG, N.TYPE_DOUBLE}:
                cur = max(t, cur, key=lambda k: rank[k])
            else:
                cur = N.TYPE_STRING
        if cur == N.TYPE_STRING:
            break
    return cur if cur is not None else N.TYPE_STRING


def _csv_field_type(x):
    if _INT_RE.match(x):
        v = int(x)
        if -2 ** 31 <= v < 2 ** 31:
            return N.TYPE_INT
        if -2 ** 63 <= v < 2 ** 63:
            return N.TYPE_LONG
        return N.TYPE_DOUBLE
    try:
        float(x)
        if re.match(r"^[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?[dDfF]?$", x) or x in ("NaN", "Infinity", "-Infinity"):
            return N.TYPE_DOUBLE
    except ValueError:
        pass
    if x.lower() in ("true", "false"):
        return N.TYPE_BOOLEAN
    return N.TYPE_STRING


def _csv_type_of_classes(classes):
    """The column type of the OR of its fields' classes (N.CSV_CLASS_*): what _csv_infer's sequential fold gives for
    any order of fields of those classes. A subset of {INT, LONG, DOUBLE} is its widest member, {BOOLEAN} is BOOLEAN,
    anything else (and no field at all) is STRING."""
    if classes and not classes & ~(N.CSV_CLASS_INT | N.CSV_CLASS_LONG | N.CSV_CLASS_DOUBLE):
        return N.TYPE_DOUBLE if classes & N.CSV_CLASS_DOUBLE else \
            N.TYPE_LONG if classes & N.CSV_CLASS_LONG else N.TYPE_INT
    return N.TYPE_BOOLEAN if classes == N.CSV_CLASS_BOOLEAN else N.TYPE_STRING


def _csv_first_record(raw):
    """(fields, complete) of the first record of a file's first bytes (the header), read as dq_csv_index reads
    records: up to the first LF outside quotes (`complete`: there is one in `raw`), a CR before it dropped, split at
    the commas outside quotes, quoted fields unquoted. A record of zero bytes has no fields."""
    end, quotes, at = None, 0, 0
    while end is None:
        nl = raw.find(b"\n", at)
        if nl < 0:
            break
        quotes += raw.count(b'"', at, nl)
        if quotes % 2 == 0:
            end = nl
        at = nl + 1
    rec = raw if end is None else raw[:end]
    if end is not None and rec.endswith(b"\r"):
        rec = rec[:-1]
    fields, start, inside = [], 0, False
    for i in range(len(rec) + 1 if rec else 0):
        c = rec[i:i + 1]
        if c == b'"':
            inside = not inside
        if i == len(rec) or (c == b"," and not inside):
            f = rec[start:i]
            if f[:1] == b'"':
                f = f[1:-1].replace(b'""', b'"')
            fields.append(f.decode("utf-8", errors="replace"))
            start = i + 1
    return fields, end is not None


def _from_csv_device(cls, path, header, infer_schema, device):
    """Table.from_csv on the GPU (csv.hip): one upload of the file's bytes, then dq_csv_index (records, field spans,
    per-column classes, refusals) and one dq_csv_column per column into torch buffers laid out as `to_device` lays
    them out. Only the header record and, for a column with ambiguous fields, one field are read on the host."""
    nbytes = os.path.getsize(path)
    if nbytes == 0:
        raise ValueError("%s: an empty file has no header and no rows" % path)
    if nbytes >= 2 ** 31:
        raise ValueError("%s: %d bytes: the device reader takes files below 2^31 bytes" % (path, nbytes))
    raw = np.fromfile(path, dtype=np.uint8)
    head = 1 << 16
    while True:
        first, complete = _csv_first_record(raw[:head].tobytes())
        if complete or head >= len(raw):
            break
        head *= 4
    names = first if header else ["_c%d" % i for i in range(len(first))]
    import torch
    from . import engine
    dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
    ctx = engine.ctx()
    if ctx.multi or ctx.device != dev.index:
        ctx = N.context(dev.index)
    data = torch.from_numpy(raw).to(dev)
    handle, res, reports = ctx.csv_index(data.data_ptr(), len(raw), max(len(names), 1), 1 if header else 0)
    if res.refusal_kind:
        raise ValueError("%s: %s at byte %d: csv.reader reads this leniently, the device reader refuses it"
                         % (path, N.CSV_REFUSALS[res.refusal_kind], res.refusal_offset))
    try:
        if not names:
            raise ValueError("%s: the first record has no fields" % path)
        n = int(res.nrows)
        cols = []
        for j, name in enumerate(names):
            rep = reports[j]
            t = _csv_type_of_classes(rep.classes) if infer_schema else N.TYPE_STRING
            if infer_schema and rep.ambiguous and not rep.classes & N.CSV_CLASS_STRING:
                # Python's \d and $ accept more than ASCII digits: the host types the first such field
                start, length, escaped = ctx.csv_field(handle, rep.first_ambiguous_row, j)
                if escaped:
                    field = raw[start:start + 2 * length].tobytes().replace(b'""', b'"')[:length]
                else:
                    field = raw[start:start + length].tobytes()
                if _csv_field_type(field.decode("utf-8")) != N.TYPE_STRING:
                    raise ValueError("%s: column %r: row %d holds %r, which the host path reads as a number or boolean "
                                     "but the device does not parse; infer_schema=False loads the column as strings"
                                     % (path, name, rep.first_ambiguous_row, field.decode("utf-8")))
                t = N.TYPE_STRING
            col = Column(name, t, None, None, length=n)
            d = {}
            if rep.valid < n:
                d["validity"] = torch.zeros(max((n + 63) // 64, 1) * 8, dtype=torch.uint8, device=dev)
            vptr = d["validity"].data_ptr() if "validity" in d else None
            if t == N.TYPE_STRING:
                d["offsets"] = torch.empty(n + 1, dtype=torch.int32, device=dev)
                total = ctx.csv_column(handle, j, t, None, vptr, d["offsets"].data_ptr())
                d["values"] = torch.empty(total + 16, dtype=torch.uint8, device=dev)
                ctx.csv_column(handle, j, t, d["values"].data_ptr(), None, d["offsets"].data_ptr())
            else:
                d["values"] = torch.empty(n * np.dtype(NUMPY_OF[t]).itemsize, dtype=torch.uint8, device=dev)
                ctx.csv_column(handle, j, t, d["values"].data_ptr(), vptr)
            col.device = d
            cols.append(col)
    finally:
        ctx.csv_free(handle)
    return cls(cols)


def _arrow_pieces(chunk_lengths, chunk_offsets, chunk_rows=None):
    """The row ranges of a chunked Arrow column for every output chunk: a list (one entry per output chunk, over rows
    [0, k), [k, 2k), ... with k = chunk_rows; one chunk of every row without it or when the rows fit one) of lists of
    pieces (arrow chunk, first row, rows, first output row). `first row` counts in the chunk's BUFFERS, so it includes
    the chunk's Arrow offset; `first output row` counts inside the output chunk. Pieces are never empty: chunks of
    zero rows give none, and a column without rows gives one output chunk without pieces. Pure arithmetic: no
    pyarrow, no torch."""
    lengths = [int(x) for x in chunk_lengths]
    total = sum(lengths)
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("chunk_rows must be at least 1, not %r" % (chunk_rows,))
    step = total if chunk_rows is None or total <= int(chunk_rows) else int(chunk_rows)
    out, c, used = [], 0, 0  # the Arrow chunk being handed out and its rows already taken
    for r0 in range(0, total, step or 1):
        rows = min(step, total - r0)
        pieces, at = [], 0
        while at < rows:
            if used == lengths[c]:
                c, used = c + 1, 0
                continue
            take = min(lengths[c] - used, rows - at)
            pieces.append((c, int(chunk_offsets[c]) + used, take, at))
            used += take
            at += take
        out.append(pieces)
    return out or [[]]


class _ArrowUpload:
    """Byte ranges of Arrow buffers into HBM for `_from_arrow_device`: each range is a zero-copy view of the Arrow
    buffer (np.frombuffer, then torch), copied once, either into its place in a final buffer (`put`) or into a
    staging tensor a kernel reads (`stage`, `stage_bits`). The copies run on torch's current stream; the native
    wrappers wait for that stream before they launch (Context._after_torch_stream) and return after their kernels
    have finished, so a staging tensor may be dropped as soon as its call returns."""

    def __init__(self, ctx, dev, torch):
        self.ctx, self.dev, self.torch = ctx, dev, torch

    def view(self, buf, start, stop):
        import warnings
        a = np.frombuffer(buf, dtype=np.uint8)[start:stop]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # torch warns that the (read-only) Arrow memory is not writable: it is only read
            return self.torch.from_numpy(a)

    def empty(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.dev)

    def put(self, dst, at, buf, start, stop):
        if stop > start:
            dst[at:at + stop - start].copy_(self.view(buf, start, stop))

    def stage(self, buf, start, stop):
        return self.view(buf, start, stop).to(self.dev)

    def stage_bits(self, items):
        """[(bitmap buffer or None, first bit, rows)] -> (the staging tensor, [(ptr or None, bytes, bit0, rows)] as
        Context.ingest_bits takes them): the bytes first // 8 .. (first + rows + 7) // 8 of each bitmap, each at an
        8-byte boundary of one tensor."""
        spans = [(first >> 3, (first + rows + 7) >> 3) if buf is not None else (0, 0) for buf, first, rows in items]
        stage = self.empty(sum((b - a + 7) & ~7 for a, b in spans))
        pieces, at = [], 0
        for (buf, first, rows), (a, b) in zip(items, spans):
            if buf is None:
                pieces.append((None, 0, 0, rows))
                continue
            self.put(stage, at, buf, a, b)
            pieces.append((stage.data_ptr() + at, b - a, first & 7, rows))
            at += (b - a + 7) & ~7
        return stage, pieces


def _piece_nulls(arr, first, rows):
    """The NULLs of rows [first, first + rows) of an Arrow array's buffers (Arrow's own count over the bitmap)."""
    if arr.null_count == 0:
        return 0
    return arr.null_count if rows == len(arr) else arr.slice(first - arr.offset, rows).null_count


def _arrow_device_plain(up, pa, name, t, chunks, pieces, wide_decimals):
    """The rows `pieces` name (see _arrow_pieces) of the Arrow arrays `chunks`, all of type `t` (not a dictionary), as
    one device-only Column laid out as `Table.to_device` lays it out. The type decisions and their errors are
    `_column_from_arrow`'s."""
    torch, ctx = up.torch, up.ctx
    n = sum(p[2] for p in pieces)
    large = pa.types.is_large_string(t)
    convert, width, prec, scale = None, 0, 0, 0  # convert: (dq_ingest_kind, param) when the cells need a kernel
    if large or pa.types.is_string(t):
        spark = N.TYPE_STRING
    elif pa.types.is_boolean(t):
        spark = N.TYPE_BOOLEAN
    elif pa.types.is_decimal(t):
        if t.precision > 18 and wide_decimals and pa.types.is_decimal128(t):
            spark, width, convert = N.TYPE_DECIMAL128, 16, (N.INGEST_DECIMAL_WIDE, 0)
        elif t.precision > 18:
            raise ValueError("column %s: DecimalType(%d,%d) exceeds the 64-bit unscaled range (wide_decimals=True "
                             "loads it as a 128-bit decimal column)" % (name, t.precision, t.scale))
        elif not pa.types.is_decimal128(t):
            raise ValueError("column %s: Arrow type %s: the device path reads decimal128 cells only" % (name, t))
        else:
            spark, width, convert = N.TYPE_DECIMAL, 16, (N.INGEST_DECIMAL_LOW, 0)
        prec, scale = t.precision, t.scale
    elif pa.types.is_timestamp(t):
        spark, width = N.TYPE_TIMESTAMP, 8
        convert = {"s": (N.INGEST_TIME_MUL, 10 ** 6), "ms": (N.INGEST_TIME_MUL, 1000), "us": None,
                   "ns": (N.INGEST_TIME_DIV, 1000)}[t.unit]
    else:
        spark = {pa.int8(): N.TYPE_BYTE, pa.int16(): N.TYPE_SHORT, pa.int32(): N.TYPE_INT, pa.int64(): N.TYPE_LONG,
                 pa.float32(): N.TYPE_FLOAT, pa.float64(): N.TYPE_DOUBLE, pa.date32(): N.TYPE_DATE}.get(t)
        if spark is None:
            raise ValueError("column %s: Arrow type %s has no Spark counterpart here" % (name, t))
        width = np.dtype(NUMPY_OF[spark]).itemsize
    bufs = {c: chunks[c].buffers() for c, _, _, _ in pieces}
    d = {}
    # validity: absent when no piece holds a NULL, else the pieces' bitmaps concatenated bitwise in one launch
    nulls = [_piece_nulls(chunks[c], first, rows) for c, first, rows, _ in pieces]
    vstage, vpieces = None, [(None, 0, 0, rows) for _, _, rows, _ in pieces]
    if sum(nulls):
        vstage, vpieces = up.stage_bits([(bufs[c][0] if k else None, first, rows)
                                         for (c, first, rows, _), k in zip(pieces, nulls)])
        d["validity"] = up.empty(max((n + 63) // 64, 1) * 8)
        ctx.ingest_bits(vpieces, n, False, d["validity"].data_ptr())
    if spark == N.TYPE_STRING:
        w, odt = (8, np.int64) if large else (4, np.int32)
        spans = []
        for c, first, rows, _ in pieces:  # the two offsets that bound the piece's bytes
            o = np.frombuffer(bufs[c][1], dtype=odt)
            spans.append((int(o[first]), int(o[first + rows])))
        total = sum(b - a for a, b in spans)
        too_long = ValueError("column %s: its strings hold %d bytes, more than the int32 offsets of one column address "
                              "(2^31 - 17); chunk_rows=k loads the table as chunks of k rows" % (name, total))
        if total > 2 ** 31 - 17:
            raise too_long
        d["values"] = up.empty(total + 16)
        d["values"][total:] = 0  # the read-past padding of the dword loads
        if n == 0:
            # no piece writes the one offset: the host path leaves the raw Arrow offset of a single empty string chunk
            # there (nothing reads it), and so does this one
            first = 0 if len(chunks) != 1 or large else int(np.frombuffer(chunks[0].buffers()[1], dtype=odt)[chunks[0].offset])
            d["offsets"] = torch.full((1,), first, dtype=torch.int32, device=up.dev)
        else:
            d["offsets"] = torch.empty(n + 1, dtype=torch.int32, device=up.dev)
        base = 0
        for i, ((c, first, rows, row0), (a, b)) in enumerate(zip(pieces, spans)):
            up.put(d["values"], base, bufs[c][2], a, b)
            src = up.stage(bufs[c][1], first * w, (first + rows + 1) * w)
            if ctx.ingest_offsets(src.data_ptr(), src.numel(), w, rows, base, i == len(pieces) - 1,
                                  d["offsets"].data_ptr() + 4 * row0):
                raise too_long
            base += b - a
    elif spark == N.TYPE_BOOLEAN:
        d["values"] = up.empty(n)
        if n:
            bits, bpieces = up.stage_bits([(bufs[c][1], first, rows) for c, first, rows, _ in pieces])
            ctx.ingest_bits(bpieces, n, True, d["values"].data_ptr())
    else:
        out_width = np.dtype(NUMPY_OF[spark]).itemsize
        d["values"] = up.empty(n * out_width)
        for (c, first, rows, row0), v in zip(pieces, vpieces):
            if convert is None or (convert[0] == N.INGEST_DECIMAL_WIDE and v[0] is None):
                up.put(d["values"], row0 * out_width, bufs[c][1], first * width, (first + rows) * width)
                continue
            src = up.stage(bufs[c][1], first * width, (first + rows) * width)
            ctx.ingest_convert(convert[0], src.data_ptr(), src.numel(), v[:3] if v[0] is not None else None, rows,
                               convert[1], d["values"].data_ptr() + row0 * out_width)
    del vstage  # vpieces point into it: it had to live until the conversions had read their validity bits
    col = Column(name, spark, None, None, decimal_precision=prec, decimal_scale=scale, length=n)
    col.device = d
    if spark == N.TYPE_TIMESTAMP:
        col.tz = t.tz
    return col


def _arrow_device_dict(up, pa, name, chunked):
    """A dictionary<string> ChunkedArray under dictionaries="keep" as a device-only DictColumn: what
    `_dict_column_from_arrow` and `DictColumn.to_device` build. The dictionary's entries are read on the host (they
    are few); the indices are widened, checked and folded with the NULL entries on the device."""
    torch, ctx = up.torch, up.ctx
    if chunked.num_chunks > 1:
        chunked = chunked.unify_dictionaries()
    chunks, t = chunked.chunks, chunked.type
    entries = chunks[0].dictionary if chunks else pa.array([], type=t.value_type)
    if pa.types.is_large_string(entries.type):
        entries = entries.cast(pa.string())
    dictionary = _string_column_from_arrow(name, entries, _arrow_validity(entries, len(entries)))
    nd = dictionary.length
    dd = _dictionary_device(dictionary, up.dev, torch)
    dict_validity = dd["dict_validity"].data_ptr() if dictionary.validity is not None else None
    pieces = _arrow_pieces([len(c) for c in chunks], [c.offset for c in chunks])[0]
    n = sum(p[2] for p in pieces)
    w, signed = t.index_type.bit_width // 8, pa.types.is_signed_integer(t.index_type)
    dd["indices"] = torch.empty(n, dtype=torch.int32, device=up.dev)
    folds, folded, null_rows = [], [], 0  # the pieces' folded bitmaps (kept until they are concatenated)
    for c, first, rows, row0 in pieces:
        bufs = chunks[c].buffers()  # of a DictionaryArray: the validity bitmap and the indices
        v, vstage = None, None  # vstage holds the bytes v points at until the piece's call has returned
        if _piece_nulls(chunks[c], first, rows):
            vstage, vp = up.stage_bits([(bufs[0], first, rows)])
            v = vp[0][:3]
        fold = up.empty((rows + 63) // 64 * 8) if v is not None or dict_validity else None
        src = up.stage(bufs[1], first * w, (first + rows) * w)
        bad_row, bad_index, nulls = ctx.ingest_indices(src.data_ptr(), src.numel(), w, signed, v, rows, nd, dict_validity,
                                                       dd["indices"].data_ptr() + 4 * row0,
                                                       fold.data_ptr() if fold is not None else None)
        if bad_row >= 0:
            raise ValueError("column %s: row %d has dictionary index %d outside [0, %d)"
                             % (name, row0 + bad_row, bad_index, nd))
        null_rows += nulls
        folds.append(fold)
        folded.append((fold.data_ptr(), fold.numel(), 0, rows) if fold is not None else (None, 0, 0, rows))
    if null_rows:
        dd["validity"] = up.empty(max((n + 63) // 64, 1) * 8)
        ctx.ingest_bits(folded, n, False, dd["validity"].data_ptr())
    del folds  # `folded` pointed into them
    col = DictColumn(name, None, None, dictionary, length=n)
    col.dict_device = dd
    return col


def _from_arrow_device(cls, table, wide_decimals, dictionaries, device, chunk_rows):
    """Table.from_arrow on the GPU (ingest.hip). The host reads metadata only: per column and Arrow chunk the type,
    offset, length, null count, buffer addresses and the two string offsets that bound a piece; it never walks the
    rows (no combine_chunks, cast, unpackbits or copy of a row buffer). Two exceptions pyarrow already implements stay
    on the host: dictionary_decode() of a dictionary column that is not kept, and unify_dictionaries() of a kept one
    whose chunks carry different dictionaries. Columns are taken in order, so the first error is the host path's."""
    import pyarrow as pa
    import torch
    from . import engine
    if dictionaries not in ("decode", "keep"):
        raise ValueError("dictionaries must be 'decode' or 'keep', not %r" % (dictionaries,))
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("chunk_rows must be at least 1, not %r" % (chunk_rows,))
    dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
    ctx = engine.ctx()
    if ctx.multi or ctx.device != dev.index:
        ctx = N.context(dev.index)
    up = _ArrowUpload(ctx, dev, torch)
    n = table.num_rows
    chunked_out = chunk_rows is not None and n > int(chunk_rows)
    step = int(chunk_rows) if chunked_out else None
    out = [[] for _ in range((n + step - 1) // step if chunked_out else 1)]
    for name, column in zip(table.column_names, table.columns):
        t = column.type
        if dictionaries == "keep" and _kept_dictionary(t, pa):
            # a chunk's dictionary is that of its own rows, as from_arrow(table.slice(...)) has it
            cols = [_arrow_device_dict(up, pa, name, column.slice(k * step, step) if chunked_out else column)
                    for k in range(len(out))]
        else:
            chunks = column.chunks
            if pa.types.is_dictionary(t):
                chunks, t = [c.dictionary_decode() for c in chunks], t.value_type
            plan = _arrow_pieces([len(c) for c in chunks], [c.offset for c in chunks], step)
            cols = [_arrow_device_plain(up, pa, name, t, chunks, pieces, wide_decimals) for pieces in plan]
        for tcols, col in zip(out, cols):
            tcols.append(col)
    torch.cuda.current_stream(dev).synchronize()  # the uploads ran on torch's stream, the scans run on the context's
    tables = [cls(cols) for cols in out]
    return ChunkedTable(tables) if chunked_out else tables[0]


def _concat_host(parts):
    """Host columns of consecutive chunks as one column (int64 string offsets)."""
    first = parts[0]
    n = sum(p.length for p in parts)
    valid = np.concatenate([unpack_validity(p.validity, p.length) for p in parts]) if parts else np.zeros(0, bool)
    validity = None if valid.all() else pack_validity(valid)
    if first.spark_type == N.TYPE_STRING:
        offs, datas, base = [np.zeros(1, dtype=np.int64)], [], 0
        for p in parts:
            o = np.asarray(p.offsets, dtype=np.int64)[:p.length + 1]
            datas.append(np.asarray(p.values, dtype=np.uint8)[int(o[0]):int(o[-1])])
            offs.append(o[1:] - o[0] + base)
            base += int(o[-1] - o[0])
        col = Column(first.name, N.TYPE_STRING, np.concatenate(datas) if datas else np.zeros(0, np.uint8), validity,
                     np.concatenate(offs), length=n)
        col.offsets64 = True
        return col
    vals = np.concatenate([np.asarray(p.values)[:p.length] for p in parts])
    return Column(first.name, first.spark_type, vals, validity, decimal_precision=first.decimal_precision,
                  decimal_scale=first.decimal_scale, length=n)


def _device_valid_bits(col, torch):
    """One bool per row of a device column's validity (all True without a bitmap)."""
    d = col.device
    dev = d["values"].device
    if d.get("validity") is None:
        return torch.ones(col.length, dtype=torch.bool, device=dev)
    v = d["validity"][:(col.length + 7) // 8]
    bits = (v.unsqueeze(1) >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1
    return bits.reshape(-1)[:col.length].bool()


def _concat_device(parts):
    """Device columns of consecutive chunks as one device column: values / UTF-8 bytes copied in HBM, validity bits
    re-packed at the chunk boundaries (byte-wise when every chunk but the last holds a multiple of 8 rows), string
    offsets rebased into int64 in place in the output."""
    import torch
    first = parts[0]
    dev = first.device["values"].device
    n = sum(p.length for p in parts)
    col = Column(first.name, first.spark_type, None, None, decimal_precision=first.decimal_precision,
                 decimal_scale=first.decimal_scale, length=n)
    d = {}
    if any(p.device.get("validity") is not None for p in parts):
        nwords = max((n + 63) // 64, 1)
        if all(p.length % 8 == 0 for p in parts[:-1]):
            out = torch.zeros(nwords * 8, dtype=torch.uint8, device=dev)
            at = 0
            for p in parts:
                nb = (p.length + 7) // 8
                v = p.device.get("validity")
                if v is None:
                    out[at:at + nb] = 0xFF
                    if p.length % 8:
                        out[at + nb - 1] = (1 << (p.length % 8)) - 1
                else:
                    out[at:at + nb].copy_(v[:nb])
                    if p.length % 8:  # bits past the chunk's last row read as NULL
                        out[at + nb - 1] &= (1 << (p.length % 8)) - 1
                at += nb
            d["validity"] = out
        else:
            bits = torch.cat([_device_valid_bits(p, torch) for p in parts])
            padded = torch.zeros(nwords * 64, dtype=torch.uint8, device=dev)
            padded[:n] = bits.to(torch.uint8)
            w = (1 << torch.arange(8, device=dev, dtype=torch.int32))
            d["validity"] = (padded.reshape(-1, 8).to(torch.int32) * w).sum(dim=1).to(torch.uint8)
    if first.spark_type == N.TYPE_STRING:
        spans = []
        for p in parts:
            o = p.device["offsets"]
            spans.append((int(o[0].item()), int(o[p.length].item())))
        total = sum(b - a for a, b in spans)
        data = torch.empty(total + 16, dtype=torch.uint8, device=dev)  # + read-past padding of the dword loads
        data[total:] = 0
        offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        offs[0] = 0
        at, base = 0, 0
        for p, (o0, o1) in zip(parts, spans):
            data[base:base + o1 - o0].copy_(p.device["values"][o0:o1])
            seg = offs[at + 1:at + 1 + p.length]
            seg.copy_(p.device["offsets"][1:p.length + 1])
            seg.add_(base - o0)
            at += p.length
            base += o1 - o0
        d["values"], d["offsets"] = data, offs
        col.offsets64 = True
    else:
        width = np.dtype(NUMPY_OF[first.spark_type]).itemsize
        d["values"] = torch.cat([p.device["values"].reshape(-1).view(torch.uint8)[:p.length * width] for p in parts])
    col.device = d
    return col
