"""Pure-Python restatement of the row-level schema validator's semantics (schema/RowLevelSchemaValidator.scala:225-281
under Spark 2.2 in a UTC session zone), written independently of the C parsers: the reference the tests compare
libdq's host parsers and the GPU validator with.

A schema is a list of dicts, as tests/golden/schema_kats.json writes them:
  {"type": "string", "name", "isNullable", "minLength", "maxLength", "matches"}
  {"type": "int", "name", "isNullable", "minValue", "maxValue"}
  {"type": "decimal", "name", "precision", "scale", "isNullable"}
  {"type": "timestamp", "name", "mask", "isNullable"}
Casts return (class, value) with class VALUE / NULL / AMBIGUOUS.
"""
import datetime
import decimal
import re

import oracle as O

VALUE, NULL, AMBIGUOUS = 1, 0, 2  # the return codes of dq_parse_decimal / dq_parse_timestamp

MAX_EXPONENT = 10000


def cast_int(s):
    """UTF8String.toInt: toLong's grammar, NULL outside the int range."""
    v = O.spark_string_to_long(s)
    if v is None or not -(1 << 31) <= v <= (1 << 31) - 1:
        return NULL, None
    return VALUE, v


_DECIMAL = re.compile(r"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE]([+-]?[0-9]+))?", re.ASCII)
_DEC_CTX = decimal.Context(prec=64, rounding=decimal.ROUND_HALF_UP, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)


def cast_decimal(s, precision, scale):
    """new java.math.BigDecimal(s).setScale(scale, HALF_UP), NULL past `precision` digits; the unscaled value."""
    if any(b >= 0x80 for b in s.encode("utf-8")):
        return AMBIGUOUS, None
    m = _DECIMAL.fullmatch(s)
    if not m:
        return NULL, None
    if m.group(1) is not None and abs(int(m.group(1))) > MAX_EXPONENT:
        return AMBIGUOUS, None
    d = decimal.Decimal(s)  # exact: the constructor keeps every digit
    if d.is_zero():
        return VALUE, 0
    if d.adjusted() >= precision - scale:  # |d| >= 10^(precision - scale): more than `precision` digits at this scale
        return NULL, None
    q = d.quantize(decimal.Decimal(1).scaleb(-scale), context=_DEC_CTX)
    unscaled = int(q.scaleb(scale, context=_DEC_CTX))
    if abs(unscaled) >= 10 ** precision:
        return NULL, None
    return VALUE, unscaled


_FIELD_WIDTH = {"yyyy": 4, "MM": 2, "dd": 2, "HH": 2, "mm": 2, "ss": 2}


def mask_elements(mask):
    """The mask as [("lit", byte) | ("field", name)]; ValueError outside the supported alphabet."""
    out, seen, i = [], set(), 0
    while i < len(mask):
        c = mask[i]
        if c == "'":
            j = i + 1
            if mask[j:j + 1] == "'":
                out.append(("lit", ord("'")))
                i += 2
                continue
            text = ""
            while True:
                if j >= len(mask):
                    raise ValueError("unterminated quote")
                if mask[j] == "'":
                    if mask[j + 1:j + 2] == "'":
                        text += "'"
                        j += 2
                        continue
                    break
                text += mask[j]
                j += 1
            out += [("lit", b) for b in text.encode("utf-8")]
            i = j + 1
        elif c.isascii() and c.isalpha():
            j = i
            while j < len(mask) and mask[j] == c:
                j += 1
            name = mask[i:j]
            if name not in _FIELD_WIDTH or name in seen or (out and out[-1][0] == "field"):
                raise ValueError("unsupported mask %r" % mask)
            seen.add(name)
            out.append(("field", name))
            i = j
        elif c.isascii():
            out.append(("lit", ord(c)))
            i += 1
        else:
            raise ValueError("non-ASCII literal")
    return out


_NUMBER = re.compile(rb"([ \t]*)(-?)([0-9]+)")
_EPOCH = datetime.datetime(1970, 1, 1)


def cast_timestamp(mask, s):
    """unix_timestamp(s, mask) in microseconds: the value of a strict in-range cell, NULL when SimpleDateFormat's walk
    fails, AMBIGUOUS otherwise."""
    b = s.encode("utf-8")
    if any(x >= 0x80 for x in b):
        return AMBIGUOUS, None
    pos, strict = 0, True
    got = {"yyyy": 1970, "MM": 1, "dd": 1, "HH": 0, "mm": 0, "ss": 0}
    for kind, arg in mask_elements(mask):
        if kind == "lit":
            if pos >= len(b) or b[pos] != arg:
                return NULL, None
            pos += 1
            continue
        m = _NUMBER.match(b, pos)
        if not m:
            return NULL, None
        pos = m.end()
        if b[pos:pos + 1] in (b"E", b"e"):
            return AMBIGUOUS, None
        if m.group(1) or m.group(2) or len(m.group(3)) != _FIELD_WIDTH[arg]:
            strict = False
        got[arg] = int(m.group(3))
    if pos != len(b) or not strict or not 1583 <= got["yyyy"] <= 9999:
        return AMBIGUOUS, None
    try:
        t = datetime.datetime(got["yyyy"], got["MM"], got["dd"], got["HH"], got["mm"], got["ss"])
    except ValueError:
        return AMBIGUOUS, None
    return VALUE, ((t - _EPOCH) // datetime.timedelta(seconds=1)) * 1000000


def kleene_and(clauses):
    if any(c is False for c in clauses):
        return False
    if any(c is None for c in clauses):
        return None
    return True


def cell_cast(d, cell):
    """(class, value) of a non-NULL cell under definition d (strings cast to themselves)."""
    if d["type"] == "int":
        return cast_int(cell)
    if d["type"] == "decimal":
        return cast_decimal(cell, d["precision"], d["scale"])
    if d["type"] == "timestamp":
        return cast_timestamp(d["mask"], cell)
    return VALUE, cell


def row_clauses(d, cell, cls, value):
    """The reference's clauses for definition d on one cell (toCNF :225-281), each True / False / None."""
    out = []
    null = cell is None
    if not d.get("isNullable", True):
        out.append(not null)
    t = d["type"]
    if t == "string":
        if d.get("minLength") is not None:
            out.append(null or len(cell) >= d["minLength"])
        if d.get("maxLength") is not None:
            out.append(null or len(cell) <= d["maxLength"])
        if d.get("matches") is not None:
            if null:
                out.append(True)
            else:
                m = re.search(d["matches"], cell)
                out.append(m is not None and m.group(0) != "")
    else:
        ok = (not null) and cls == VALUE
        out.append(null or ok)
        if t == "int":
            if d.get("minValue") is not None:  # `colIsNull.isNull or cast >= min`: FALSE OR (NULL when no value)
                out.append(value >= d["minValue"] if ok else None)
            if d.get("maxValue") is not None:
                out.append(True if null else (value <= d["maxValue"] if ok else None))
    return out


class ModelResult:
    pass


def validate(columns, rows, schema):
    """The validator over rows (lists of str | None): verdicts, the valid rows (schema columns cast; decimals as
    unscaled ints, timestamps as microseconds) and the invalid rows, in row order, with ambiguous cells cast to NULL
    (the ambiguous="invalid" policy; num_ambiguous counts their rows, first_ambiguous names the first definition's
    column)."""
    r = ModelResult()
    r.verdicts, r.valid, r.invalid, r.num_unknown, r.num_ambiguous = [], [], [], 0, 0
    amb_defs = set()
    for row in rows:
        clauses, casts, amb = [], {}, False
        for k, d in enumerate(schema):
            cell = row[columns.index(d["name"])]
            cls, value = (NULL, None) if cell is None else cell_cast(d, cell)
            if cls == AMBIGUOUS:
                amb = True
                amb_defs.add(k)
            if d["type"] != "string":
                casts[d["name"]] = value if cls == VALUE else None
            clauses += row_clauses(d, cell, cls, value)
        v = kleene_and(clauses)
        r.verdicts.append(v)
        r.num_ambiguous += amb
        if v is True:
            r.valid.append([casts.get(c, cell) for c, cell in zip(columns, row)])
        elif v is False:
            r.invalid.append(list(row))
        else:
            r.num_unknown += 1
    r.first_ambiguous = schema[min(amb_defs)]["name"] if amb_defs else None
    return r
