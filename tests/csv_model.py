"""A plain model of the device CSV reader's contract: the four refusal rules and a state-machine
reader of the record / field semantics, over a file's bytes. No GPU, no native code: tests compare it with csv.reader
(test_csv_model.py) and the device with it (test_gpu_csv.py)."""
import csv
import io
import random

QUOTE_IN_FIELD, TEXT_AFTER_QUOTE, LONE_CR, UNTERMINATED_QUOTE = 1, 2, 3, 4

# the raw generator of the issue: files of 0-14 tokens of this alphabet
ALPHABET = [",", ",", '"', '"', "\n", "\n", "\r\n", "\r", "1", "a", ".", " ", "-", "é"]


def random_files(count, seed=7):
    """`count` random files (bytes) of 0-14 tokens of ALPHABET, drawn with random.Random(seed)."""
    rng = random.Random(seed)
    for _ in range(count):
        yield "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 14))).encode("utf-8")


def refusal(data):
    """None for an accepted file, else (kind, byte offset) of the first refusal: the smallest offset, the lower kind on
    a tie. q = the quotes before byte i; a byte is outside quotes when q is even."""
    n, q, found, last_quote = len(data), 0, [], None
    for i in range(n):
        c = data[i:i + 1]
        if c == b'"':
            if q % 2 == 0:  # an opening quote
                if i > 0 and data[i - 1:i] not in (b",", b"\n", b'"'):
                    found.append((i, QUOTE_IN_FIELD))
            else:  # a closing quote
                if not (i + 1 == n or data[i + 1:i + 2] in (b",", b"\n", b'"') or data[i + 1:i + 3] == b"\r\n"):
                    found.append((i, TEXT_AFTER_QUOTE))
            last_quote = i
            q += 1
        elif c == b"\r" and q % 2 == 0 and data[i + 1:i + 2] != b"\n":
            found.append((i, LONE_CR))
    if q % 2:
        found.append((last_quote, UNTERMINATED_QUOTE))  # the unpaired quote is the file's last
    if not found:
        return None
    offset, kind = min(found)
    return kind, offset


def records(data):
    """The records of an accepted file as csv.reader gives them: a list of fields (str) per record, [] for a record of
    zero bytes. Outside quotes ',' ends a field and LF or CR LF a record; a field whose first byte is '"' is quoted,
    its value the bytes between the enclosing quotes with "" collapsed; the bytes after the last terminator are a
    record when there is at least one."""
    out, n, start, q = [], len(data), 0, 0
    bounds = []  # (start, end) of the records
    for i in range(n):
        c = data[i:i + 1]
        if c == b'"':
            q += 1
        elif c == b"\n" and q % 2 == 0:
            bounds.append((start, i - 1 if i > start and data[i - 1:i] == b"\r" else i))
            start = i + 1
    if start < n:
        bounds.append((start, n))
    for s, e in bounds:
        rec = data[s:e]
        if not rec:
            out.append([])
            continue
        fields, at, inside = [], 0, False
        for i in range(len(rec) + 1):
            c = rec[i:i + 1]
            if c == b'"':
                inside = not inside
            if i == len(rec) or (c == b"," and not inside):
                f = rec[at:i]
                if f[:1] == b'"':
                    f = f[1:-1].replace(b'""', b'"')
                fields.append(f.decode("utf-8"))
                at = i + 1
        out.append(fields)
    return out


def reader_records(data):
    """csv.reader's records of the same bytes (the host path's reading: text mode, newline="")."""
    return list(csv.reader(io.StringIO(data.decode("utf-8"), newline="")))


# ---- typing ---------------------------------------------------------------------------------------------------------
INT, LONG, DOUBLE, BOOLEAN, STRING = 1, 2, 4, 8, 16  # native.CSV_CLASS_*


def field_class(x):
    """The class of an ASCII field that does not end in LF, written without `re`, `int` or `float`: what the kernel's
    state machine computes."""
    body = x[1:] if x[:1] in ("+", "-") else x
    digits = "0123456789"
    if body and all(c in digits for c in body):
        v, neg = 0, x[0] == "-"
        for c in body:
            v = v * 10 + digits.index(c)
        if v < 2 ** 31 or (neg and v == 2 ** 31):
            return INT
        if v < 2 ** 63 or (neg and v == 2 ** 63):
            return LONG
        return DOUBLE
    mant, exp = body, None
    for k, c in enumerate(body):
        if c in "eE":
            mant, exp = body[:k], body[k + 1:]
            break
    if exp is not None:
        e = exp[1:] if exp[:1] in ("+", "-") else exp
        exp_ok = bool(e) and all(c in digits for c in e)
    else:
        exp_ok = True
    whole, dot, frac = mant.partition(".")
    mant_ok = all(c in digits for c in whole + frac) and (bool(whole) or (bool(dot) and bool(frac)))
    if mant_ok and exp_ok:
        return DOUBLE
    if x in ("NaN", "Infinity", "-Infinity"):
        return DOUBLE
    if x.lower() in ("true", "false"):
        return BOOLEAN
    return STRING


def type_of_classes(classes):
    """The column's class (INT / LONG / DOUBLE / BOOLEAN / STRING) from the OR of its fields' classes."""
    if classes and not classes & ~(INT | LONG | DOUBLE):
        return DOUBLE if classes & DOUBLE else LONG if classes & LONG else INT
    return BOOLEAN if classes == BOOLEAN else STRING
