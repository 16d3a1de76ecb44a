"""The contract of the device CSV reader, checked on the CPU: the refusal rules and the record / field semantics
(csv_model.py) against csv.reader, the class-to-type fold and the per-field classes against the host path's
_csv_infer / _csv_field_type, and the public surface (Table.from_csv(device=...), the C-ABI entry points)."""
import inspect
import itertools

import deequ_amd.native as N
from deequ_amd import table as T
from deequ_amd.table import Table

import csv_model as M

TYPE_OF = {M.INT: N.TYPE_INT, M.LONG: N.TYPE_LONG, M.DOUBLE: N.TYPE_DOUBLE, M.BOOLEAN: N.TYPE_BOOLEAN,
           M.STRING: N.TYPE_STRING}
SAMPLE = {M.INT: "7", M.LONG: "3000000000", M.DOUBLE: "1.5", M.BOOLEAN: "true", M.STRING: "x"}

# every literal the contract names, and the neighbours where a parser goes wrong
FIELDS = [
    "0", "7", "+5", "-0", "00012", "2147483647", "2147483648", "-2147483648", "-2147483649", "+2147483648",
    "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809",
    "00000000000000000000000000001", "99999999999999999999", "-99999999999999999999", "1" + "0" * 30,
    "1.", ".5", "1.e3", "-.5e-3", "1e400", "1E5", "1e+5", "1e-5", "+.5", "-1.", "1.5e", "1e", "e5", ".", "+", "-", "+.", ".e3",
    "1..2", "1.2.3", "1e5.0", "1e5e5", "--1", "+-1", "1-", "1+", "1.5d", "1.5D", "1.5f", "1.5F", "1d", "1_0", " 1", "1 ",
    "0x10", "0X1p3", "1,5", "١٢", "NaN", "nan", "NAN", "-NaN", "+NaN", "Infinity", "-Infinity", "+Infinity", "infinity",
    "inf", "-inf", "Inf", "true", "false", "tRuE", "FALSE", "True", "tru", "truee", "falsee", " true", "yes", "t", "",
    "a", "abc", '"', 'a"b', "1\r", "\r", "1\t", "\t1", "1\x0b", "1\x0c", "1\x1c", "1e5 ", "0.0", "-0.0", "0e0", "00.00",
]


def test_model_equals_csv_reader_on_every_accepted_random_file():
    refused = accepted = 0
    for data in M.random_files(200_000):
        if M.refusal(data) is not None:
            refused += 1
            continue
        accepted += 1
        assert M.records(data) == M.reader_records(data), data
    assert (refused, accepted) == (127_505, 72_495)


def test_refusal_kinds_and_offsets():
    assert M.refusal(b'a,b\n1,"x"\n') is None
    assert M.refusal(b'a,b"c\n') == (M.QUOTE_IN_FIELD, 3)
    assert M.refusal(b'a,"b"c\n') == (M.TEXT_AFTER_QUOTE, 4)
    assert M.refusal(b'a\rb\n') == (M.LONE_CR, 1)
    assert M.refusal(b'a,"bc\n') == (M.UNTERMINATED_QUOTE, 2)
    assert M.refusal(b'a,"b""c\n') == (M.UNTERMINATED_QUOTE, 5)  # the unpaired quote is the file's last
    assert M.refusal(b'a\rb,c"d\n') == (M.LONE_CR, 1)  # the earlier of two
    assert M.refusal(b'a"') == (M.QUOTE_IN_FIELD, 1)  # a tie: the lower kind
    assert M.refusal(b'"a"\r') == (M.TEXT_AFTER_QUOTE, 2)
    assert M.refusal(b'"a"\r\n"b"') is None
    assert M.refusal(b'"a\rb"\n') is None


def test_class_fold_equals_csv_infer_over_all_multisets():
    classes = (M.INT, M.LONG, M.DOUBLE, M.BOOLEAN, M.STRING)
    assert T._csv_infer([]) == N.TYPE_STRING == TYPE_OF[M.type_of_classes(0)] == T._csv_type_of_classes(0)
    for k in range(1, 5):
        for multiset in itertools.combinations_with_replacement(classes, k):
            union = 0
            for c in multiset:
                union |= c
            for order in set(itertools.permutations(multiset)):
                expect = T._csv_infer([None] + [SAMPLE[c] for c in order])
                assert TYPE_OF[M.type_of_classes(union)] == expect, order
                assert T._csv_type_of_classes(union) == expect, order


def test_field_classes_equal_csv_field_type():
    assert len(set(FIELDS)) == len(FIELDS)
    for x in FIELDS:
        if x == "" or any(ord(c) >= 0x80 for c in x) or x.endswith("\n"):
            continue  # NULL, or ambiguous: the host decides those
        assert TYPE_OF[M.field_class(x)] == T._csv_field_type(x), x
    for named in ("+5", "-0", "00012", "1.", ".5", "1.e3", "-.5e-3", "1e400", "NaN", "Infinity", "-Infinity", "tRuE", "nan",
                  "inf", "+Infinity", "1.5d", "1_0", " 1", "0x10"):
        assert named in FIELDS
    for x in ("nan", "inf", "+Infinity", "1.5d", "1_0", " 1", "0x10"):
        assert M.field_class(x) == M.STRING, x


def test_from_csv_takes_a_device():
    p = inspect.signature(Table.from_csv).parameters
    assert list(p) == ["path", "header", "infer_schema", "device"]
    assert p["device"].default is None and p["header"].default is True and p["infer_schema"].default is True


def test_csv_entry_points_are_declared_and_exported():
    names = {"dq_csv_index", "dq_csv_field", "dq_csv_column", "dq_csv_free"}
    assert names <= set(N.EXPORTED_SYMBOLS)
    lib = N.load_library()
    for s in names:
        assert hasattr(lib, s), s
    assert N.CSV_TILE_BYTES == 16384 and N.CSV_KERNELS[0] == "csv_quotes" and len(N.CSV_KERNELS) == 5
    assert (N.CSV_CLASS_INT, N.CSV_CLASS_LONG, N.CSV_CLASS_DOUBLE, N.CSV_CLASS_BOOLEAN, N.CSV_CLASS_STRING) == \
        (M.INT, M.LONG, M.DOUBLE, M.BOOLEAN, M.STRING)
    assert lib.dq_abi_version() == 2


def test_header_record_is_read_as_the_device_reads_records(tmp_path):
    first = T._csv_first_record
    assert first(b"a,b\n1,2\n") == (["a", "b"], True)
    assert first(b'a,"b,""c"""\r\nx') == (["a", 'b,"c"'], True)
    assert first(b'"a\nb",c') == (["a\nb", "c"], False)
    assert first(b"\nx") == ([], True)
    assert first(b"a,") == (["a", ""], False)
    assert first("﻿id,é\n".encode("utf-8")) == (["﻿id", "é"], True)


def test_device_path_refuses_without_a_gpu_call(tmp_path):
    import pytest
    empty = tmp_path / "empty.csv"
    empty.write_bytes(b"")
    with pytest.raises(ValueError, match="empty file"):
        Table.from_csv(str(empty), device=0)
