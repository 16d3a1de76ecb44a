"""128-bit decimal columns (DQ_TYPE_DECIMAL128, precision 19..38) on the host: ingest, the shared arithmetic of
csrc/dq_dec128.h through its C entry points (dq_dec128_to_double, dq_spark_hash64), the wide Sum / Mean state
algebra (dq_state_merge / dq_state_fold, states.py) and a stand-alone AddressSanitizer + UBSan program over the
header. Expected values come from tests/decimal128_model.py (Python int / decimal / fractions / xxhash). No GPU."""
import ctypes
import decimal
import os
import subprocess
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import decimal128_model as M
from deequ_amd import native as N
from deequ_amd.states import MeanState, SumState, state_from_native
from deequ_amd.table import ChunkedTable, Table, column_to_arrow, dec128_int

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WIDE = pa.decimal128(38, 18)
VALUES = [Decimal("123.45"), None, Decimal("-99"), Decimal("678.000000000000000001"),
          Decimal("99999999999999999999.999999999999999999"), Decimal("-99999999999999999999.999999999999999999"),
          None, Decimal(0), Decimal("-0.000000000000000001")]


def unscaled(col):
    exact = decimal.Context(prec=60)
    return [None if v is None else int(v.scaleb(col.decimal_scale, context=exact)) for v in col.to_pylist()]


# ---- ingest ----------------------------------------------------------------------------------------------------
def test_model_conversion_agrees_with_exact_rationals():
    for v, s in M.hard_cases()[::7] + M.random_cases(500, 3):
        assert M.to_double(v, s) == float(Fraction(v, 10 ** s)), (v, s)


def test_default_still_raises_and_names_the_option():
    t = pa.table({"big": pa.array([Decimal(1)], pa.decimal128(30, 2))})
    with pytest.raises(ValueError, match="exceeds") as e:
        Table.from_arrow(t)
    assert "wide_decimals" in str(e.value)


def test_from_arrow_wide_takes_the_cells_and_zeroes_null_slots():
    t = Table.from_arrow(pa.table({"x": pa.array(VALUES, WIDE)}), wide_decimals=True)
    c = t["x"]
    assert c.spark_type == N.TYPE_DECIMAL128 and c.type_name == "DecimalType(38,18)"
    assert (c.decimal_precision, c.decimal_scale) == (38, 18) and c.values.dtype.itemsize == 16
    assert c.to_pylist() == VALUES
    assert all(isinstance(v, Decimal) for v in c.to_pylist() if v is not None)
    assert [dec128_int(c.values[i]) for i in (1, 6)] == [0, 0]  # NULL slots
    assert c.value_at(0) == Decimal("123.45") and c.cells_at([2, 1]) == [Decimal(-99), None]
    assert c.is_numeric()
    # the bytes are Arrow's: little-endian two's complement
    assert c.values.tobytes()[16 * 2:16 * 3] == M.cell(-99 * 10 ** 18)


@pytest.mark.parametrize("start,length", [(1, 5), (3, 3), (8, 1), (2, 0)])
def test_from_arrow_sliced_and_chunked(start, length):
    arr = pa.array(VALUES, WIDE)
    t = Table.from_arrow(pa.table({"x": arr.slice(start, length)}), wide_decimals=True)
    assert t["x"].to_pylist() == VALUES[start:start + length]
    chunked = pa.chunked_array([arr.slice(0, 4), arr.slice(4, 1), arr.slice(5)])
    t = Table.from_arrow(pa.table({"x": chunked}), wide_decimals=True)
    assert t["x"].to_pylist() == VALUES


def test_from_parquet_and_to_arrow_round_trip(tmp_path):
    p = str(tmp_path / "w.parquet")
    src = pa.table({"x": pa.array(VALUES, WIDE), "k": pa.array(range(len(VALUES)), pa.int64())})
    pq.write_table(src, p, row_group_size=4)
    with pytest.raises(ValueError, match="wide_decimals"):
        Table.from_parquet(p)
    t = Table.from_parquet(p, wide_decimals=True)
    assert t["x"].to_pylist() == VALUES and t["k"].spark_type == N.TYPE_LONG
    back = column_to_arrow(t["x"], pa)
    assert back.type == WIDE and back.to_pylist() == VALUES
    assert Table.from_arrow(pa.table({"x": back}), wide_decimals=True)["x"].to_pylist() == VALUES


def test_narrow_decimals_stay_long_backed():
    t = Table.from_arrow(pa.table({"d": pa.array([Decimal("12.50")], pa.decimal128(18, 2))}), wide_decimals=True)
    assert t["d"].spark_type == N.TYPE_DECIMAL and t["d"].values.dtype == np.int64


def test_from_rows_with_explicit_precision():
    rows = [(Decimal("123.45"),), (99,), ("678",), (None,), (-(10 ** 20 - 1),)]
    t = Table.from_rows(rows, ["x"], ["decimal(38,18)"])
    c = t["x"]
    assert c.spark_type == N.TYPE_DECIMAL128 and c.type_name == "DecimalType(38,18)"
    assert unscaled(c) == [12345 * 10 ** 16, 99 * 10 ** 18, 678 * 10 ** 18, None, -(10 ** 20 - 1) * 10 ** 18]
    t = Table.from_pydict({"x": [1, None]}, types={"x": "DecimalType(20,0)"})
    assert t["x"].type_name == "DecimalType(20,0)" and t["x"].to_pylist() == [Decimal(1), None]
    for bad in (10 ** 20, Decimal("0.0000000000000000001"), "abc", 1.5):
        with pytest.raises(ValueError):
            Table.from_rows([(bad,)], ["x"], ["decimal(38,18)"])
    # a bare "decimal" infers as before (precision <= 18, long-backed)
    t = Table.from_rows([(Decimal("1.5"),)], ["x"], ["decimal"])
    assert t["x"].spark_type == N.TYPE_DECIMAL
    assert Table.from_rows([(Decimal("1.5"),)], ["x"], ["decimal(10,2)"])["x"].spark_type == N.TYPE_DECIMAL


def test_chunked_table_and_row_subsets_carry_the_width():
    t = Table.from_rows([(v,) for v in VALUES], ["x"], ["decimal(38,18)"])
    a = t.select_rows(np.arange(len(VALUES)) < 4)
    b = t.select_rows(np.arange(len(VALUES)) >= 4)
    assert a["x"].to_pylist() + b["x"].to_pylist() == VALUES
    whole = ChunkedTable([a, b]).concat(["x"])
    assert whole["x"].spark_type == N.TYPE_DECIMAL128 and whole["x"].to_pylist() == VALUES
    nat = t["x"].native()
    assert (nat.spark_type, nat.decimal_precision, nat.decimal_scale, nat.length) == (12, 38, 18, len(VALUES))


# ---- dq_dec128_to_double ---------------------------------------------------------------------------------------
def test_to_double_hard_cases_bit_exact():
    cases = M.hard_cases()
    assert len(cases) > 600
    for v, s in cases:
        assert M.bits(N.dec128_to_double(v, s)) == M.bits(M.to_double(v, s)), (v, s)


def test_to_double_20000_random_cases_bit_exact():
    lib = N.load_library()
    for v, s in M.random_cases(20000, 20260101):
        got = lib.dq_dec128_to_double(M.cell(v), s)
        assert M.bits(got) == M.bits(M.to_double(v, s)), (v, s)


def test_to_double_is_exported_and_guards_its_arguments():
    assert "dq_dec128_to_double" in N.EXPORTED_SYMBOLS
    lib = N.load_library()
    assert np.isnan(lib.dq_dec128_to_double(M.cell(1), 39)) and np.isnan(lib.dq_dec128_to_double(None, 0))
    assert lib.dq_abi_version() == 2 and ctypes.sizeof(N.DqState) == 424


# ---- dq_spark_hash64 -------------------------------------------------------------------------------------------
def test_java_byte_forms():
    assert [M.java_bytes(v).hex() for v in (0, -1, 128, -128, -129, 127)] == ["00", "ff", "0080", "80", "ff7f", "7f"]


def test_spark_hash_byte_length_edges_and_random_values():
    for v in M.HASH_EDGES + M.hard_values() + M.random_values(2000, 77, 127):
        assert N.spark_hash64(N.TYPE_DECIMAL128, v) == M.spark_hash(v), v


# ---- dq_state_merge / dq_state_fold ------------------------------------------------------------------------------
def wide_state(kind, total, scale, count=1):
    st = N.DqState()
    st.kind, st.present = kind, 1
    f = st.u.mean if kind == N.OP_MEAN else st.u.dbl
    f.exact, f.wscale = 2, scale
    for i, limb in enumerate(N.wide_sum_limbs(total)):
        f.wsum[i] = limb
    over = abs(total) >= M.LIMIT
    f.woverflow = int(over)
    if kind == N.OP_MEAN:
        f.sum, f.count = (float("nan") if over else M.to_double(total, scale)), count
    else:
        f.value = float("nan") if over else M.to_double(total, scale)
    return st


def total_of(st):
    f = st.u.mean if st.kind == N.OP_MEAN else st.u.dbl
    assert f.exact == 2
    return N.wide_sum_value(f.wsum), f.wscale, f.woverflow, (f.sum if st.kind == N.OP_MEAN else f.value)


CARRIES = [((1 << 64) - 1, 1), (1 << 64, -1), ((1 << 127) - 1, (1 << 127) - 1), (-(1 << 127), -(1 << 127)),
           (-(1 << 128), (1 << 128) + 5), (M.LIMIT - 1, -(M.LIMIT - 1)), (-1, 1), ((1 << 128) - 1, 1),
           (3 * 10 ** 37, 4 * 10 ** 37 + 7)]


@pytest.mark.parametrize("kind", [N.OP_SUM, N.OP_MEAN])
def test_merge_carries_limbs_in_both_directions(kind):
    for a, b in CARRIES:
        out = N.merge_states(wide_state(kind, a, 18, 2), wide_state(kind, b, 18, 3))
        tot, scale, over, val = total_of(out)
        assert (tot, scale) == (a + b, 18), (a, b)
        assert over == int(abs(a + b) >= M.LIMIT)
        if not over:
            assert M.bits(val) == M.bits(M.to_double(a + b, 18)), (a, b)
        if kind == N.OP_MEAN:
            assert out.u.mean.count == 5


@pytest.mark.parametrize("kind", [N.OP_SUM, N.OP_MEAN])
def test_fold_of_three_parts_equals_the_single_total(kind):
    parts = [M.LIMIT - 1, 12345678901234567890123, -(M.LIMIT - 1)]
    buf = b"".join(bytes(wide_state(kind, p, 18, 7)) for p in parts)
    out = N.fold_states(buf, 3, 1)[0]
    tot, _, over, val = total_of(out)
    assert tot == sum(parts) and not over and M.bits(val) == M.bits(M.to_double(sum(parts), 18))
    # the doubles of the parts do not add up to it: the merge must not add rounded values
    assert sum(M.to_double(p, 18) for p in parts) != val
    st = state_from_native(out)
    assert st.wide == (sum(parts), 18) and st.metricValue() == (val / 21 if kind == N.OP_MEAN else val)


@pytest.mark.parametrize("kind", [N.OP_SUM, N.OP_MEAN])
def test_total_of_ten_to_the_38_is_flagged(kind):
    from deequ_amd.metrics import MetricCalculationRuntimeException
    for a, b in ((M.LIMIT - 1, 1), (-(M.LIMIT - 1), -1), (9 * 10 ** 37, 2 * 9 * 10 ** 37)):
        out = N.merge_states(wide_state(kind, a, 0), wide_state(kind, b, 0))
        tot, _, over, val = total_of(out)
        assert tot == a + b and over == 1 and np.isnan(val)
        with pytest.raises(MetricCalculationRuntimeException, match="overflow"):
            state_from_native(out).metricValue()
    ok = N.merge_states(wide_state(kind, M.LIMIT - 2, 0), wide_state(kind, 1, 0))
    assert total_of(ok)[2] == 0 and state_from_native(ok).metricValue() is not None


def test_python_states_merge_like_the_library():
    a, b = SumState(0.0, wide=(M.LIMIT - 1, 18)), SumState(0.0, wide=(-(M.LIMIT - 1) + 5, 18))
    assert a.sum(b).wide == (5, 18) and a.sum(b).metricValue() == 5e-18
    m = MeanState(1.0, 2, wide=(10 ** 18, 18)).sum(MeanState(2.0, 2, wide=(2 * 10 ** 18, 18)))
    assert (m.wide, m.count, m.metricValue()) == ((3 * 10 ** 18, 18), 4, 0.75)
    # a state without the exact total (loaded from a provider) merges as the reference's doubles
    assert SumState(1.5).sum(SumState(2.0, wide=(2, 0))).metricValue() == 3.5
    # existing long partials are untouched
    assert SumState(3.0, 3).sum(SumState(4.0, 4)).exact == 7


# ---- the header under AddressSanitizer + UBSan, stand-alone --------------------------------------------------------
def test_header_under_asan_ubsan(tmp_path):
    """csrc/dq_dec128.h compiled into tests/sanitize/dec128_checks.cpp (its own main) with the host compiler's
    sanitizers and run directly: the hard cases and 20 000 random ones against the model, plus the 192-bit adds."""
    build = os.path.join(HERE, "sanitize", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "dec128_checks")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-DDQ_HOST_ONLY", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", exe,
                    os.path.join(HERE, "sanitize", "dec128_checks.cpp")], check=True)
    cases = M.hard_cases() + [(v, 0) for v in M.HASH_EDGES] + M.random_cases(20000, 11)
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for v, s in cases:
            c = M.cell(v)
            f.write("%x %x %d %x %x %x\n" % (int.from_bytes(c[:8], "little"), int.from_bytes(c[8:], "little"), s,
                                             M.bits(M.to_double(v, s)), M.to_long(v, s) & (2 ** 64 - 1),
                                             M.spark_hash(v) & (2 ** 64 - 1)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, \
        (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "dec128_checks: ok %d cases" % len(cases) in p.stdout


# ---- exact, order-free StandardDeviation states -------------------------------------------------------------------
def stddev_state(values, scale):
    from deequ_amd.states import StandardDeviationState
    n, avg, m2 = M.moments(values, scale)
    return StandardDeviationState(n, avg, m2, sums=M.exact_sums(values, scale))


def test_standard_deviation_states_with_exact_sums_merge_to_the_whole_tables_bits():
    values = M.random_values(600, 13, 100) + [7 * 10 ** 18] * 5
    whole = stddev_state(values, 18)
    assert (whole.n, whole.avg, whole.m2) == M.moments(values, 18)  # the exact moments, rounded once
    for cuts in ([0, 1, 64, 300, 605], [0, 604, 605], [0, 200, 400, 605]):
        parts = [stddev_state(values[a:b], 18) for a, b in zip(cuts, cuts[1:])]
        acc = parts[0]
        for p in parts[1:]:
            acc = acc.sum(p)
        assert (acc.n, M.bits(acc.avg), M.bits(acc.m2)) == (whole.n, M.bits(whole.avg), M.bits(whole.m2)), cuts
        assert M.bits(acc.metricValue()) == M.bits(whole.metricValue())
    const = stddev_state([9 * 10 ** 37] * 3, 0)
    assert const.m2 == 0.0 and const.metricValue() == 0.0 and const.avg == 9e37
    # the library's merge adds the same integers
    def native(values):
        st = N.DqState()
        st.kind, st.present = N.OP_STANDARD_DEVIATION, 1
        n, avg, m2 = M.moments(values, 18)
        st.u.stddev.n, st.u.stddev.avg, st.u.stddev.m2, st.u.stddev.exact = n, avg, m2, 1
        s1, s2 = M.exact_sums(values, 18)
        for i, x in enumerate(N.value_limbs(s1, 6)):
            st.u.stddev.xs1[i] = x
        for i, x in enumerate(N.value_limbs(s2, 11)):
            st.u.stddev.xs2[i] = x
        return st
    out = state_from_native(N.merge_states(native(values[:100]), native(values[100:])))
    assert out.sums == whole.sums and (out.avg, out.m2) == (whole.avg, whole.m2)
    plain = N.DqState()
    plain.kind, plain.present = N.OP_STANDARD_DEVIATION, 1
    plain.u.stddev.n, plain.u.stddev.avg, plain.u.stddev.m2 = 2.0, 1.0, 0.5
    assert N.merge_states(native(values[:100]), plain).u.stddev.exact == 0  # one side without sums: fp64 merge
