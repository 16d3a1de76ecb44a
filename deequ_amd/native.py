"""ctypes binding of libdq.so (include/dq.h) — the same C-ABI a JVM host binds over JNI.

The library is loaded from the package directory (built in-tree by __graft_entry__.build()).
There is no CPU fallback: if the library or a GPU is missing, operations raise.
"""
import ctypes
import sys
import os
import threading

import numpy as np

# Hardware queues per process. A run drives up to ~7 streams at once (the main context, helper contexts for the
# second row chunk, the early KLL pass, the pass-3 histograms, the groupings and AnalysisRunBuilder.runAsync, plus
# torch's); with HIP's default of 4 queues, streams share a queue and one stream's kernels wait behind another's (the
# C5 step's histograms queued ~60 ms behind the text grouping). Read by the HIP runtime when it initialises (the first
# HIP call of the process): set here, before that, unless the user set it. C5 step: 4 queues 159-173 ms, 8 queues
# 143-145 ms (profiles/r06/c5_hw_queues_ab_r06v.txt).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DQ_LIBRARY") or os.path.join(_HERE, "libdq.so")

# ---- constants mirrored from include/dq.h -------------------------------------------------------
DQ_OK = 0
STATUS_NAMES = {0: "DQ_OK", -1: "DQ_ERR_INVALID_ARGUMENT", -2: "DQ_ERR_UNSUPPORTED", -3: "DQ_ERR_DEVICE",
                -4: "DQ_ERR_OUT_OF_MEMORY", -5: "DQ_ERR_NO_DEVICE", -6: "DQ_ERR_PREDICATE",
                -7: "DQ_ERR_ALIGNMENT"}

TYPE_BOOLEAN, TYPE_BYTE, TYPE_SHORT, TYPE_INT, TYPE_LONG, TYPE_FLOAT, TYPE_DOUBLE, TYPE_STRING, \
    TYPE_DATE, TYPE_TIMESTAMP, TYPE_DECIMAL = range(1, 12)
TYPE_DECIMAL128 = 12  # 16-byte unscaled cells, precision 19..38 (DQ_TYPE_DECIMAL128)
DEC128_TILE_ROWS = 1024  # rows one workgroup of the decimal128 scan takes per step (dq_internal.h kD128TileRows)
CSV_TILE_BYTES = 16384  # bytes one workgroup of the CSV tokenizer takes (dq.h DQ_CSV_TILE_BYTES)
CSV_CLASS_INT, CSV_CLASS_LONG, CSV_CLASS_DOUBLE, CSV_CLASS_BOOLEAN, CSV_CLASS_STRING = 1, 2, 4, 8, 16
# dq_csv_refusal, by kind
CSV_REFUSALS = {1: "a quote inside an unquoted field", 2: "text after a closing quote",
                3: "a carriage return outside quotes that no line feed follows",
                4: "an unterminated quoted field (an odd number of quotes)"}

COL_DEVICE = 0x1
COL_OFFSETS64 = 0x2  # STRING: int64 offsets (dq_frequencies only)
SCAN_OUT_DEVICE = 0x1
FREQ_INCLUDE_NULLS = 0x1
FREQ_KEYS_VALUES, FREQ_KEYS_ROWS = 0, 1
FREQ_PAIRS_DEVICE = 0x1

OP_SIZE, OP_COMPLETENESS, OP_COMPLIANCE, OP_MEAN, OP_SUM, OP_MINIMUM, OP_MAXIMUM, OP_STANDARD_DEVIATION, \
    OP_CORRELATION, OP_APPROX_COUNT_DISTINCT, OP_MIN_LENGTH, OP_MAX_LENGTH, OP_DATATYPE = range(1, 14)

# predicate opcodes
P_COL, P_CONST, P_NULL = 1, 2, 3
P_EQ, P_NE, P_LT, P_LE, P_GT, P_GE, P_EQ_NULLSAFE = 10, 11, 12, 13, 14, 15, 16
P_AND, P_OR, P_NOT, P_IS_NULL, P_IS_NOT_NULL, P_IN, P_COALESCE = 20, 21, 22, 23, 24, 25, 26
P_ADD, P_SUB, P_MUL, P_DIV, P_MOD, P_NEG = 30, 31, 32, 33, 34, 35
P_LIKE, P_LENGTH, P_CAST_DOUBLE, P_CAST_LONG, P_CAST_STRING_NUM, P_REGEX = 40, 41, 42, 43, 44, 45
P_RLIKE, P_LOWER, P_UPPER, P_TRIM, P_CASE, P_ISNAN, P_ABS, P_SUBSTR, P_YEAR, P_MONTH, P_DAY, P_NANVL = range(46, 58)
V_BOOL, V_LONG, V_DOUBLE, V_STRING = 1, 2, 3, 4

SYNTH_DYADIC, SYNTH_UNIFORM, SYNTH_NORMAL, SYNTH_INT32R, SYNTH_KEY30, SYNTH_GAUSS01, SYNTH_GAUSS_CORR = range(1, 8)
SYNTH_STR_CAT50, SYNTH_STR_BOOL, SYNTH_STR_CAT100, SYNTH_STR_INT, SYNTH_STR_DEC, SYNTH_STR_MIXNUM, SYNTH_STR_TEXT = \
    101, 102, 103, 104, 105, 106, 107

HLL_NUM_WORDS = 52

# dq_scan_kernel, in enum order
FREQ_PATHS = ("fast", "fast_narrow", "fast_done", "exact", "partitioned", "sorted", "small", "small_optimistic", "fast_spill",
              "split_buckets", "long_tuples")
SCAN_KERNELS = ("striped", "striped_heavy", "heavy8", "heavy8_full", "bits", "pred_simple", "pred_vm", "regex",
                "strings", "where_fused", "where_masks", "decimal128", "dict_counts", "dict_fold", "dict_decode",
                "filter_validity", "row_outcomes", "freq_probe")
# the dq_scan_kernel entries after them: the kernels of the device CSV reader (dq_csv_index, dq_csv_column)
CSV_KERNELS = ("csv_quotes", "csv_mark", "csv_rows", "csv_fields", "csv_column")
# the device CSV writer counts on its own (dq_csv_write_launch_count, dq_csv_write_route_count), in enum order
CSV_WRITE_KERNELS = ("csv_write_mark", "csv_write_sizes", "csv_write_write")
CSV_WRITE_ROUTES = ("stage", "direct")
CSV_WRITE_STAGE_BYTES = 31744  # dq.h DQ_CSV_WRITE_STAGE_BYTES
CSV_WRITE_TILE_ROWS = 256      # rows of one tile of the write kernel
# and after those: the kernels that bring uploaded Arrow buffers into the column layout (dq_ingest_*)
INGEST_KERNELS = ("ingest_validity", "ingest_bool", "ingest_offsets", "ingest_convert", "ingest_indices")
# dq_ingest_kind
INGEST_DECIMAL_LOW, INGEST_DECIMAL_WIDE, INGEST_TIME_MUL, INGEST_TIME_DIV = 1, 2, 3, 4

# Every symbol include/dq.h declares (checked by tests/test_native_abi.py).
EXPORTED_SYMBOLS = (
    "dq_abi_version", "dq_open", "dq_close", "dq_last_error", "dq_set_stream", "dq_synchronize", "dq_scan",
    "dq_scan_launch_count", "dq_state_merge", "dq_state_fold", "dq_hll_count", "dq_spark_hash64", "dq_frequencies",
    "dq_freq_summarize", "dq_freq_key_kind", "dq_freq_top", "dq_freq_export", "dq_freq_free", "dq_partition_keys",
    "dq_quantile_summary", "dq_quantile_summaries", "dq_kll_sketch", "dq_cast_column", "dq_synth_column", "dq_synth_freq_keys",
    "dq_synth_validity", "dq_frequencies_ex", "dq_freq_export_device", "dq_freq_from_pairs", "dq_freq_merge", "dq_freq_row_counts", "dq_synth_strings",
    "dq_freq_mutual_information", "dq_open_devices", "dq_ctx_num_devices", "dq_ctx_uses_rccl", "dq_scan_sharded",
    "dq_scan_streamed", "dq_scan_kernel_launches", "dq_freq_path_count", "dq_kll_sketch_columns",
    "dq_kll_merge_states", "dq_scratch_trim", "dq_frequencies_parts", "dq_set_priority",
    "dq_schema_validate", "dq_schema_launch_count", "dq_gather_rows", "dq_parse_int32", "dq_parse_decimal",
    "dq_parse_timestamp", "dq_split_rows", "dq_split_row_is_test", "dq_dec128_to_double",
    "dq_dict_scan", "dq_dict_counts", "dq_dict_decode", "dq_filter_validity", "dq_freq_row_bits", "dq_row_outcomes",
    "dq_freq_probe", "dq_csv_index", "dq_csv_field", "dq_csv_column", "dq_csv_free",
    "dq_csv_write_size", "dq_csv_write", "dq_csv_write_launch_count", "dq_csv_write_route_count",
    "dq_ingest_bits", "dq_ingest_offsets", "dq_ingest_convert", "dq_ingest_indices",
)


class DqColumn(ctypes.Structure):
    _fields_ = [("spark_type", ctypes.c_int32), ("flags", ctypes.c_uint32), ("length", ctypes.c_int64),
                ("values", ctypes.c_void_p), ("validity", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("decimal_precision", ctypes.c_int32), ("decimal_scale", ctypes.c_int32)]


class DqDictColumn(ctypes.Structure):
    """dq_dict_column: a dictionary-encoded STRING column (device buffers)."""
    _fields_ = [("flags", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("length", ctypes.c_int64),
                ("indices", ctypes.c_void_p), ("validity", ctypes.c_void_p), ("dictionary", DqColumn)]


ROW_NOT_NULL, ROW_PREDICATE, ROW_BITS = 1, 2, 3  # dq_row_term_kind
ROW_FILTERED_NULL = 0x1
ROW_MAX_TERMS, ROW_MAX_CHECKS = 64, 16


class DqRowTerm(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("index", ctypes.c_int32), ("where", ctypes.c_int32), ("check", ctypes.c_int32),
                ("pass_bits", ctypes.c_void_p), ("considered_bits", ctypes.c_void_p)]


class DqRowCheck(ctypes.Structure):
    _fields_ = [("pass_bits", ctypes.c_void_p), ("values", ctypes.c_void_p), ("validity", ctypes.c_void_p)]


class DqCsvResult(ctypes.Structure):
    _fields_ = [("nrows", ctypes.c_int64), ("refusal_kind", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("refusal_offset", ctypes.c_int64)]


class DqCsvColumnReport(ctypes.Structure):
    _fields_ = [("classes", ctypes.c_int32), ("reserved", ctypes.c_int32), ("valid", ctypes.c_int64),
                ("ambiguous", ctypes.c_int64), ("first_ambiguous_row", ctypes.c_int64)]


class DqIngestPiece(ctypes.Structure):
    """dq_ingest_piece: the bits of one slice of an Arrow chunk (device memory) and its place in the output."""
    _fields_ = [("src", ctypes.c_void_p), ("src_bytes", ctypes.c_int64), ("src_bit0", ctypes.c_int64),
                ("rows", ctypes.c_int64), ("out_row0", ctypes.c_int64)]


class DqIngestIndexReport(ctypes.Structure):
    _fields_ = [("bad_row", ctypes.c_int64), ("bad_index", ctypes.c_int64), ("null_rows", ctypes.c_int64)]


class DqConst(ctypes.Structure):
    _fields_ = [("tag", ctypes.c_int32), ("str_len", ctypes.c_int32), ("i64", ctypes.c_int64),
                ("f64", ctypes.c_double), ("str_offset", ctypes.c_int64)]


class DqPredicate(ctypes.Structure):
    _fields_ = [("code", ctypes.c_void_p), ("code_len", ctypes.c_int32), ("n_consts", ctypes.c_int32),
                ("consts", ctypes.c_void_p), ("strings", ctypes.c_void_p), ("strings_len", ctypes.c_int64)]


class DqOp(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("column", ctypes.c_int32 * 2), ("where", ctypes.c_int32),
                ("predicate", ctypes.c_int32)]


class _NumMatches(ctypes.Structure):
    _fields_ = [("num_matches", ctypes.c_int64)]


class _NumMatchesAndCount(ctypes.Structure):
    _fields_ = [("num_matches", ctypes.c_int64), ("count", ctypes.c_int64)]


class _Mean(ctypes.Structure):
    _fields_ = [("sum", ctypes.c_double), ("count", ctypes.c_int64), ("isum", ctypes.c_int64), ("exact", ctypes.c_int32),
                ("pad", ctypes.c_int32), ("wsum", ctypes.c_uint64 * 3), ("wscale", ctypes.c_int32),
                ("woverflow", ctypes.c_int32)]


class _Dbl(ctypes.Structure):
    _fields_ = [("value", ctypes.c_double), ("isum", ctypes.c_int64), ("exact", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("wsum", ctypes.c_uint64 * 3), ("wscale", ctypes.c_int32), ("woverflow", ctypes.c_int32)]


def wide_sum_value(limbs):
    """The exact 192-bit two's-complement sum of a DECIMAL128 Sum / Mean state (three little-endian limbs) as an int."""
    v = int(limbs[0]) | (int(limbs[1]) << 64) | (int(limbs[2]) << 128)
    return v - (1 << 192) if v >> 191 else v


def wide_sum_limbs(v):
    v &= (1 << 192) - 1
    return [v & 0xFFFFFFFFFFFFFFFF, (v >> 64) & 0xFFFFFFFFFFFFFFFF, v >> 128]


class _StdDev(ctypes.Structure):
    _fields_ = [("n", ctypes.c_double), ("avg", ctypes.c_double), ("m2", ctypes.c_double),
                ("xs1", ctypes.c_uint64 * 6), ("xs2", ctypes.c_uint64 * 11), ("exact", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


MOMENT_S1_UNIT, MOMENT_S2_UNIT = 180, 360  # xs1 counts 2^-180, xs2 counts 2^-360 (dq_dec128.h)


def limbs_value(limbs):
    """Little-endian 64-bit limbs of a two's-complement integer -> Python int."""
    n = len(limbs)
    v = sum(int(x) << (64 * i) for i, x in enumerate(limbs))
    return v - (1 << (64 * n)) if v >> (64 * n - 1) else v


def value_limbs(v, n):
    v &= (1 << (64 * n)) - 1
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


class _Corr(ctypes.Structure):
    _fields_ = [("n", ctypes.c_double), ("x_avg", ctypes.c_double), ("y_avg", ctypes.c_double),
                ("ck", ctypes.c_double), ("x_mk", ctypes.c_double), ("y_mk", ctypes.c_double)]


class _Hll(ctypes.Structure):
    _fields_ = [("words", ctypes.c_int64 * HLL_NUM_WORDS)]


class _DataType(ctypes.Structure):
    _fields_ = [("num_null", ctypes.c_int64), ("num_fractional", ctypes.c_int64), ("num_integral", ctypes.c_int64),
                ("num_boolean", ctypes.c_int64), ("num_string", ctypes.c_int64)]


class _StateUnion(ctypes.Union):
    _fields_ = [("num_matches", _NumMatches), ("num_matches_and_count", _NumMatchesAndCount), ("mean", _Mean),
                ("dbl", _Dbl), ("stddev", _StdDev), ("corr", _Corr), ("hll", _Hll), ("datatype", _DataType)]


class DqState(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("present", ctypes.c_int32), ("u", _StateUnion)]


class DqFreqSummary(ctypes.Structure):
    _fields_ = [("num_rows", ctypes.c_int64), ("num_groups", ctypes.c_int64), ("num_unique", ctypes.c_int64),
                ("entropy", ctypes.c_double), ("entropy_rows", ctypes.c_int64), ("max_count", ctypes.c_int64),
                ("null_count", ctypes.c_int64), ("entropy_fx_lo", ctypes.c_uint64), ("entropy_fx_hi", ctypes.c_int64)]


def fx_value(lo, hi):
    """The exact fixed-point entropy sum of a dq_freq_summary (2^-104 units) as a Python int."""
    return (int(hi) << 64) | int(lo)


def fx_of(t):
    """dq_common.h fx_of: a double rounded once to signed fixed point of 2^-104 units (round half up in magnitude)."""
    import struct
    u = struct.unpack("<Q", struct.pack("<d", float(t)))[0]
    e = (u >> 52) & 0x7FF
    m = (u & ((1 << 52) - 1)) | ((1 << 52) if e else 0)
    sh = (e if e else 1) - 1075 + 104
    if sh >= 0:
        v = m << min(sh, 74)
    elif sh > -64:
        v = (m + (1 << (-sh - 1))) >> -sh
    else:
        v = 0
    return -v if u >> 63 else v


def fx_to_float(v):
    """dq_common.h fx_to_double: one correctly rounded conversion (Python's int / float true division of an int by a
    power of two rounds correctly), then an exact scale."""
    return v / float(1 << 104) if abs(v) < (1 << 1000) else float("nan")


class DqFreqOptions(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32), ("weights_device", ctypes.c_uint32), ("weights", ctypes.c_void_p),
                ("key_type", ctypes.c_int32), ("pad", ctypes.c_int32)]


STATE_SIZE = ctypes.sizeof(DqState)

SCHEMA_STRING, SCHEMA_INT, SCHEMA_DECIMAL, SCHEMA_TIMESTAMP = 1, 2, 3, 4
SCHEMA_AMBIGUOUS_NULL = 0x1
PARSE_NULL, PARSE_VALUE, PARSE_AMBIGUOUS = 0, 1, 2


class DqSchemaColumn(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("column", ctypes.c_int32), ("nullable", ctypes.c_int32),
                ("has_min", ctypes.c_int32), ("has_max", ctypes.c_int32), ("precision", ctypes.c_int32),
                ("scale", ctypes.c_int32), ("program_len", ctypes.c_int32), ("min_value", ctypes.c_int64),
                ("max_value", ctypes.c_int64), ("program", ctypes.c_void_p), ("cast_values", ctypes.c_void_p),
                ("cast_validity", ctypes.c_void_p)]


class DqSchemaResult(ctypes.Structure):
    _fields_ = [("num_valid", ctypes.c_int64), ("num_invalid", ctypes.c_int64), ("num_unknown", ctypes.c_int64),
                ("num_ambiguous", ctypes.c_int64), ("first_ambiguous_column", ctypes.c_int32), ("pad", ctypes.c_int32)]


class NativeError(RuntimeError):
    """A failed libdq call (status code + dq_last_error message)."""

    def __init__(self, status, message):
        self.status = status
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), message))


_lib = None
_lib_lock = threading.Lock()


def load_library(path=None):
    """Load libdq.so and declare its prototypes. Raises if the library was not built."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise NativeError(-5, "libdq.so not found at %s: run __graft_entry__.build() (no CPU fallback exists)" % p)
        lib = ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
        c_void_p, c_int, c_int64, c_uint32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32
        sig = {
            "dq_abi_version": (c_int, []),
            "dq_open": (c_void_p, [c_int, ctypes.POINTER(c_int)]),
            "dq_close": (None, [c_void_p]),
            "dq_last_error": (ctypes.c_char_p, [c_void_p]),
            "dq_set_stream": (c_int, [c_void_p, c_void_p]),
            "dq_synchronize": (c_int, [c_void_p]),
            "dq_scratch_trim": (None, [c_void_p, c_int64]),
            "dq_set_priority": (c_int, [c_void_p, c_int]),
            "dq_frequencies_parts": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
            "dq_scan": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                c_uint32]),
            "dq_scan_launch_count": (c_int64, [c_void_p]),
            "dq_scan_kernel_launches": (c_int64, [c_void_p, ctypes.c_int32]),
            "dq_freq_path_count": (c_int64, [c_void_p, ctypes.c_int32]),
            "dq_state_merge": (c_int, [c_void_p, c_void_p, c_void_p]),
            "dq_state_fold": (c_int, [c_void_p, c_int, c_int, c_void_p]),
            "dq_hll_count": (ctypes.c_double, [c_void_p]),
            "dq_spark_hash64": (c_int64, [ctypes.c_int32, c_void_p, c_int64]),
            "dq_frequencies": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_uint32, c_void_p]),
            "dq_freq_summarize": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
            "dq_freq_key_kind": (c_int, [c_void_p]),
            "dq_freq_top": (c_int64, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
            "dq_freq_export": (c_int64, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
            "dq_freq_free": (None, [c_void_p, c_void_p]),
            "dq_partition_keys": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
            "dq_quantile_summary": (c_int64, [c_void_p, c_void_p, c_int64, ctypes.c_double, c_int64, c_void_p,
                                              c_void_p, c_void_p]),
            "dq_quantile_summaries": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p,
                                              c_void_p, c_void_p, c_void_p]),
            "dq_kll_sketch": (c_int64, [c_void_p, c_void_p, c_int64, ctypes.c_int32, ctypes.c_double, c_void_p,
                                        c_int64]),
            "dq_kll_sketch_columns": (c_int64, [c_void_p, c_void_p, ctypes.c_int32, c_int64, ctypes.c_int32,
                                                ctypes.c_double, c_void_p, c_int64, c_void_p]),
            "dq_kll_merge_states": (c_int64, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64]),
            "dq_cast_column": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_int32, c_void_p, c_void_p]),
            "dq_synth_column": (c_int, [c_void_p, ctypes.c_int32, ctypes.c_uint64, c_int64, c_int64, c_void_p]),
            "dq_synth_freq_keys": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p]),
            "dq_synth_validity": (c_int, [c_void_p, ctypes.c_uint64, c_int64, c_int64, ctypes.c_int32, c_void_p]),
            "dq_frequencies_ex": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
            "dq_freq_row_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_uint32]),
            "dq_synth_strings": (c_int, [c_void_p, ctypes.c_int32, ctypes.c_uint64, c_int64, c_int64, c_void_p, c_void_p,
                                         c_void_p]),
            "dq_freq_export_device": (c_int64, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
            "dq_freq_from_pairs": (c_int, [c_void_p, ctypes.c_int32, c_void_p, c_void_p, c_int64, c_uint32, c_int64,
                                           c_int64, c_void_p]),
            "dq_freq_merge": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
            "dq_freq_mutual_information": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
            "dq_open_devices": (c_void_p, [c_void_p, c_int, ctypes.POINTER(c_int)]),
            "dq_scan_streamed": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                         c_int64]),
            "dq_ctx_num_devices": (c_int, [c_void_p]),
            "dq_ctx_uses_rccl": (c_int, [c_void_p]),
            "dq_scan_sharded": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                        c_void_p]),
            "dq_schema_validate": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_uint32, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
            "dq_schema_launch_count": (c_int64, [c_void_p]),
            "dq_gather_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
            "dq_parse_int32": (c_int, [ctypes.c_char_p, ctypes.c_int32, c_void_p]),
            "dq_parse_decimal": (c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_void_p]),
            "dq_parse_timestamp": (c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32,
                                           c_void_p]),
            "dq_split_rows": (c_int, [c_void_p, c_int64, c_int64, ctypes.c_uint64, ctypes.c_double, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
            "dq_split_row_is_test": (c_int, [c_int64, ctypes.c_uint64, ctypes.c_double]),
            "dq_dec128_to_double": (ctypes.c_double, [c_void_p, ctypes.c_int32]),
            "dq_dict_scan": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p,
                                     c_int, c_void_p]),
            "dq_dict_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
            "dq_dict_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
            "dq_filter_validity": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p,
                                           c_void_p]),
            "dq_freq_row_bits": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64]),
            "dq_freq_probe": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p]),
            "dq_row_outcomes": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                        c_int, c_uint32, c_void_p, c_void_p]),
            "dq_csv_index": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_int32, ctypes.c_int32, c_void_p, c_void_p,
                                     c_void_p]),
            "dq_csv_field": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_int32, c_void_p, c_void_p, c_void_p]),
            "dq_csv_column": (c_int, [c_void_p, c_void_p, ctypes.c_int32, ctypes.c_int32, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
            "dq_csv_free": (None, [c_void_p, c_void_p]),
            "dq_csv_write_size": (c_int, [c_void_p, c_void_p, ctypes.c_int32, c_int64, c_void_p, c_void_p]),
            "dq_csv_write": (c_int, [c_void_p, c_void_p, ctypes.c_int32, c_int64, c_void_p, c_void_p, c_int64]),
            "dq_csv_write_launch_count": (c_int64, [c_void_p, ctypes.c_int32]),
            "dq_csv_write_route_count": (c_int64, [c_void_p, ctypes.c_int32]),
            "dq_ingest_bits": (c_int, [c_void_p, c_void_p, ctypes.c_int32, c_int64, ctypes.c_int32, c_void_p]),
            "dq_ingest_offsets": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_int32, c_int64, c_int64, ctypes.c_int32,
                                          c_void_p, c_void_p]),
            "dq_ingest_convert": (c_int, [c_void_p, ctypes.c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                          c_int64, c_void_p]),
            "dq_ingest_indices": (c_int, [c_void_p, c_void_p, c_int64, ctypes.c_int32, ctypes.c_int32, c_void_p, c_int64,
                                          c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
        }
        for name, (res, args) in sig.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        if path is None:
            _lib = lib
        return lib


def hll_count(words):
    """DeequHyperLogLogPlusPlusUtils.count over 52 packed register words (host-side, C-ABI)."""
    lib = load_library()
    arr = (ctypes.c_int64 * HLL_NUM_WORDS)(*[int(np.int64(np.uint64(w & 0xFFFFFFFFFFFFFFFF))) for w in words])
    return lib.dq_hll_count(arr)


def parse_int32(cell):
    """dq_parse_int32: cast(cell as int) of the row-level schema validator, (class, value) (host-side, C-ABI)."""
    out = ctypes.c_int32(0)
    rc = load_library().dq_parse_int32(cell, len(cell), ctypes.byref(out))
    return rc, (int(out.value) if rc == PARSE_VALUE else None)


def parse_decimal(cell, precision, scale):
    """dq_parse_decimal: cast(cell as decimal(precision, scale)), (class, unscaled value)."""
    out = ctypes.c_int64(0)
    rc = load_library().dq_parse_decimal(cell, len(cell), int(precision), int(scale), ctypes.byref(out))
    return rc, (int(out.value) if rc == PARSE_VALUE else None)


def parse_timestamp(program, cell):
    """dq_parse_timestamp: unix_timestamp(cell, mask) over a compiled mask, (class, microseconds)."""
    out = ctypes.c_int64(0)
    rc = load_library().dq_parse_timestamp(program, len(program), cell, len(cell), ctypes.byref(out))
    return rc, (int(out.value) if rc == PARSE_VALUE else None)


def split_row_is_test(global_row, seed, test_ratio):
    """dq_split_row_is_test: 1 = the row is in the TEST set, 0 = TRAIN, < 0 = bad argument (host-side, C-ABI)."""
    return int(load_library().dq_split_row_is_test(int(global_row), int(seed) & 0xFFFFFFFFFFFFFFFF, float(test_ratio)))


def kll_merge_states(a, b):
    """dq_kll_merge_states: KLLState.sum of two serialized KLLStates (host-side, C-ABI)."""
    lib = load_library()
    cap = len(a) + len(b) + 64
    while True:
        out = ctypes.create_string_buffer(cap)
        n = lib.dq_kll_merge_states(a, len(a), b, len(b), out, cap)
        if n < 0:
            raise NativeError(int(n), "dq_kll_merge_states: malformed KLLState bytes")
        if n <= cap:
            return out.raw[:n]
        cap = int(n)


def dec128_cell(unscaled):
    """The 16-byte little-endian two's-complement cell of an unscaled value (a ctypes buffer)."""
    return ctypes.create_string_buffer((int(unscaled) & ((1 << 128) - 1)).to_bytes(16, "little"), 16)


def dec128_to_double(unscaled, scale):
    """dq_dec128_to_double: Decimal.toDouble of one DECIMAL128 cell (host-side, C-ABI; the kernel's own code)."""
    return float(load_library().dq_dec128_to_double(dec128_cell(unscaled), int(scale)))


def spark_hash64(spark_type, value):
    """Spark XxHash64Function.hash(value, type, 42) as a signed 64-bit int (test hook)."""
    lib = load_library()
    if spark_type == TYPE_DECIMAL128:  # value: the unscaled integer
        return lib.dq_spark_hash64(spark_type, dec128_cell(value), 16)
    if spark_type == TYPE_STRING:
        b = value.encode("utf-8") if isinstance(value, str) else bytes(value)
        buf = ctypes.create_string_buffer(b, len(b))
        return lib.dq_spark_hash64(spark_type, buf, len(b))
    dtype = {TYPE_BOOLEAN: np.uint8, TYPE_BYTE: np.int8, TYPE_SHORT: np.int16, TYPE_INT: np.int32,
             TYPE_DATE: np.int32, TYPE_LONG: np.int64, TYPE_TIMESTAMP: np.int64, TYPE_DECIMAL: np.int64,
             TYPE_FLOAT: np.float32, TYPE_DOUBLE: np.float64}[spark_type]
    a = np.array([value], dtype=dtype)
    return lib.dq_spark_hash64(spark_type, a.ctypes.data, a.nbytes)


def merge_states(a, b):
    """State.sum through the C-ABI (dq_state_merge)."""
    lib = load_library()
    out = DqState()
    rc = lib.dq_state_merge(ctypes.byref(a), ctypes.byref(b), ctypes.byref(out))
    if rc != DQ_OK:
        raise NativeError(rc, "dq_state_merge")
    return out


def fold_states(buf, nparts, nops):
    """dq_state_fold over a part-major buffer of nparts x nops dq_state records (any object exposing
    the buffer protocol, e.g. a pinned host tensor's numpy view); returns nops DqState."""
    lib = load_library()
    arr = np.frombuffer(buf, dtype=np.uint8, count=nparts * nops * STATE_SIZE)
    out = (DqState * max(nops, 1))()
    rc = lib.dq_state_fold(arr.ctypes.data, int(nparts), int(nops), out)
    if rc != DQ_OK:
        raise NativeError(rc, "dq_state_fold")
    return [out[i] for i in range(nops)]


class Context:
    """One dq_ctx bound to one GPU (one per process / rank), or — `devices` given — one context over several
    GPUs of this node (dq_open_devices: row-sharded scans, RCCL exchange of grouping keys)."""

    def __init__(self, device=0, devices=None):
        self.lib = load_library()
        status = ctypes.c_int(0)
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            self.handle = self.lib.dq_open_devices(arr, len(devices), ctypes.byref(status))
            device = int(devices[0])
        else:
            self.handle = self.lib.dq_open(int(device), ctypes.byref(status))
        if not self.handle:
            raise NativeError(status.value, "dq_open(%r) failed: a MI355X GPU is required" % (devices or device))
        self.device = device
        self.devices = list(devices) if devices is not None else [device]
        self.multi = devices is not None  # dq_open_devices: host columns in, host results out

    def num_devices(self):
        return self.lib.dq_ctx_num_devices(self.handle)

    def uses_rccl(self):
        return bool(self.lib.dq_ctx_uses_rccl(self.handle))

    def close(self):
        if self.handle:
            self.lib.dq_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        msg = self.lib.dq_last_error(self.handle)
        return msg.decode() if msg else ""

    def check(self, rc, what):
        if rc != DQ_OK:
            raise NativeError(rc, "%s: %s" % (what, self.last_error()))

    def set_stream(self, stream_ptr):
        self.check(self.lib.dq_set_stream(self.handle, ctypes.c_void_p(stream_ptr or 0)), "dq_set_stream")

    def set_priority(self, priority):
        """dq_set_priority: 1 high, 0 normal, -1 low stream priority for this context's work."""
        if getattr(self, "_priority", 0) != priority:
            self.check(self.lib.dq_set_priority(self.handle, int(priority)), "dq_set_priority")
            self._priority = priority

    def synchronize(self):
        self.check(self.lib.dq_synchronize(self.handle), "dq_synchronize")

    def scan_launch_count(self):
        return self.lib.dq_scan_launch_count(self.handle)

    def kernel_launches(self):
        """{kernel name: launches so far} of the scan path (dq_scan_kernel_launches)."""
        return {name: int(self.lib.dq_scan_kernel_launches(self.handle, i)) for i, name in enumerate(SCAN_KERNELS)}

    def freq_paths(self):
        """{grouping build path: count so far} (dq_freq_path_count): which build produced the tables."""
        return {name: int(self.lib.dq_freq_path_count(self.handle, i)) for i, name in enumerate(FREQ_PATHS)}

    def scan(self, columns, nrows, ops, preds, out_device_ptr=None):
        """Run dq_scan. `columns`: list of DqColumn, `ops`: list of DqOp, `preds`: list of DqPredicate.
        Returns a list of DqState (host) or None when writing to a device buffer."""
        ncol = len(columns)
        col_arr = (DqColumn * max(ncol, 1))(*columns)
        op_arr = (DqOp * max(len(ops), 1))(*ops)
        pred_arr = (DqPredicate * max(len(preds), 1))(*preds)
        if out_device_ptr is not None:
            rc = self.lib.dq_scan(self.handle, col_arr, ncol, int(nrows), op_arr, len(ops), pred_arr, len(preds),
                                  ctypes.c_void_p(out_device_ptr), SCAN_OUT_DEVICE)
            self.check(rc, "dq_scan")
            return None
        out = (DqState * max(len(ops), 1))()
        rc = self.lib.dq_scan(self.handle, col_arr, ncol, int(nrows), op_arr, len(ops), pred_arr, len(preds), out, 0)
        self.check(rc, "dq_scan")
        return [out[i] for i in range(len(ops))]

    def dict_scan(self, columns, dicts, nrows, ops, preds):
        """Run dq_dict_scan: ops over dictionary-encoded columns (`dicts`: list of DqDictColumn; an op's column index
        len(columns) + d names dicts[d]). Returns a list of DqState (host)."""
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        dict_arr = (DqDictColumn * max(len(dicts), 1))(*dicts)
        op_arr = (DqOp * max(len(ops), 1))(*ops)
        pred_arr = (DqPredicate * max(len(preds), 1))(*preds)
        out = (DqState * max(len(ops), 1))()
        rc = self.lib.dq_dict_scan(self.handle, col_arr, len(columns), dict_arr, len(dicts), int(nrows), op_arr, len(ops),
                                   pred_arr, len(preds), out)
        self.check(rc, "dq_dict_scan")
        return [out[i] for i in range(len(ops))]

    def dict_counts(self, dict_column, counts_dev_ptr):
        """dq_dict_counts: the per-entry row counts into counts_dev_ptr (n_dict int64); returns (rows, non-NULL rows)."""
        rows = (ctypes.c_int64 * 2)()
        rc = self.lib.dq_dict_counts(self.handle, ctypes.byref(dict_column), ctypes.c_void_p(counts_dev_ptr), rows)
        self.check(rc, "dq_dict_counts")
        return int(rows[0]), int(rows[1])

    def dict_decode(self, dict_column, offsets_ptr, values_ptr=None):
        """dq_dict_decode: the sizing call (values_ptr None: writes the offsets) or the copy call; returns the decoded
        byte count."""
        nbytes = ctypes.c_int64(0)
        rc = self.lib.dq_dict_decode(self.handle, ctypes.byref(dict_column), ctypes.c_void_p(offsets_ptr),
                                     ctypes.c_void_p(values_ptr) if values_ptr else None, ctypes.byref(nbytes))
        self.check(rc, "dq_dict_decode")
        return int(nbytes.value)

    def scan_streamed(self, columns, nrows, ops, preds, chunk_rows):
        """dq_scan_streamed: host columns streamed through HBM in row chunks (copy / scan overlapped)."""
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        op_arr = (DqOp * max(len(ops), 1))(*ops)
        pred_arr = (DqPredicate * max(len(preds), 1))(*preds)
        out = (DqState * max(len(ops), 1))()
        rc = self.lib.dq_scan_streamed(self.handle, col_arr, len(columns), int(nrows), op_arr, len(ops), pred_arr,
                                       len(preds), out, int(chunk_rows))
        self.check(rc, "dq_scan_streamed")
        return [out[i] for i in range(len(ops))]

    def quantile_summary(self, column, nrows, relative_error):
        """dq_quantile_summary: exact (value, rank) samples of a zero-uncertainty GK summary of the
        column's non-NULL values, and their count n."""
        cap = int(nrows) if relative_error <= 0.0 else min(int(nrows), int(2.0 / relative_error) + 8)
        cap = max(cap, 2)
        vals = np.empty(cap, dtype=np.float64)
        ranks = np.empty(cap, dtype=np.int64)
        count = ctypes.c_int64(0)
        ns = self.lib.dq_quantile_summary(self.handle, ctypes.byref(column), int(nrows), float(relative_error), cap,
                                          vals.ctypes.data, ranks.ctypes.data, ctypes.byref(count))
        if ns < 0:
            self.check(int(ns), "dq_quantile_summary")
        return vals[:ns].copy(), ranks[:ns].copy(), int(count.value)

    def quantile_summaries(self, requests):
        """dq_quantile_summaries: requests = [(parts, relative_error)], parts = the DqColumns of one column's
        consecutive row ranges; returns [(values, ranks, n)] per request, as quantile_summary over the parts
        concatenated."""
        if not requests:
            return []
        parts, begin, rels, cap = [], [0], [], 2
        for cols, rel in requests:
            parts.extend(cols)
            begin.append(len(parts))
            rels.append(float(rel))
            rows = sum(int(c.length) for c in cols)
            cap = max(cap, rows if rel <= 0.0 else min(rows, int(2.0 / rel) + 8))
        nreq = len(requests)
        part_arr = (DqColumn * len(parts))(*parts)
        begin_arr = np.asarray(begin, dtype=np.int32)
        rel_arr = np.asarray(rels, dtype=np.float64)
        vals = np.empty(nreq * cap, dtype=np.float64)
        ranks = np.empty(nreq * cap, dtype=np.int64)
        counts = np.zeros(nreq, dtype=np.int64)
        nsamp = np.zeros(nreq, dtype=np.int64)
        rc = self.lib.dq_quantile_summaries(self.handle, part_arr, begin_arr.ctypes.data, nreq, rel_arr.ctypes.data,
                                            cap, vals.ctypes.data, ranks.ctypes.data, counts.ctypes.data,
                                            nsamp.ctypes.data)
        self.check(rc, "dq_quantile_summaries")
        return [(vals[r * cap:r * cap + nsamp[r]].copy(), ranks[r * cap:r * cap + nsamp[r]].copy(), int(counts[r]))
                for r in range(nreq)]

    def kll_sketch(self, column, nrows, sketch_size, shrinking_factor):
        """dq_kll_sketch: the KLLState bytes of one partition holding the column's rows in order."""
        cap = 1 << 16
        while True:
            buf = np.empty(cap, dtype=np.uint8)
            n = self.lib.dq_kll_sketch(self.handle, ctypes.byref(column), int(nrows), int(sketch_size),
                                       float(shrinking_factor), buf.ctypes.data, cap)
            if n < 0:
                self.check(int(n), "dq_kll_sketch")
            if n <= cap:
                return buf[:n].tobytes()
            cap = int(n)

    def kll_sketch_columns(self, columns, nrows, sketch_size, shrinking_factor):
        """dq_kll_sketch_columns: the KLLState bytes of each column (one partition each, rows in order), sketched in
        one call (parallel host schedules, one round trip)."""
        arr = (DqColumn * max(len(columns), 1))(*columns)
        sizes = np.zeros(max(len(columns), 1), dtype=np.int64)
        cap = (1 << 18) * max(len(columns), 1)  # a default sketch's state is ~40 KB: one call, not a size probe + a rerun
        while True:
            buf = np.empty(cap, dtype=np.uint8)
            n = self.lib.dq_kll_sketch_columns(self.handle, arr, len(columns), int(nrows), int(sketch_size),
                                               float(shrinking_factor), buf.ctypes.data, cap, sizes.ctypes.data)
            if n < 0:
                self.check(int(n), "dq_kll_sketch_columns")
            if n <= cap:
                out, at = [], 0
                for k in range(len(columns)):
                    out.append(buf[at:at + int(sizes[k])].tobytes())
                    at += int(sizes[k])
                return out
            cap = int(n)

    def cast_column(self, column, nrows, to_type, values_dev_ptr, validity_dev_ptr):
        """dq_cast_column: Spark Cast(column -> long | double) into caller-owned device buffers (torch's queued work
        on them, e.g. a zero fill, completes first: the cast runs on the context's stream)."""
        self._after_torch_stream()
        self.check(self.lib.dq_cast_column(self.handle, ctypes.byref(column), int(nrows), int(to_type),
                                            ctypes.c_void_p(values_dev_ptr), ctypes.c_void_p(validity_dev_ptr)),
                   "dq_cast_column")

    def schema_launch_count(self):
        return int(self.lib.dq_schema_launch_count(self.handle))

    def schema_validate(self, columns, nrows, defs, flags, true_ptr, false_ptr, ambiguous_ptr):
        """dq_schema_validate: returns (status, DqSchemaResult); a failed call is left to the caller, which names the
        ambiguous column from the result."""
        self._after_torch_stream()
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        def_arr = (DqSchemaColumn * max(len(defs), 1))(*defs)
        res = DqSchemaResult()
        rc = self.lib.dq_schema_validate(self.handle, col_arr, len(columns), int(nrows), def_arr, len(defs), int(flags),
                                         ctypes.c_void_p(true_ptr), ctypes.c_void_p(false_ptr),
                                         ctypes.c_void_p(ambiguous_ptr), ctypes.byref(res))
        return rc, res

    def gather_rows(self, column, nrows, select_ptr, nselected, values_ptr, validity_ptr, offsets_ptr=None):
        """dq_gather_rows; returns the bytes of a string gather."""
        self._after_torch_stream()
        nbytes = ctypes.c_int64(0)
        self.check(self.lib.dq_gather_rows(self.handle, ctypes.byref(column), int(nrows), ctypes.c_void_p(select_ptr),
                                           int(nselected), ctypes.c_void_p(values_ptr) if values_ptr else None,
                                           ctypes.c_void_p(validity_ptr) if validity_ptr else None,
                                           ctypes.c_void_p(offsets_ptr) if offsets_ptr else None, ctypes.byref(nbytes)),
                   "dq_gather_rows")
        return int(nbytes.value)

    FILTER_TARGETS = 32  # targets of one dq_filter_validity call (dq_internal.h kFilterTargets)

    def filter_validity(self, columns, nrows, pred, targets, out_ptrs):
        """dq_filter_validity: `pred` (a DqPredicate) over `columns`, ANDed into the validity of the columns indexed by
        `targets`, into the device bitmaps `out_ptrs` ((nrows + 63) // 64 words each); returns the TRUE rows."""
        self._after_torch_stream()
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        tgt = np.asarray(targets, dtype=np.int32)
        outs = (ctypes.c_void_p * max(len(out_ptrs), 1))(*[int(p) for p in out_ptrs])
        true_rows = ctypes.c_int64(0)
        self.check(self.lib.dq_filter_validity(self.handle, col_arr, len(columns), int(nrows), ctypes.byref(pred),
                                               tgt.ctypes.data, len(tgt), outs, ctypes.byref(true_rows)),
                   "dq_filter_validity")
        return int(true_rows.value)

    def freq_row_bits(self, table_handle, unique_ptr, part_ptr, nrows):
        """dq_freq_row_bits: per source row of a frequency table, `group count == 1` and `group count > 0` as two
        device bitmaps ((nrows + 63) // 64 words each)."""
        self._after_torch_stream()
        self.check(self.lib.dq_freq_row_bits(self.handle, table_handle, ctypes.c_void_p(unique_ptr),
                                             ctypes.c_void_p(part_ptr), int(nrows)), "dq_freq_row_bits")

    def freq_probe(self, table_handle, columns, nrows, key_columns, bits_ptr=None, outcome_ptr=None):
        """dq_freq_probe: the rows of `columns` (DqColumn list; `key_columns` index it, paired by position with the
        table's key columns) against a frequency table under SQL '='. Optional device outputs: a bitmap
        ((nrows + 63) // 64 words) and one 0/1 byte per row. Returns the number of matching rows."""
        self._after_torch_stream()
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        keys = np.asarray(key_columns, dtype=np.int32)
        matched = ctypes.c_int64(0)
        self.check(self.lib.dq_freq_probe(self.handle, table_handle, col_arr, len(columns), int(nrows), keys.ctypes.data,
                                          len(keys), ctypes.c_void_p(bits_ptr) if bits_ptr else None,
                                          ctypes.c_void_p(outcome_ptr) if outcome_ptr else None, ctypes.byref(matched)),
                   "dq_freq_probe")
        return int(matched.value)

    def row_outcomes(self, columns, nrows, preds, terms, checks, flags=0):
        """dq_row_outcomes: `terms` (DqRowTerm) over `columns` / `preds` (DqPredicate) folded into the output buffers of
        `checks` (DqRowCheck) in one launch; returns ([(matched, considered)] per term, [(TRUE rows, NULL rows)] per
        check)."""
        self._after_torch_stream()
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        pred_arr = (DqPredicate * max(len(preds), 1))(*preds)
        term_arr = (DqRowTerm * max(len(terms), 1))(*terms)
        check_arr = (DqRowCheck * max(len(checks), 1))(*checks)
        tc = (ctypes.c_int64 * (2 * max(len(terms), 1)))()
        cc = (ctypes.c_int64 * (2 * max(len(checks), 1)))()
        self.check(self.lib.dq_row_outcomes(self.handle, col_arr, len(columns), int(nrows), pred_arr, len(preds), term_arr,
                                            len(terms), check_arr, len(checks), int(flags), tc, cc), "dq_row_outcomes")
        return ([(int(tc[2 * i]), int(tc[2 * i + 1])) for i in range(len(terms))],
                [(int(cc[2 * i]), int(cc[2 * i + 1])) for i in range(len(checks))])

    def csv_kernel_launches(self):
        """{kernel name: launches so far} of the device CSV reader (the DQ_KERNEL_CSV_* entries)."""
        return {name: int(self.lib.dq_scan_kernel_launches(self.handle, len(SCAN_KERNELS) + i))
                for i, name in enumerate(CSV_KERNELS)}

    def csv_index(self, bytes_ptr, nbytes, ncols, skip_records):
        """dq_csv_index over device bytes: (handle or None for a refused file, DqCsvResult, [DqCsvColumnReport])."""
        self._after_torch_stream()
        handle = ctypes.c_void_p(None)
        res = DqCsvResult()
        reports = (DqCsvColumnReport * max(int(ncols), 1))()
        self.check(self.lib.dq_csv_index(self.handle, ctypes.c_void_p(bytes_ptr), int(nbytes), int(ncols),
                                         int(skip_records), ctypes.byref(handle), ctypes.byref(res), reports),
                   "dq_csv_index")
        return handle.value, res, [reports[i] for i in range(int(ncols))]

    def csv_field(self, handle, row, col):
        """dq_csv_field: (start, unquoted length, escaped) of one field of an index."""
        start, length, escaped = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self.check(self.lib.dq_csv_field(self.handle, ctypes.c_void_p(handle), int(row), int(col), ctypes.byref(start),
                                         ctypes.byref(length), ctypes.byref(escaped)), "dq_csv_field")
        return int(start.value), int(length.value), bool(escaped.value)

    def csv_column(self, handle, col, spark_type, values_ptr, validity_ptr, offsets_ptr=None):
        """dq_csv_column into caller-owned device buffers; returns the bytes of a string column."""
        self._after_torch_stream()
        nbytes = ctypes.c_int64(0)
        self.check(self.lib.dq_csv_column(self.handle, ctypes.c_void_p(handle), int(col), int(spark_type),
                                          ctypes.c_void_p(values_ptr) if values_ptr else None,
                                          ctypes.c_void_p(validity_ptr) if validity_ptr else None,
                                          ctypes.c_void_p(offsets_ptr) if offsets_ptr else None, ctypes.byref(nbytes)),
                   "dq_csv_column")
        return int(nbytes.value)

    def csv_free(self, handle):
        if handle:
            self.lib.dq_csv_free(self.handle, ctypes.c_void_p(handle))

    def csv_write_kernel_launches(self):
        """{kernel name: launches so far} of the device CSV writer (dq_csv_write_launch_count)."""
        return {name: int(self.lib.dq_csv_write_launch_count(self.handle, i)) for i, name in enumerate(CSV_WRITE_KERNELS)}

    def csv_write_routes(self):
        """{route: tiles of the write kernel that took it so far} (dq_csv_write_route_count)."""
        return {name: int(self.lib.dq_csv_write_route_count(self.handle, i)) for i, name in enumerate(CSV_WRITE_ROUTES)}

    def csv_write_size(self, columns, nrows, row_start_ptr):
        """dq_csv_write_size: fills row_start (device, nrows + 1 int64); returns the body's bytes."""
        self._after_torch_stream()
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        total = ctypes.c_int64(0)
        self.check(self.lib.dq_csv_write_size(self.handle, col_arr, len(columns), int(nrows),
                                              ctypes.c_void_p(row_start_ptr), ctypes.byref(total)), "dq_csv_write_size")
        return int(total.value)

    def csv_write_body(self, columns, nrows, row_start_ptr, out_ptr, out_bytes):
        """dq_csv_write: the body into out (device, out_bytes bytes) from the sizing call's row_start."""
        self._after_torch_stream()
        col_arr = (DqColumn * max(len(columns), 1))(*columns)
        self.check(self.lib.dq_csv_write(self.handle, col_arr, len(columns), int(nrows), ctypes.c_void_p(row_start_ptr),
                                         ctypes.c_void_p(out_ptr) if out_ptr else None, int(out_bytes)), "dq_csv_write")

    def csv_write(self, columns, nrows, device, limit=2 ** 31):
        """The CSV body of device columns (a list of DqColumn) as a device uint8 tensor, without touching disk: the
        sizing call, one allocation, the write call. A body of `limit` bytes or more raises ValueError."""
        import torch
        dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        row_start = torch.empty(int(nrows) + 1, dtype=torch.int64, device=dev)
        total = self.csv_write_size(columns, nrows, row_start.data_ptr())
        if total >= limit:
            raise ValueError("the CSV body holds %d bytes: the device writer takes bodies below 2^31 bytes; a "
                             "ChunkedTable writes its chunks one after the other" % total)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        self.csv_write_body(columns, nrows, row_start.data_ptr(), out.data_ptr() if total else None, total)
        return out

    def ingest_kernel_launches(self):
        """{kernel name: launches so far} of the Arrow ingest (the DQ_KERNEL_INGEST_* entries)."""
        return {name: int(self.lib.dq_scan_kernel_launches(self.handle, len(SCAN_KERNELS) + len(CSV_KERNELS) + i))
                for i, name in enumerate(INGEST_KERNELS)}

    def ingest_bits(self, pieces, nrows, to_bytes, out_ptr):
        """dq_ingest_bits: `pieces` = [(src_ptr or None, src_bytes, src_bit0, rows)] in row order -> the validity
        words (to_bytes False) or one byte per row (True) at out_ptr."""
        self._after_torch_stream()
        arr = (DqIngestPiece * max(len(pieces), 1))()
        at = 0
        for k, (src, nbytes, bit0, rows) in enumerate(pieces):
            arr[k].src, arr[k].src_bytes, arr[k].src_bit0, arr[k].rows, arr[k].out_row0 = src, nbytes, bit0, rows, at
            at += rows
        self.check(self.lib.dq_ingest_bits(self.handle, arr, len(pieces), int(nrows), 1 if to_bytes else 0,
                                           ctypes.c_void_p(out_ptr)), "dq_ingest_bits")

    def ingest_offsets(self, src_ptr, src_bytes, src_width, rows, base, write_last, out_ptr):
        """dq_ingest_offsets for one piece; True when a rebased offset left [0, 2^31)."""
        self._after_torch_stream()
        flag = ctypes.c_int32(0)
        self.check(self.lib.dq_ingest_offsets(self.handle, ctypes.c_void_p(src_ptr), int(src_bytes), int(src_width),
                                              int(rows), int(base), 1 if write_last else 0, ctypes.c_void_p(out_ptr),
                                              ctypes.byref(flag)), "dq_ingest_offsets")
        return bool(flag.value)

    def ingest_convert(self, kind, src_ptr, src_bytes, validity, rows, param, out_ptr):
        """dq_ingest_convert for one piece; `validity` = (ptr, bytes, bit0) or None."""
        self._after_torch_stream()
        vptr, vbytes, vbit0 = validity or (None, 0, 0)
        self.check(self.lib.dq_ingest_convert(self.handle, int(kind), ctypes.c_void_p(src_ptr), int(src_bytes),
                                              ctypes.c_void_p(vptr) if vptr else None, int(vbytes), int(vbit0), int(rows),
                                              int(param), ctypes.c_void_p(out_ptr)), "dq_ingest_convert")

    def ingest_indices(self, src_ptr, src_bytes, width, signed, validity, rows, n_dict, dict_validity_ptr, out_ptr,
                       out_validity_ptr):
        """dq_ingest_indices for one piece: (bad_row or -1, bad_index, null_rows)."""
        self._after_torch_stream()
        vptr, vbytes, vbit0 = validity or (None, 0, 0)
        rep = DqIngestIndexReport()
        self.check(self.lib.dq_ingest_indices(self.handle, ctypes.c_void_p(src_ptr), int(src_bytes), int(width),
                                              1 if signed else 0, ctypes.c_void_p(vptr) if vptr else None, int(vbytes),
                                              int(vbit0), int(rows), int(n_dict),
                                              ctypes.c_void_p(dict_validity_ptr) if dict_validity_ptr else None,
                                              ctypes.c_void_p(out_ptr),
                                              ctypes.c_void_p(out_validity_ptr) if out_validity_ptr else None,
                                              ctypes.byref(rep)), "dq_ingest_indices")
        return int(rep.bad_row), int(rep.bad_index), int(rep.null_rows)

    def split_rows(self, nrows, row0, seed, test_ratio, train_ptr, test_ptr):
        """dq_split_rows into two device bitmaps (either pointer may be None); returns (num_train, num_test)."""
        self._after_torch_stream()
        ntrain, ntest = ctypes.c_int64(0), ctypes.c_int64(0)
        self.check(self.lib.dq_split_rows(self.handle, int(nrows), int(row0), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          float(test_ratio), ctypes.c_void_p(train_ptr) if train_ptr else None,
                                          ctypes.c_void_p(test_ptr) if test_ptr else None, ctypes.byref(ntrain),
                                          ctypes.byref(ntest)),
                   "dq_split_rows")
        return int(ntrain.value), int(ntest.value)

    def _after_torch_stream(self):
        """The generators run on the context's stream; a buffer torch just allocated and filled (torch.zeros) on its
        own stream must be complete before they write into it. The stream is this thread's current stream of the
        context's device (explicitly: a helper thread starts on device 0)."""
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_initialized():
            for d in self.devices:
                torch.cuda.current_stream(int(d)).synchronize()

    def synth_column(self, kind, seed, row0, nrows, dev_ptr):
        self._after_torch_stream()
        self.check(self.lib.dq_synth_column(self.handle, kind, seed & 0xFFFFFFFFFFFFFFFF, row0, nrows,
                                            ctypes.c_void_p(dev_ptr)), "dq_synth_column")

    def synth_freq_keys(self, total_rows, distinct, row0, nrows, dev_ptr):
        self._after_torch_stream()
        self.check(self.lib.dq_synth_freq_keys(self.handle, int(total_rows), int(distinct), int(row0), int(nrows),
                                               ctypes.c_void_p(dev_ptr)), "dq_synth_freq_keys")

    def synth_strings(self, kind, seed, row0, nrows, offsets_ptr, bytes_ptr=None):
        """dq_synth_strings: offsets first (returns the text bytes), then the bytes."""
        self._after_torch_stream()
        total = ctypes.c_int64(0)
        self.check(self.lib.dq_synth_strings(self.handle, int(kind), seed & 0xFFFFFFFFFFFFFFFF, int(row0), int(nrows),
                                             ctypes.c_void_p(offsets_ptr),
                                             ctypes.c_void_p(bytes_ptr) if bytes_ptr else None, ctypes.byref(total)),
                   "dq_synth_strings")
        return int(total.value)

    def synth_validity(self, seed, row0, nrows, null_permille, dev_ptr):
        self._after_torch_stream()
        self.check(self.lib.dq_synth_validity(self.handle, seed & 0xFFFFFFFFFFFFFFFF, row0, nrows, null_permille,
                                              ctypes.c_void_p(dev_ptr)), "dq_synth_validity")


_contexts = {}
_aux_lock = threading.Lock()
_aux_pool = {}     # (device, slot) -> [Context, ...]
_aux_leased = set()  # id() of the aux contexts a helper thread drives right now


def lease_aux_context(device=0, slot="aux", priority=0):
    """A single-device context of `device` (its own stream and scratch cache) for one helper thread: the cached
    context of `slot` unless another thread holds it (dq.h: calls on one ctx are not re-entrant), else another one of
    the slot's pool. Return it with release_aux_context. Helper work overlaps the main context's (the
    ColumnProfiler's histogram pass beside its numeric pass, a run's grouping builds beside its scans)."""
    key = (int(device), slot)
    ctx = None
    with _aux_lock:
        pool = _aux_pool.setdefault(key, [])
        for c in pool:
            if id(c) not in _aux_leased:
                _aux_leased.add(id(c))
                ctx = c
                break
    if ctx is None:
        ctx = Context(device)  # outside the lock: dq_open may take a while
        with _aux_lock:
            _aux_pool[key].append(ctx)
            _aux_leased.add(id(ctx))
    try:
        ctx.set_priority(priority)  # (the leased context is idle: its stream can be replaced)
    except BaseException:
        release_aux_context(ctx)
        raise
    return ctx


def release_aux_context(ctx):
    """The helper is done with `ctx`: its cached scratch beyond the idle cap is released and the context may be leased
    again."""
    try:
        ctx.lib.dq_scratch_trim(ctx.handle, AUX_IDLE_SCRATCH_BYTES)
    finally:
        with _aux_lock:
            _aux_leased.discard(id(ctx))


# idle device scratch an aux context keeps between runs (its builds re-use it instead of hipMalloc'ing again; an
# allocation that fails on any context of the device releases the others' idle scratch first, dq_api.cpp). r06: the
# same 48 GB as a context's own cap (dq_api.cpp kScratchCacheCap). At 16 GiB the C5 text grouping's ~27 GB working set
# was freed and re-allocated every run; on some boxes those hipFree / hipMalloc rounds made the overlapped C5 step
# 340-560 ms, with the scratch-heavy passes alone 5-16x slower afterwards (profiles/r06/c5_priority_risk_r06bg.txt)
AUX_IDLE_SCRATCH_BYTES = int(float(os.environ.get("DQ_AUX_IDLE_SCRATCH", 48e9)))


def aux_context(device=0, slot="aux"):
    """The cached context of `slot` (see lease_aux_context) without a lease: single-threaded callers only."""
    key = (int(device), slot)
    with _aux_lock:
        pool = _aux_pool.setdefault(key, [])
        if pool:
            return pool[0]
    ctx = Context(device)
    with _aux_lock:
        _aux_pool[key].append(ctx)
    return ctx


def context(device=0):
    """Process-wide cached context for a device. DQ_DEVICES="0,1,..." makes it one multi-device context over
    those GPUs (every host-column scan / grouping of the runner is then row-sharded across them)."""
    spec = os.environ.get("DQ_DEVICES")
    key = ("multi", spec) if spec else device
    ctx = _contexts.get(key)
    if ctx is None:
        ctx = Context(device, devices=[int(d) for d in spec.split(",")] if spec else None)
        _contexts[key] = ctx
    return ctx
