/*
 * dq.h — C-ABI of the MI355X-native deequ metrics engine (libdq.so).
 *
 * This is the drop-in boundary for deequ's AnalysisRunner hot path. The reference has no native
 * code: the seams replaced here are Scala methods, cited per entry point. A JVM host binds these
 * symbols over JNI; this repository's host mirror binds them over ctypes
 * (deequ_amd/native.py).
 *
 * Conventions
 *   - Plain C types only; no torch / HIP types cross this boundary (streams are `void*`).
 *   - Every call returns 0 (DQ_OK) on success or a negative dq_status; dq_last_error(ctx) then
 *     holds a message. A failed dq_scan fails EVERY op of the batch, mirroring the catch-all in
 *     runScanningAnalyzers (R/AnalysisRunner.scala:320-323).
 *   - A dq_ctx from dq_open is bound to one GPU; one from dq_open_devices spans several GPUs of the node. A ctx
 *     is not re-entrant: one driver thread per ctx. Several contexts of one GPU (each its own stream, scratch
 *     cache and pinned staging) may be driven by different threads at once: independent passes of one analysis
 *     then overlap on the device (the Python host runs grouping builds, histogram builds and the odd row chunks of
 *     a shard on helper contexts this way). Inputs are read-only to every context; a buffer one context's stream
 *     writes must not be read by another before that stream is synchronised.
 *   - States are returned in native byte order (little-endian on x86/MI355X hosts) with the
 *     field order of the reference's HdfsStateProvider layouts (A/StateProvider.scala:187-262).
 *
 * Path abbreviations: A/ = src/main/scala/com/amazon/deequ/analyzers/,
 * R/ = A/runners/, C/ = A/catalyst/ (all under /root/reference).
 */
#ifndef DEEQU_AMD_DQ_H
#define DEEQU_AMD_DQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQ_ABI_VERSION 2

/* ---------------------------------------------------------------------------------------------
 * Status codes
 * ------------------------------------------------------------------------------------------- */
typedef enum dq_status {
    DQ_OK = 0,
    DQ_ERR_INVALID_ARGUMENT = -1,  /* bad op / column index / length mismatch          */
    DQ_ERR_UNSUPPORTED = -2,       /* op not defined for this Spark type               */
    DQ_ERR_DEVICE = -3,            /* HIP runtime error (message in dq_last_error)     */
    DQ_ERR_OUT_OF_MEMORY = -4,
    DQ_ERR_NO_DEVICE = -5,         /* no MI355X visible: the engine never falls back   */
    DQ_ERR_PREDICATE = -6,         /* malformed predicate program                      */
    DQ_ERR_ALIGNMENT = -7          /* device column not 16-B (values) / 8-B (bitmap) aligned */
} dq_status;

/* ---------------------------------------------------------------------------------------------
 * Columns: Arrow-style buffers carrying the *Spark* physical type. The type is mandatory because
 * HLL hashing (C/StatefulHyperloglogPlus.scala:93) and Sum/Min/Max result rules depend on it.
 * ------------------------------------------------------------------------------------------- */
typedef enum dq_spark_type {
    DQ_TYPE_BOOLEAN = 1,    /* uint8 0/1                                 */
    DQ_TYPE_BYTE = 2,       /* int8                                      */
    DQ_TYPE_SHORT = 3,      /* int16                                     */
    DQ_TYPE_INT = 4,        /* int32                                     */
    DQ_TYPE_LONG = 5,       /* int64                                     */
    DQ_TYPE_FLOAT = 6,      /* float32                                   */
    DQ_TYPE_DOUBLE = 7,     /* float64                                   */
    DQ_TYPE_STRING = 8,     /* UTF-8 bytes in `values`, int32 `offsets`  */
    DQ_TYPE_DATE = 9,       /* int32 days since epoch                    */
    DQ_TYPE_TIMESTAMP = 10, /* int64 microseconds since epoch            */
    DQ_TYPE_DECIMAL = 11,   /* int64 unscaled value, precision <= 18     */
    /* 16-byte little-endian two's-complement unscaled value (Arrow's decimal128 cell), 19 <= decimal_precision <= 38,
     * 0 <= decimal_scale <= precision; device values 16-byte aligned; results are defined for |unscaled| < 10^38.
     * Spark hashes and stores precision <= 18 as longs: those stay DQ_TYPE_DECIMAL. Accepted by single-device dq_scan
     * (Completeness, Sum, Mean, Minimum, Maximum, StandardDeviation, ApproxCountDistinct; a `where` may read other
     * columns) and as a dq_cast_column source; every other entry point fails it with DQ_ERR_UNSUPPORTED. */
    DQ_TYPE_DECIMAL128 = 12
} dq_spark_type;

#define DQ_COL_DEVICE 0x1u /* values/validity/offsets are device pointers on the ctx's GPU */
/* STRING: `offsets` points to length + 1 int64 offsets (Arrow large_string) -- a column whose UTF-8 bytes pass
 * 2^31, e.g. the row chunks of a shard concatenated in HBM for one grouping build. Accepted by dq_frequencies(_ex)
 * only; every other entry point fails such a column with DQ_ERR_UNSUPPORTED. */
#define DQ_COL_OFFSETS64 0x2u

typedef struct dq_column {
    int32_t spark_type;        /* dq_spark_type                                               */
    uint32_t flags;            /* DQ_COL_*                                                    */
    int64_t length;            /* rows                                                        */
    const void* values;        /* fixed width: `length` elements; STRING: UTF-8 data bytes    */
    const uint8_t* validity;   /* Arrow LSB-first bitmap (bit i set = row i non-null), or NULL */
    const int32_t* offsets;    /* STRING only: length + 1 offsets into `values`                */
    int32_t decimal_precision; /* DECIMAL only                                                 */
    int32_t decimal_scale;     /* DECIMAL only                                                 */
} dq_column;

/* ---------------------------------------------------------------------------------------------
 * Predicates (`where` filters and Compliance predicates). deequ accepts Spark SQL strings
 * (A/Analyzer.scala:409-432, A/Compliance.scala:49-52); the host compiles them to this postfix
 * program, evaluated per row on the GPU with SQL three-valued logic.
 * ------------------------------------------------------------------------------------------- */
typedef enum dq_pred_opcode {
    DQ_P_COL = 1,        /* arg: column index          -> push column value (NULL if invalid) */
    DQ_P_CONST = 2,      /* arg: constant index        -> push constant                       */
    DQ_P_NULL = 3,       /*                            -> push NULL                           */
    DQ_P_EQ = 10, DQ_P_NE = 11, DQ_P_LT = 12, DQ_P_LE = 13, DQ_P_GT = 14, DQ_P_GE = 15,
    DQ_P_EQ_NULLSAFE = 16, /* <=>                                                              */
    DQ_P_AND = 20, DQ_P_OR = 21, DQ_P_NOT = 22,
    DQ_P_IS_NULL = 23, DQ_P_IS_NOT_NULL = 24,
    DQ_P_IN = 25,        /* arg: n                     -> x IN (v1..vn); n+1 operands          */
    DQ_P_COALESCE = 26,  /* arg: n operands                                                    */
    DQ_P_ADD = 30, DQ_P_SUB = 31, DQ_P_MUL = 32, DQ_P_DIV = 33, DQ_P_MOD = 34, DQ_P_NEG = 35,
    DQ_P_LIKE = 40,      /* arg: constant index of the pattern; 1 operand                      */
    DQ_P_LENGTH = 41,    /* UTF-8 character count                                             */
    /* Spark 2.2 Cast: string -> DOUBLE is Double.parseDouble (NULL where it throws), string -> LONG is
     * UTF8String.toLong, DOUBLE -> LONG is Java's d.toLong (saturating, NaN -> 0). A string whose double needs
     * parseDouble's arbitrary-precision path (a hexadecimal literal, or more than 19 significant digits on a rounding
     * boundary) fails the dq_scan call with DQ_ERR_UNSUPPORTED, as dq_cast_column does; so does such a string in a
     * comparison with a number, in arithmetic, abs or isnan (Spark's implicit string -> double cast). */
    DQ_P_CAST_DOUBLE = 42, DQ_P_CAST_LONG = 43, DQ_P_CAST_STRING_NUM = 44,
    /* PatternMatch (A/PatternMatch.scala:46-48): arg = index of a STRING constant holding a compiled
     * java.util.regex program (deequ_amd/regex.py image, 4-byte aligned in the pool); 1 operand.
     * TRUE when the first Matcher.find() match of the value's string form is non-empty, FALSE
     * otherwise, also for NULL (`when(regexp_extract(..) != "", 1).otherwise(0)`). Only as the whole
     * program [COL c, REGEX k], over STRING / integral / BOOLEAN columns. */
    DQ_P_REGEX = 45,
    /* str RLIKE regex (Spark RLike: Pattern.compile(regex).matcher(str).find(), any match): arg = index of a STRING
     * constant holding a compiled regex program (as DQ_P_REGEX); 1 operand, a non-string one as its Spark string
     * cast. NULL in -> NULL. */
    DQ_P_RLIKE = 46,
    DQ_P_LOWER = 47, DQ_P_UPPER = 48,  /* lower(str) / upper(str): simple Unicode case mappings                 */
    DQ_P_TRIM = 49,      /* arg 0 trim, 1 ltrim, 2 rtrim (ASCII spaces, Spark 2.2 UTF8String.trim)                 */
    DQ_P_CASE = 50,      /* CASE WHEN c1 THEN v1 .. [ELSE e] END: arg = 2 * #WHEN + has ELSE; operands c1 v1 .. [e] */
    DQ_P_ISNAN = 51,     /* isnan(x): never NULL                                                                  */
    DQ_P_ABS = 52,
    DQ_P_SUBSTR = 53,    /* substring(str, pos, len): 3 operands, UTF8String.substringSQL                          */
    DQ_P_YEAR = 54, DQ_P_MONTH = 55, DQ_P_DAY = 56, /* arg 0: DATE days, 1: TIMESTAMP micros (UTC session zone)  */
    DQ_P_NANVL = 57      /* nanvl(a, b): 2 operands                                                               */
} dq_pred_opcode;

typedef enum dq_value_tag { DQ_V_BOOL = 1, DQ_V_LONG = 2, DQ_V_DOUBLE = 3, DQ_V_STRING = 4 } dq_value_tag;

typedef struct dq_const {
    int32_t tag;           /* dq_value_tag                                         */
    int32_t str_len;       /* STRING: byte length                                  */
    int64_t i64;           /* BOOL / LONG                                          */
    double f64;            /* DOUBLE                                               */
    int64_t str_offset;    /* STRING: offset into dq_predicate.strings             */
} dq_const;

typedef struct dq_predicate {
    const int32_t* code;   /* pairs (opcode, arg)                                  */
    int32_t code_len;      /* number of int32 words (2 per instruction)            */
    int32_t n_consts;
    const dq_const* consts;
    const uint8_t* strings;/* string constant pool                                 */
    int64_t strings_len;
} dq_predicate;

/* ---------------------------------------------------------------------------------------------
 * Scan-shareable ops. One dq_op per deduplicated analyzer (VerificationSuite does not dedupe,
 * M/VerificationSuite.scala:119; the host does).
 * ------------------------------------------------------------------------------------------- */
typedef enum dq_op_kind {
    DQ_OP_SIZE = 1,                 /* A/Size.scala:33-47                    -> num_matches            */
    DQ_OP_COMPLETENESS = 2,         /* A/Completeness.scala:26-46            -> num_matches_and_count  */
    DQ_OP_COMPLIANCE = 3,           /* A/Compliance.scala:37-53              -> num_matches_and_count  */
    DQ_OP_MEAN = 4,                 /* A/Mean.scala:25-54                    -> mean                   */
    DQ_OP_SUM = 5,                  /* A/Sum.scala:25-52                     -> dbl                    */
    DQ_OP_MINIMUM = 6,              /* A/Minimum.scala:25-53                 -> dbl                    */
    DQ_OP_MAXIMUM = 7,              /* A/Maximum.scala:25-53                 -> dbl                    */
    DQ_OP_STANDARD_DEVIATION = 8,   /* A/StandardDeviation.scala:25-73       -> stddev                 */
    DQ_OP_CORRELATION = 9,          /* A/Correlation.scala:26-105            -> corr                   */
    DQ_OP_APPROX_COUNT_DISTINCT = 10,/* A/ApproxCountDistinct.scala:26-64    -> hll                    */
    DQ_OP_MIN_LENGTH = 11,          /* A/MinLength.scala:25-41               -> dbl                    */
    DQ_OP_MAX_LENGTH = 12,          /* A/MaxLength.scala:25-41               -> dbl                    */
    DQ_OP_DATATYPE = 13             /* A/DataType.scala:32-183               -> datatype               */
} dq_op_kind;

typedef struct dq_op {
    int32_t kind;       /* dq_op_kind                                         */
    int32_t column[2];  /* column indices; column[1] only for CORRELATION     */
    int32_t where;      /* predicate index of the `where` filter, -1 = none   */
    int32_t predicate;  /* COMPLIANCE: predicate index; otherwise -1          */
} dq_op;

#define DQ_HLL_NUM_WORDS 52 /* DeequHyperLogLogPlusPlusUtils.NUM_WORDS, C/StatefulHyperloglogPlus.scala:154 */
#define DQ_HLL_REGISTERS 512

/* One state per op. present == 0 encodes `None` (ifNoNullsIn, A/Analyzer.scala:389-403), which
 * the host turns into EmptyStateException (A/Analyzer.scala:444-455). */
typedef struct dq_state {
    int32_t kind;
    int32_t present;
    union {
        struct { int64_t num_matches; } num_matches;                        /* NumMatches          */
        struct { int64_t num_matches; int64_t count; } num_matches_and_count;/* NumMatchesAndCount  */
        /* MeanState / SumState. For integral (non-decimal) columns Spark sums in a Long that wraps around and
         * casts the FINAL sum to Double (A/Sum.scala:34-37): `isum` keeps that exact Long partial and
         * `exact` = 1 so merges of shards / chunks (dq_state_merge, dq_state_fold) add the Longs and re-cast,
         * rather than adding rounded doubles. `sum` / `value` is always (double)isum then.
         * DQ_TYPE_DECIMAL128 columns: `exact` = 2 and `wsum` is the exact 192-bit sum of the unscaled values (three
         * little-endian 64-bit limbs, two's complement) with the column's scale in `wscale`; merges add the limbs and
         * convert again (Spark aggregates in decimal and casts once, A/Sum.scala:40). `woverflow` = 1 when the total
         * has 39 or more digits (|wsum| >= 10^38: Spark's sum type is at most decimal(38, s)); `sum` / `value` is NaN
         * then and the host fails that analyzer alone. */
        struct { double sum; int64_t count; int64_t isum; int32_t exact; int32_t pad;
                 uint64_t wsum[3]; int32_t wscale; int32_t woverflow; } mean;
        struct { double value; int64_t isum; int32_t exact; int32_t pad;
                 uint64_t wsum[3]; int32_t wscale; int32_t woverflow; } dbl;  /* Sum/Min/Max State */
        /* StandardDeviationState. DQ_TYPE_DECIMAL128 columns: `exact` = 1 and xs1 / xs2 are the exact sums of the
         * per-row doubles x and of x^2 as two's-complement integers (little-endian 64-bit limbs) in units of 2^-180
         * and 2^-360: merges add them, so any cut of the rows gives the same bits; avg / m2 are the fp64 Welford /
         * Chan values of the same rows (within 1e-12 of the exact ones). */
        struct { double n, avg, m2; uint64_t xs1[6]; uint64_t xs2[11]; int32_t exact; int32_t pad; } stddev;
        struct { double n, x_avg, y_avg, ck, x_mk, y_mk; } corr;            /* CorrelationState    */
        struct { int64_t words[DQ_HLL_NUM_WORDS]; } hll;                    /* ApproxCountDistinctState */
        struct { int64_t num_null, num_fractional, num_integral, num_boolean, num_string; } datatype;
    } u;
} dq_state;

#define DQ_SCAN_OUT_DEVICE 0x1u /* `out` is a device pointer: dq_scan returns without syncing */

/* ---------------------------------------------------------------------------------------------
 * Frequency tables (grouping analyzers). Replaces FrequencyBasedAnalyzer.computeFrequencies
 * (A/GroupingAnalyzers.scala:53-79) and the fused aggregation over the table in
 * runAnalyzersForParticularGrouping (R/AnalysisRunner.scala:480-548).
 * ------------------------------------------------------------------------------------------- */
typedef struct dq_freq_table dq_freq_table; /* device-resident (key -> count) table */

#define DQ_FREQ_INCLUDE_NULLS 0x1u /* Histogram semantics: null is a key ("NullValue"), all rows count */

typedef struct dq_freq_summary {
    int64_t num_rows;      /* rows with >= 1 non-null grouping column (A/GroupingAnalyzers.scala:73-76) */
    int64_t num_groups;    /* count(*) over the table  (CountDistinct, Distinctness numerator)         */
    int64_t num_unique;    /* sum[count == 1]          (Uniqueness, UniqueValueRatio numerator)        */
    double entropy;        /* sum over groups of -(c/N) ln(c/N), N = entropy_rows                     */
    int64_t entropy_rows;  /* the N used for `entropy`                                                 */
    int64_t max_count;
    int64_t null_count;    /* DQ_FREQ_INCLUDE_NULLS: rows whose keys are all NULL (one extra group)  */
    /* `entropy` exactly as the order-free sum it was rounded from: each group's term rounded once to
     * a signed 128-bit integer of 2^-104 units, the integers added. entropy ==
     * (double)(hi:lo) * 2^-104. Parts of a sharded table (disjoint groups) add these, not `entropy`,
     * so any split of the same groups gives the same bits. */
    uint64_t entropy_fx_lo;
    int64_t entropy_fx_hi;
} dq_freq_summary;

/* ---------------------------------------------------------------------------------------------
 * Entry points
 * ------------------------------------------------------------------------------------------- */
typedef struct dq_ctx dq_ctx;

int dq_abi_version(void);

/* Bind a context to HIP device `device`. Fails with DQ_ERR_NO_DEVICE when no GPU is visible. */
dq_ctx* dq_open(int device, int* status);
void dq_close(dq_ctx* ctx);
const char* dq_last_error(const dq_ctx* ctx);

/* One context over `ndev` GPUs of this node (multi-GPU row): dq_scan over host columns splits the
 * rows into contiguous 2048-row-aligned shards, one per device, scans them concurrently and returns the states
 * folded in device order with the reference merges (the partition merge inside R/AnalysisRunner.scala:313);
 * dq_frequencies pre-aggregates each shard on its device and exchanges the (key, count) groups by owner device
 * over RCCL (ncclSend / ncclRecv all-to-all over xGMI), so each group lives on exactly one device. The context
 * owns one RCCL communicator per device (ncclCommInitAll) when the devices are distinct; a repeated device
 * (several shards on one GPU, e.g. to test the sharded path on one card) moves the groups with device copies
 * instead. ndev == 1 runs the same sharded path with one shard. dq_quantile_summary runs its selection passes on every
 * device's shard and returns the order statistics of the whole column (the same samples as one device); dq_kll_sketch
 * sketches one partition per device and merges them in device order (QuantileNonSample.merge, as KLLRunner's reduce
 * over partitions, R/KLLRunner.scala:104-112); dq_cast_column casts every device's shard into HOST result buffers. */
dq_ctx* dq_open_devices(const int* devices, int ndev, int* status);
int dq_ctx_num_devices(const dq_ctx* ctx);
int dq_ctx_uses_rccl(const dq_ctx* ctx);   /* 1 when the context's exchange runs over RCCL */

/* dq_scan over columns already resident in HBM across the devices of a multi-device context: shard i's columns
 * (shard_columns[i][0..ncols), DQ_COL_DEVICE on device i, or host) hold shard_rows[i] rows. States come back
 * folded in device order (host memory). */
int dq_scan_sharded(dq_ctx* ctx, const dq_column* const* shard_columns, const int64_t* shard_rows, int ncols,
                    const dq_op* ops, int nops, const dq_predicate* preds, int npreds, dq_state* out);

/* Run kernels on this HIP stream (hipStream_t as void*); NULL = the context's own stream. */
int dq_set_stream(dq_ctx* ctx, void* stream);
/* (r06) HIP stream priority of the context's own stream and its internal side streams: 1 high, 0 normal, -1 low
 * (hipDeviceGetStreamPriorityRange's ends). Waits for the context's queued work. A context whose work is on a job's
 * critical path (e.g. a run submitted beside a ColumnProfiler's passes) dispatches ahead of the device's other
 * contexts. No reference counterpart (Spark's scheduler pools are the nearest analogue). */
int dq_set_priority(dq_ctx* ctx, int priority);
int dq_synchronize(dq_ctx* ctx);

/* Release the context's idle cached device scratch (the grouping builds' partition buffers and tables) beyond
 * keep_bytes, oldest first; 0 releases all of it. A context's scratch cache is locked, so this may be called from
 * any thread (a second context of the device that has finished its helper work). When an allocation fails, a
 * context also releases the idle scratch of every other context of its device before it gives up. No reference
 * counterpart: Spark's executors own their memory (host-side bookkeeping of this engine). */
void dq_scratch_trim(dq_ctx* ctx, int64_t keep_bytes);

/* The fused scan: replaces runScanningAnalyzers (R/AnalysisRunner.scala:289-336), i.e. the single
 * `data.agg(...).collect()` of all ScanShareableAnalyzer.aggregationFunctions() (:306-313) plus
 * fromAggregationResult (A/Analyzer.scala:172-175). Every column is read once from HBM.
 * `out` receives nops dq_state records (host memory unless DQ_SCAN_OUT_DEVICE). */
int dq_scan(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows,
            const dq_op* ops, int nops, const dq_predicate* preds, int npreds,
            dq_state* out, uint32_t flags);

/* dq_scan over host columns streamed through HBM in chunks of chunk_rows rows (rounded to 2048): the copy of the
 * next chunk (its own stream, double-buffered device chunks) overlaps the scan of the current one, and the chunks'
 * states are folded in row order with the reference merges — for tables larger than HBM and host-resident batches
 * (end-to-end rate bound by the host link). Host columns only; `out` is host memory. */
int dq_scan_streamed(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops,
                     const dq_predicate* preds, int npreds, dq_state* out, int64_t chunk_rows);

/* Number of fused-scan kernel launches issued so far (the analogue of the SparkMonitor job count
 * asserted in T/analyzers/runners/AnalysisRunnerTests.scala:50-74). */
int64_t dq_scan_launch_count(const dq_ctx* ctx);

/* Kernel launches of the scan path by kernel (all devices of a multi-device context), so a test can prove which
 * kernel shape evaluated its ops (tests/test_gpu_configs.py). */
typedef enum dq_scan_kernel {
    DQ_KERNEL_STRIPED = 0,        /* scan_values_kernel: count / sum / min / max / moments, striped 16-B loads     */
    DQ_KERNEL_STRIPED_HEAVY = 1,  /* scan_values_kernel HEAVY: HLL / fused compare over 1-, 2-, 4-byte columns    */
    DQ_KERNEL_HEAVY8 = 2,         /* scan_heavy8_kernel: 8-byte HLL / fused compare / Correlation pairs           */
    DQ_KERNEL_HEAVY8_FULL = 3,    /* scan_heavy8_kernel with every flag on and no `where` (the north-star suite)  */
    DQ_KERNEL_BITS = 4,           /* scan_bits_kernel: Size(where), unread Completeness, non-fused Compliance     */
    DQ_KERNEL_PRED_SIMPLE = 5,    /* pred_simple_kernel: a simple predicate into TRUE / NOT-NULL bitmaps          */
    DQ_KERNEL_PRED_VM = 6,        /* predicate_kernel: the general predicate VM                                   */
    DQ_KERNEL_REGEX = 7,          /* regex_match_kernel (PatternMatch)                                            */
    DQ_KERNEL_STRINGS = 8,        /* scan_strings_kernel                                                          */
    DQ_KERNEL_WHERE_FUSED = 9,    /* a value scan that also evaluates a `where` and writes its masks              */
    DQ_KERNEL_WHERE_MASKS = 10,   /* where_masks_kernel: a `where` into per-column masks (no fused producer)       */
    DQ_KERNEL_DECIMAL128 = 11,    /* scan_decimal128_kernel: every (DECIMAL128 column, where) slot of a call      */
    DQ_KERNEL_DICT_COUNTS = 12,   /* dict_counts_kernel: every (dictionary column, where) slot of a call          */
    DQ_KERNEL_DICT_FOLD = 13,     /* dict_fold_kernel: the per-entry fold of a dq_dict_scan call                  */
    DQ_KERNEL_DICT_DECODE = 14,   /* dq_dict_decode calls that copied bytes (a kept column handed on decoded)     */
    DQ_KERNEL_FILTER_VALIDITY = 15, /* filter_validity_kernel: a `where` ANDed into key-column validity bitmaps   */
    DQ_KERNEL_ROW_OUTCOMES = 16,  /* row_outcomes_kernel: the per-check row outcomes of one dq_row_outcomes call  */
    DQ_KERNEL_FREQ_PROBE = 17,    /* probe_kernel: another table's rows against a frequency table (dq_freq_probe)  */
    DQ_KERNEL_CSV_QUOTES = 18,    /* csv_quotes_kernel: quote counts per tile of a CSV file (dq_csv_index)         */
    DQ_KERNEL_CSV_MARK = 19,      /* csv_mark_kernel: terminator / delimiter bitmaps and the refusal checks        */
    DQ_KERNEL_CSV_ROWS = 20,      /* csv_rows_kernel: record starts                                                */
    DQ_KERNEL_CSV_FIELDS = 21,    /* csv_fields_kernel: field spans, classes and ambiguity reports                 */
    DQ_KERNEL_CSV_COLUMN = 22,    /* the per-column kernels of dq_csv_column (lengths, gather, typed parse)        */
    DQ_KERNEL_INGEST_VALIDITY = 23, /* ingest_validity_kernel: validity bitmaps of Arrow chunks concatenated bitwise  */
    DQ_KERNEL_INGEST_BOOL = 24,   /* ingest_bool_kernel: Arrow boolean bits into one byte per row                  */
    DQ_KERNEL_INGEST_OFFSETS = 25, /* ingest_offsets_kernel: string offsets of one Arrow chunk rebased into int32   */
    DQ_KERNEL_INGEST_CONVERT = 26, /* the typed conversions of dq_ingest_convert (decimal cells, timestamp units)   */
    DQ_KERNEL_INGEST_INDICES = 27, /* ingest_indices_kernel: dictionary indices widened, checked and folded         */
    DQ_KERNEL_COUNT = 28
} dq_scan_kernel;
int64_t dq_scan_kernel_launches(const dq_ctx* ctx, int32_t kernel);

/* A `where` filter as validity bitmaps, for the analyzers that take no filter argument on the device (the grouping
 * analyzers, ApproxQuantile): they skip NULL cells -- a grouping drops the rows whose key columns are all NULL -- so a
 * row the filter drops is a row whose key cells are NULL. `pred` is evaluated over `columns` (host or device columns
 * of nrows rows, as dq_scan takes them: the same validation, the same kernels, SQL three-valued logic) and, in one
 * further kernel launch, out_validity_dev[j] = TRUE(pred) & validity(columns[target_columns[j]]) for j in
 * [0, ntargets), ntargets <= 32; a target without a bitmap counts as all ones. A target need not be read by `pred`,
 * and only its validity is read (device bitmaps 8-B aligned). Every output is a device buffer, 8-B aligned,
 * LSB-first, (nrows + 63) / 64 words: EVERY word is written, and bits at and past nrows are 0 whatever the input
 * bitmaps hold there. *true_rows = the rows on which `pred` is TRUE. nrows == 0 launches nothing.
 * Status: as dq_scan for the predicate (DQ_ERR_PREDICATE, and DQ_ERR_UNSUPPORTED with dq_scan's texts for a regex past
 * its backtracking budget or a string only Double.parseDouble's arbitrary-precision path converts; the outputs are
 * then undefined); DQ_ERR_ALIGNMENT for a misaligned bitmap; DQ_ERR_UNSUPPORTED on a multi-device context. */
int dq_filter_validity(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_predicate* pred,
                       const int32_t* target_columns, int ntargets, uint8_t* const* out_validity_dev,
                       int64_t* true_rows);

/* ---------------------------------------------------------------------------------------------
 * Row-level results (VerificationResult.rowLevelResultsAsDataFrame of later deequ releases): one
 * BOOLEAN outcome column per check, the AND of its terms, written by ONE kernel launch next to the table in HBM.
 * ------------------------------------------------------------------------------------------- */
typedef enum dq_row_term_kind {
    DQ_ROW_NOT_NULL = 1,   /* Completeness: passes where columns[index] is not NULL                              */
    DQ_ROW_PREDICATE = 2,  /* Compliance / PatternMatch: passes where preds[index] is TRUE (FALSE and NULL fail) */
    DQ_ROW_BITS = 3        /* caller-supplied device bitmaps, as dq_freq_row_bits writes them (uniqueness)       */
} dq_row_term_kind;

typedef struct dq_row_term {
    int32_t kind;                    /* dq_row_term_kind                                                         */
    int32_t index;                   /* NOT_NULL: column index; PREDICATE: predicate index; BITS: not read       */
    int32_t where;                   /* predicate index of the term's `where`, -1 = none; BITS: not read         */
    int32_t check;                   /* index of the check the term belongs to                                   */
    const uint8_t* pass_bits;        /* BITS: rows that pass; device, 8-B aligned, (nrows + 63) / 64 words       */
    const uint8_t* considered_bits;  /* BITS: rows the term considers; the same shape                            */
} dq_row_term;

typedef struct dq_row_check {
    uint8_t* pass_bits;  /* out: rows whose outcome is TRUE; device, 8-B aligned, (nrows + 63) / 64 words            */
    uint8_t* values;     /* out: the BOOLEAN column, one byte per row; device, 16-B aligned, nrows rounded up to 16 B */
    uint8_t* validity;   /* out, DQ_ROW_FILTERED_NULL only: rows whose outcome is not NULL; shaped as pass_bits      */
} dq_row_check;

#define DQ_ROW_FILTERED_NULL 0x1u /* a row a term does not consider is NULL (default: it passes) */
#define DQ_ROW_MAX_TERMS 64
#define DQ_ROW_MAX_CHECKS 16

/* The outcome of every row under every check. Term t considers the rows on which its `where` is TRUE (every row
 * without one; a BITS term the rows of considered_bits) and passes the considered rows on which its source holds.
 * term_counts[2 t] = rows considered and passed (`matched`), term_counts[2 t + 1] = rows considered: for NOT_NULL and
 * PREDICATE terms exactly the NumMatchesAndCount that dq_scan returns for Completeness / Compliance under the same
 * `where`. A check's outcome on a row is the AND of its terms (no terms: TRUE):
 *   default               a term a row is not considered by passes it. TRUE unless a term fails; no validity bitmap.
 *   DQ_ROW_FILTERED_NULL  such a term is NULL there; SQL three-valued AND: FALSE if any term fails, else NULL if any
 *                         term is NULL, else TRUE. checks[c].validity is written.
 * check_counts[2 c] = TRUE rows, check_counts[2 c + 1] = NULL rows (0 without the flag); the FALSE rows are the rest.
 * `columns` / `preds` are host or device columns of nrows rows and predicates as dq_scan takes them (the same
 * validation, SQL three-valued logic, the same predicate kernels -- but `column <op> constant` over a numeric column,
 * which dq_scan fuses into a value scan, is evaluated by the row_outcomes launch itself, so the call issues no more
 * predicate launches than a scan); every predicate of `preds` is evaluated exactly once, whatever
 * the number of terms and filters that name it, and only the validity of a NOT_NULL column is read (device bitmaps 8-B
 * aligned). Outputs: EVERY word of pass_bits / validity is written, bits at and past nrows are 0 whatever the inputs
 * hold there; values[i] is 0 / 1 for i < nrows (0 where the outcome is FALSE or NULL) and 0 from nrows up to the next
 * multiple of 16. term_counts (2 * nterms) and check_counts (2 * nchecks) are host memory. nrows == 0 launches nothing.
 * Status: as dq_scan for the predicates (the outputs are then undefined); DQ_ERR_UNSUPPORTED for more than
 * DQ_ROW_MAX_TERMS terms or DQ_ROW_MAX_CHECKS checks (the caller splits by check) and on a multi-device context;
 * DQ_ERR_ALIGNMENT for a misaligned bitmap or a values buffer not 16-B aligned; DQ_ERR_INVALID_ARGUMENT for an index out
 * of range, a missing buffer, or a NOT_NULL column whose length is not nrows. */
int dq_row_outcomes(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_predicate* preds, int npreds,
                    const dq_row_term* terms, int nterms, const dq_row_check* checks, int nchecks, uint32_t flags,
                    int64_t* term_counts, int64_t* check_counts);

/* ---------------------------------------------------------------------------------------------
 * Dictionary-encoded STRING columns (Arrow dictionary<values=string, indices=int32>, as parquet writes categorical
 * strings): kept encoded on the GPU. Every answer below is a function of the dictionary entries and of how many rows
 * under the `where` point at each entry, so the per-row pass is a 4-byte index histogram (dict_counts_kernel) and
 * lengths, DataType classes, XXH64 and predicates run once per entry. Single-device contexts, device buffers.
 *   - Row i is NULL iff its validity bit is clear. The caller folds rows that point at a NULL entry into the bitmap;
 *     the index of a NULL row is not read as an address but must be readable memory.
 *   - `dictionary` is a STRING dq_column of n_dict + 1 entries (int32 offsets, a validity bitmap, bytes 4-B aligned
 *     with >= 16 readable bytes past the end): entries [0, n_dict) are the dictionary -- duplicates, unused entries,
 *     NULL entries and the empty string are fine -- and entry n_dict is NULL. It stands for the NULL rows when a
 *     predicate is evaluated once per entry (`c IS NULL` is TRUE there).
 *   - An index outside [0, n_dict) on a non-NULL row fails the call with DQ_ERR_INVALID_ARGUMENT; it is never used as
 *     an address.
 * ------------------------------------------------------------------------------------------- */
typedef struct dq_dict_column {
    uint32_t flags;            /* DQ_COL_DEVICE (required)                                       */
    uint32_t pad;
    int64_t length;            /* rows                                                           */
    const int32_t* indices;    /* `length` indices, 4-B aligned                                  */
    const uint8_t* validity;   /* Arrow LSB-first bitmap, 8-B aligned and whole 8-byte words, or NULL */
    dq_column dictionary;      /* see above: length = n_dict + 1                                 */
} dq_dict_column;

/* The states dq_scan would write over the decoded columns, from one dict_counts_kernel launch over every
 * (dictionary column, where) slot of the call plus one per-entry fold. ops[i].column[0] = ncols + d names dicts[d].
 * Kinds: COMPLETENESS, MIN_LENGTH, MAX_LENGTH, APPROX_COUNT_DISTINCT, DATATYPE, and COMPLIANCE whose predicate reads
 * only that dictionary column and constants (every DQ_P_COL of it is taken as the dictionary column, whatever its
 * arg; [COL, REGEX] programs are PatternMatch): the predicate is evaluated over the n_dict + 1 entries by the kernels
 * dq_scan uses, and the counts are summed under its TRUE bitmap. ops[i].where indexes `preds` and reads `columns`
 * (plain device columns of nrows rows) only. `out` is host memory. Anything else: DQ_ERR_UNSUPPORTED. */
int dq_dict_scan(dq_ctx* ctx, const dq_column* columns, int ncols, const dq_dict_column* dicts, int ndicts, int64_t nrows,
                 const dq_op* ops, int nops, const dq_predicate* preds, int npreds, dq_state* out);

/* counts_dev[e] (n_dict int64, device) = non-NULL rows of `dict` that point at entry e; rows[0] = the column's rows,
 * rows[1] = its non-NULL rows (host). The grouping analyzers over one dictionary column build their frequency table
 * from (entries with a count > 0, counts) with dq_frequencies_ex weights; duplicate entries add up there. Exact
 * (integer atomics), also past 2^32 rows per entry. DQ_DICT_LDS_ENTRIES (read per call, default 16384, at most 16384):
 * dictionaries of up to that many entries count in workgroup-private LDS counters, larger ones with 64-bit global
 * atomics. DQ_DICT_LDS_COPIES (1, 2 or 4; measurements only) lowers the number of LDS counter copies from 8. */
int dq_dict_counts(dq_ctx* ctx, const dq_dict_column* dict, int64_t* counts_dev, int64_t* rows);

/* Decode on the device: the plain STRING column of the same rows. Two calls, as dq_gather_rows: with out_values ==
 * NULL, writes out_offsets (length + 1 int32, device; a NULL row is empty) and *out_bytes; then with out_values
 * (>= *out_bytes + 16 bytes) and the same out_offsets, copies the bytes and zeroes the 16 bytes after them. The rows'
 * validity bitmap is the dictionary column's own. DQ_ERR_UNSUPPORTED when the decoded bytes would reach 2^31. */
int dq_dict_decode(dq_ctx* ctx, const dq_dict_column* dict, int32_t* out_offsets, void* out_values, int64_t* out_bytes);

/* Which grouping build produced the frequency tables of this context so far (all devices of a multi-device
 * context), so a test can prove which path it checked against the oracle (tests/test_gpu_grouping_oracle.py). */
typedef enum dq_freq_path {
    DQ_FREQ_PATH_FAST = 0,              /* fast build pass 1 (partition1_fast) over 64-bit keys                */
    DQ_FREQ_PATH_FAST_NARROW = 1,       /* fast build pass 1 over 32-bit offsets around a sampled base         */
    DQ_FREQ_PATH_FAST_DONE = 2,         /* fast builds that produced their table (no exact-path fallback)      */
    DQ_FREQ_PATH_EXACT = 3,             /* exactly-counted path (extract_count + digit histograms)             */
    DQ_FREQ_PATH_PARTITIONED = 4,       /* exact path: radix partition passes (partition1 / scatter2)          */
    DQ_FREQ_PATH_SORTED = 5,            /* exact path: keys sorted on the bucket bits                          */
    DQ_FREQ_PATH_SMALL = 6,             /* one-pass small builds launched (sized or optimistic)                */
    DQ_FREQ_PATH_SMALL_OPTIMISTIC = 7,  /* optimistic small builds (no sizing pass) that produced their table  */
    DQ_FREQ_PATH_FAST_SPILL = 8,        /* fast builds whose full buckets spilled keys (inserted after the build) */
    DQ_FREQ_PATH_SPLIT_BUCKETS = 9,     /* builds with buckets split over several work items (atomic merge)    */
    DQ_FREQ_PATH_LONG_TUPLES = 10,      /* general builds of one string key column with keys past 15 bytes     */
                                        /* (two-word tuples for the short keys, byte compares for the rest)    */
    DQ_FREQ_PATH_COUNT = 11
} dq_freq_path;
int64_t dq_freq_path_count(const dq_ctx* ctx, int32_t path);

/* Semigroup merge of two states of the same op kind (State.sum, per analyzer file);
 * also used for the rank-ordered fold after the RCCL all-gather. */
int dq_state_merge(const dq_state* a, const dq_state* b, dq_state* out);

/* Rank-ordered fold of nparts x nops states (part-major, e.g. an all-gather of per-rank dq_scan outputs):
 * out[i] = states[0][i] + states[1][i] + ... with dq_state_merge, deterministic for every rank count. */
int dq_state_fold(const dq_state* states, int nparts, int nops, dq_state* out);

/* DeequHyperLogLogPlusPlusUtils.count (C/StatefulHyperloglogPlus.scala:210-257), including the
 * Java int-shift quirk `1 << Midx` and precision-9 bias correction; returns the rounded estimate. */
double dq_hll_count(const int64_t words[DQ_HLL_NUM_WORDS]);

/* Spark XxHash64Function.hash(value, type, 42) for one fixed-width value (test hook). DQ_TYPE_DECIMAL128: `value`
 * points to the 16-byte cell; the hash is XXH64 over unscaledValue().toByteArray (minimal big-endian bytes). */
int64_t dq_spark_hash64(int32_t spark_type, const void* value, int64_t len);

/* Decimal.toDouble of one DQ_TYPE_DECIMAL128 cell (16 bytes at `value`): the double nearest to unscaled * 10^-scale,
 * ties to even, 0 <= scale <= 38. Host only; the same code as the scan kernel and the cast. */
double dq_dec128_to_double(const void* value, int32_t scale);

/* Build the (key -> count) table of the given key columns (computeFrequencies). */
int dq_frequencies(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows,
                   const int32_t* key_columns, int nkeys, uint32_t flags, dq_freq_table** table);
/* Fused aggregation over the table (Uniqueness/Distinctness/UniqueValueRatio/Entropy/CountDistinct);
 * entropy_rows <= 0 means "use this table's num_rows". */
int dq_freq_summarize(dq_ctx* ctx, const dq_freq_table* table, int64_t entropy_rows, dq_freq_summary* out);
/* How exported groups are identified: DQ_FREQ_KEYS_VALUES = the canonical 64-bit key of the single
 * fixed-width key column (integers sign-extended, FLOAT/DOUBLE bit patterns with NaN canonical),
 * DQ_FREQ_KEYS_ROWS = the smallest row index of the group (multi-column or string keys). */
#define DQ_FREQ_KEYS_VALUES 0
#define DQ_FREQ_KEYS_ROWS 1
int dq_freq_key_kind(const dq_freq_table* table);
/* Export up to k (key, count) pairs with the largest counts (Histogram top-N, A/Histogram.scala:76-78).
 * Ties are broken by slot order (deterministic). Returns the number written, < 0 on error. */
int64_t dq_freq_top(dq_ctx* ctx, const dq_freq_table* table, int64_t k, int64_t* keys, int64_t* counts);
/* Export the whole table (every group's key and count). Returns the number written, < 0 on error. */
int64_t dq_freq_export(dq_ctx* ctx, const dq_freq_table* table, int64_t capacity, int64_t* keys, int64_t* counts);
void dq_freq_free(dq_ctx* ctx, dq_freq_table* table);

/* Build options: Histogram semantics, and pre-aggregated input (each row stands for weights[row] rows: the
 * partial tables of a sharded computeFrequencies, or persisted (key, count) states). */
typedef struct dq_freq_options {
    uint32_t flags;          /* DQ_FREQ_INCLUDE_NULLS                                                  */
    uint32_t weights_device; /* 1: `weights` is a device pointer on the ctx's GPU                       */
    const int64_t* weights;  /* nrows counts (>= 0), NULL = every row counts once                       */
    int32_t key_type;        /* declared Spark type of the single key column's canonical values, 0 = its own */
    int32_t pad;
} dq_freq_options;
int dq_frequencies_ex(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const int32_t* key_columns,
                      int nkeys, const dq_freq_options* options, dq_freq_table** table);
/* dq_frequencies_ex over a table held as row-range parts read where they lie (the row chunks of a ChunkedTable, no
 * concatenation): parts[p * ncols + c] is column c's part p, device columns with int32 offsets; the table's rows are
 * the parts in order (exported representative rows are indices into that order). Two parts on a one-device context,
 * unweighted (r06); other shapes return DQ_ERR_UNSUPPORTED and the caller concatenates. The fast fixed-width build
 * reads one part only, so a fixed-width single key takes the general path here. */
int dq_frequencies_parts(dq_ctx* ctx, const dq_column* parts, int nparts, int ncols, const int32_t* key_columns,
                         int nkeys, const dq_freq_options* options, dq_freq_table** table);

/* Every group of a DQ_FREQ_KEYS_VALUES table as (canonical key, count) into device arrays (the NULL group of a
 * DQ_FREQ_INCLUDE_NULLS table is summary.null_count, not exported). Returns the number written or < 0. */
int64_t dq_freq_export_device(dq_ctx* ctx, const dq_freq_table* table, int64_t capacity, int64_t* keys_dev,
                              int64_t* counts_dev);

#define DQ_FREQ_PAIRS_DEVICE 0x1u /* keys / counts of dq_freq_from_pairs are device pointers */
/* A DQ_FREQ_KEYS_VALUES table from (canonical key, count) pairs — duplicates are added — with the state's numRows
 * and NULL-group count: the persisted frequency states of HdfsStateProvider (A/StateProvider.scala:137-160) and
 * the groups exchanged between shards. */
int dq_freq_from_pairs(dq_ctx* ctx, int32_t key_spark_type, const int64_t* keys, const int64_t* counts, int64_t n,
                       uint32_t flags, int64_t num_rows, int64_t null_count, dq_freq_table** table);

/* FrequenciesAndNumRows.sum (A/GroupingAnalyzers.scala:127-147): null-safe full outer join on the key, counts
 * added, numRows added — on the GPU, for two DQ_FREQ_KEYS_VALUES tables of the same key type. */
int dq_freq_merge(dq_ctx* ctx, const dq_freq_table* a, const dq_freq_table* b, dq_freq_table** out);

/* MutualInformation.computeMetricFrom (A/MutualInformation.scala:35-97): joint = the (x, y) table, x / y = the
 * single-column tables of the same rows (their counts are the marginals of the joint table's non-NULL keys).
 * *mi = sum over joint groups with both keys non-NULL of (pxy/N) ln((pxy/N) / ((px/N)(py/N))), N = joint numRows;
 * *present = 0 when no group joins (the reference's NULL sum -> empty state). The three tables are built over the
 * same rows: all unweighted, or all weighted by the same per-row counts (dq_frequencies_ex over a state's groups). */
int dq_freq_mutual_information(dq_ctx* ctx, const dq_freq_table* joint, const dq_freq_table* x,
                               const dq_freq_table* y, double* mi, int32_t* present);

/* Per row of the table's own source (the nrows rows it was built over by dq_frequencies / dq_frequencies_ex): the
 * count of the row's group, 0 for a row that takes no part (all key columns NULL without DQ_FREQ_INCLUDE_NULLS) —
 * the join of the rows with their frequency table, as MutualInformation joins the joint groups with the marginal
 * tables (A/MutualInformation.scala:50-74); the sharded MutualInformation attaches px / py to exchanged groups
 * with it. `counts` holds nrows entries (a device pointer with DQ_FREQ_PAIRS_DEVICE). */
int dq_freq_row_counts(dq_ctx* ctx, const dq_freq_table* table, int64_t* counts, int64_t nrows, uint32_t flags);

/* The same join as two bits per row instead of an 8-byte count: bit i of unique_bits_dev = row i's group has count 1
 * (the row is unique under the table's keys), bit i of part_bits_dev = its group has a count > 0 (the row takes part:
 * some key column is not NULL). Both are device buffers, 8-B aligned, LSB-first, (nrows + 63) / 64 words; EVERY word is
 * written, and bits at and past nrows are 0. One wave takes 64 consecutive rows and stores the two ballot words; the
 * outputs are the pass / considered bitmaps of a DQ_ROW_BITS term. The table and nrows as dq_freq_row_counts takes them,
 * with its errors (a single-device table built over rows that still has its slot table: DQ_ERR_UNSUPPORTED otherwise;
 * nrows must be the table's source rows); DQ_ERR_ALIGNMENT for a misaligned bitmap. nrows == 0 launches nothing. */
int dq_freq_row_bits(dq_ctx* ctx, const dq_freq_table* table, uint8_t* unique_bits_dev, uint8_t* part_bits_dev,
                     int64_t nrows);

/* Semi-join probe. For each of `nrows` rows of `columns`: does its key (key_columns[0..nkeys), paired by
 * position with the key columns `t` was built over) equal a key of `t` under SQL '='?
 * match_bits_dev: optional device bitmap, 8-byte aligned, (nrows+63)/64 words, bits past nrows clear.
 * outcome_dev:    optional device bytes, one 0/1 byte per row (the cells of a BOOLEAN column).
 * matched:        the number of matching rows.
 * A NULL component on either side never matches (the table's own grouping is null-safe; the probe is not). `t` is a
 * single-device table; over general keys (strings, several columns) it must still have its source rows, which the
 * probe compares with. The probe columns are host buffers (staged for the call) or DQ_COL_DEVICE. Type pairs: the
 * same Spark type; any two of BYTE / SHORT / INT / LONG (by value); DECIMAL of one scale. DQ_ERR_UNSUPPORTED: a
 * FLOAT / DOUBLE / DECIMAL128 pair or any other, a multi-device table or context, a DQ_FREQ_INCLUDE_NULLS table over
 * one STRING column (it counts NULL as "NullValue"). DQ_ERR_INVALID_ARGUMENT: nkeys differs from the table's key
 * count. nrows == 0 launches nothing. One launch (probe_kernel), counted under DQ_KERNEL_FREQ_PROBE. */
int dq_freq_probe(dq_ctx*, const dq_freq_table* t, const dq_column* columns, int ncols, int64_t nrows,
                  const int32_t* key_columns, int nkeys, uint8_t* match_bits_dev, uint8_t* outcome_dev,
                  int64_t* matched);

/* ApproxQuantile / ApproxQuantiles (A/ApproxQuantile.scala:28-103, A/ApproxQuantiles.scala:39-101): replaces the
 * per-row PercentileDigest.add of StatefulApproxQuantile.update (C/StatefulApproxQuantile.scala:65-72). Computes
 * EXACT order statistics of the column's non-NULL values cast to double, in java.lang.Double.compare order
 * (-0.0 < 0.0, NaN largest), at 1-based ranks 1, n and every max(1, floor(relative_error * n))-th rank in between:
 * the samples (value, g = rank gap, delta = 0) of a Greenwald-Khanna summary with no rank uncertainty, from which
 * the host builds Spark's QuantileSummaries / PercentileDigest (relative_error = 0 returns all n sorted values).
 * Numeric columns only (Preconditions.isNumeric). values_out / ranks_out hold max_samples entries (2/relative_error
 * + 2 always suffices when relative_error * n >= 1; n otherwise). *count receives n. Returns the number of samples
 * written (0 for an empty or all-NULL column), or a negative dq_status. */
int64_t dq_quantile_summary(dq_ctx* ctx, const dq_column* column, int64_t nrows, double relative_error,
                            int64_t max_samples, double* values_out, int64_t* ranks_out, int64_t* count_out);

/* Several ApproxQuantile summaries at once — the ApproxQuantile(s) analyzers of one analysis run over one shard,
 * each column given as one or more consecutive row ranges ("parts": the chunks of a ChunkedTable, read where they
 * lie, no concatenation). Request r summarises parts[part_begin[r] .. part_begin[r+1]) (same type; each part's own
 * `length` rows) at relative_error[r]: values_out / ranks_out + r * max_samples receive exactly the samples
 * dq_quantile_summary returns for those parts concatenated, counts_out[r] = n, samples_out[r] = their number.
 * One host round trip for all requests (A/ApproxQuantile.scala:28-103 via the runner's batched aggregation,
 * R/AnalysisRunner.scala:289-336). A multi-device context takes one part per request. Returns 0 or a negative
 * dq_status. */
int dq_quantile_summaries(dq_ctx* ctx, const dq_column* parts, const int32_t* part_begin, int nreq,
                          const double* relative_error, int64_t max_samples, double* values_out, int64_t* ranks_out,
                          int64_t* counts_out, int64_t* samples_out);

/* KLLSketch (A/KLLSketch.scala:82-176) as KLLRunner.computeKLLSketchesInExtraPass builds it
 * (R/KLLRunner.scala:91-179): replaces the per-row QuantileNonSample.update loop of sketchPartitions for ONE
 * partition whose non-NULL values (cast to double) arrive in row order. Writes the KLLState bytes
 * (A/KLLSketch.scala:56-66: min f64, max f64, then the KLLSketchSerializer layout,
 * A/catalyst/KLLSketchSerializer.scala:60-80; all big-endian) to state_out when they fit in `capacity`, and
 * returns their length (call again with a larger buffer when the return value exceeds capacity), or a negative
 * dq_status. BYTE/SHORT/INT/LONG/FLOAT/DOUBLE columns only (other types: DQ_ERR_UNSUPPORTED, as
 * KLLRunner.emptySketches throws). NaN items are stored canonical. */
int64_t dq_kll_sketch(dq_ctx* ctx, const dq_column* column, int64_t nrows, int32_t sketch_size,
                      double shrinking_factor, uint8_t* state_out, int64_t capacity);

/* The KLL extra pass over several columns of one table at once (R/KLLRunner.scala:91-112 sketches every KLL column
 * in one pass over the partitions): column i's KLLState bytes, exactly those of dq_kll_sketch, go to
 * state_out + (sum of sizes[0..i)) and sizes[i] receives their length. Returns the total length (nothing is written
 * when it exceeds `capacity`: call again with a larger buffer) or a negative dq_status. The columns' compaction
 * schedules are computed on parallel host threads; the NULL-compaction passes and every compaction level (per kernel
 * class) are one launch each over all the columns, with one host round trip for all of them. */
int64_t dq_kll_sketch_columns(dq_ctx* ctx, const dq_column* columns, int32_t ncols, int64_t nrows, int32_t sketch_size,
                              double shrinking_factor, uint8_t* state_out, int64_t capacity, int64_t* sizes);

/* KLLState.sum of two serialized KLLState byte strings (A/KLLSketch.scala:49-54: QuantileNonSample.merge,
 * A/QuantileNonSample.scala:218-234, then condense until the sketch fits; java max / min of the extremes) — the
 * partition sketches of KLLRunner's treeReduce (R/KLLRunner.scala:104-112) and the row chunks of a chunked table.
 * Host only (no context, no device). Writes the merged state to `out` when it fits in `capacity` and returns its
 * length, or DQ_ERR_INVALID_ARGUMENT for malformed input. */
int64_t dq_kll_merge_states(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb, uint8_t* out, int64_t capacity);

/* ColumnProfiler.castColumn (M/profiles/ColumnProfiler.scala:346-355): Spark 2.2 Cast of a column to LONG or
 * DOUBLE. STRING sources: UTF8String.toLong (no trimming, optional sign, digits, optional '.' + digits truncated,
 * overflow NULL) / java.lang.Double.parseDouble (correctly rounded); strings that do not parse become NULL.
 * Numeric sources: integers sign-extend / convert, FLOAT/DOUBLE -> LONG as Java's (long) (NaN 0, saturating),
 * DECIMAL(p <= 18) and DECIMAL128 -> Decimal.toLong (truncating, low 64 bits) / Decimal.toDouble, BOOLEAN -> 0/1. values_dev receives nrows x 8 B,
 * validity_dev ceil(nrows / 64) x 8 B (LSB-first bitmap); both device memory, 8-B aligned. Returns DQ_OK, or
 * DQ_ERR_UNSUPPORTED when a string needs Double.parseDouble's arbitrary-precision path (hexadecimal literal, or
 * more than 19 significant digits on a rounding boundary) — never a silent guess. On a multi-device context
 * (dq_open_devices) the column is a host column and values_dev / validity_dev are HOST buffers of the same sizes. */
int dq_cast_column(dq_ctx* ctx, const dq_column* column, int64_t nrows, int32_t to_type, void* values_dev,
                   uint8_t* validity_dev);

/* ---------------------------------------------------------------------------------------------
 * Row-level schema validation (schema/RowLevelSchemaValidator.scala:183-281): one fused verdict
 * pass over STRING columns, then a row compaction. Single-device contexts, device-resident columns.
 * ------------------------------------------------------------------------------------------- */
typedef enum dq_schema_kind {
    DQ_SCHEMA_STRING = 1,    /* min / max: UTF-8 character counts; program: a regex image (deequ_amd/regex.py) */
    DQ_SCHEMA_INT = 2,       /* cast(c as int); min / max: value bounds (int32 range)                          */
    DQ_SCHEMA_DECIMAL = 3,   /* cast(c as decimal(precision, scale)), 0 <= scale <= precision <= 18            */
    DQ_SCHEMA_TIMESTAMP = 4  /* unix_timestamp(c, mask); program: the compiled mask (see below)               */
} dq_schema_kind;

/* One column definition. `program` is host memory: for STRING the compiled regex (program_len 0 = no `matches`), for
 * TIMESTAMP the mask as a byte program of elements {0, b} = the literal byte b and {1..6} = the fields yyyy MM dd HH
 * mm ss (each at most once, never two in a row). cast_values / cast_validity (INT: nrows x int32, DECIMAL: nrows x
 * int64 unscaled, TIMESTAMP: nrows x int64 microseconds UTC; validity ceil(nrows / 64) x 8 B) are device buffers,
 * 8-B aligned, written for every row (NULL where the cell is NULL or does not cast); either may be NULL. */
typedef struct dq_schema_column {
    int32_t kind;              /* dq_schema_kind                                  */
    int32_t column;            /* index into `columns`: a STRING column           */
    int32_t nullable;          /* 0 adds the clause `c IS NOT NULL`               */
    int32_t has_min, has_max;
    int32_t precision, scale;  /* DECIMAL                                         */
    int32_t program_len;       /* bytes                                           */
    int64_t min_value, max_value;
    const void* program;
    void* cast_values;
    uint8_t* cast_validity;
} dq_schema_column;

typedef struct dq_schema_result {
    int64_t num_valid;               /* rows whose verdict is TRUE                                          */
    int64_t num_invalid;             /* FALSE                                                               */
    int64_t num_unknown;             /* NULL: a NULL cell of an INT column with a minimum (reference :246)  */
    int64_t num_ambiguous;           /* rows with a cell whose JVM parse this engine does not reproduce     */
    int32_t first_ambiguous_column;  /* `column` of the first definition with such a cell, or -1            */
    int32_t pad;
} dq_schema_result;

#define DQ_SCHEMA_AMBIGUOUS_NULL 0x1u /* an ambiguous cell casts to NULL (default: the call fails) */

/* The verdict of every row under `defs` (SQL three-valued AND of the reference's CNF clauses, in definition order) in
 * one kernel launch, with the casts of the INT / DECIMAL / TIMESTAMP definitions. true_bits / false_bits /
 * ambiguous_bits: device bitmaps of ceil(nrows / 64) x 8 B (LSB-first), any may be NULL (counts only). String bytes
 * buffers are 4-B aligned with >= 16 readable bytes past the end. Ambiguous cells (a byte >= 0x80 in a DECIMAL /
 * TIMESTAMP cell, a decimal exponent past +-10000, a timestamp that SimpleDateFormat's lenient parse may accept but
 * is not exactly the mask's shape with in-range fields) fail the call with DQ_ERR_UNSUPPORTED — `result` is filled
 * — unless flags has DQ_SCHEMA_AMBIGUOUS_NULL. */
int dq_schema_validate(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_schema_column* defs,
                       int ndefs, uint32_t flags, uint8_t* true_bits, uint8_t* false_bits, uint8_t* ambiguous_bits,
                       dq_schema_result* result);
/* Verdict-kernel launches of this context so far (one per call with rows and definitions). */
int64_t dq_schema_launch_count(const dq_ctx* ctx);

/* The rows of one device column whose bit is set in select_bits (device, ceil(nrows / 64) x 8 B), in row order;
 * nselected must equal the number of set bits. Fixed width: out_values receives nselected elements, out_validity
 * (may be NULL) ceil(nselected / 64) x 8 B. STRING: two calls — with out_values == NULL, writes out_offsets
 * (nselected + 1 int32, device), out_validity and *out_bytes; then with out_values (>= *out_bytes + 16 bytes) and the
 * same out_offsets, copies the bytes and zeroes the 16 bytes after them. */
int dq_gather_rows(dq_ctx* ctx, const dq_column* column, int64_t nrows, const uint8_t* select_bits, int64_t nselected,
                   void* out_values, uint8_t* out_validity, int32_t* out_offsets, int64_t* out_bytes);

/* The validator's casts of one cell, host only (no context, no device): 1 = value (written to *out), 0 = NULL,
 * 2 = ambiguous. */
int dq_parse_int32(const uint8_t* s, int32_t n, int32_t* out);
int dq_parse_decimal(const uint8_t* s, int32_t n, int32_t precision, int32_t scale, int64_t* out);
int dq_parse_timestamp(const uint8_t* program, int32_t program_len, const uint8_t* s, int32_t n, int64_t* out);

/* ---- CSV files parsed on the device (Table.from_csv(path, device=...)) -----------------------------------------------
 * The dialect is Python's csv.reader default: ',' delimiter, '"' quote, a doubled quote as the escape. With q(i) the
 * number of '"' bytes before byte i, a byte is outside quotes when q(i) is even; outside quotes ',' ends a field and LF
 * or CR LF ends a record. A field whose first byte is '"' is quoted: its value is the bytes between the enclosing
 * quotes with "" collapsed. A record of zero bytes is a row of NULL cells; the bytes after the last terminator are a
 * record when there is at least one; an empty field is NULL, a missing field is NULL, fields past ncols are dropped.
 * Input is taken to be UTF-8 and is not validated.
 *
 * Input that csv.reader reads leniently is refused: the call returns DQ_OK with refusal_kind != 0, the byte offset of
 * the first occurrence (the smallest offset; the lower kind on a tie) and no handle. */
#define DQ_CSV_TILE_BYTES 16384 /* bytes one workgroup of the tokenizer takes */
typedef enum dq_csv_refusal {
    DQ_CSV_OK = 0,
    DQ_CSV_QUOTE_IN_FIELD = 1,     /* an opening quote (q even) not at the start of the file or after ',', LF, '"'  */
    DQ_CSV_TEXT_AFTER_QUOTE = 2,   /* a closing quote (q odd) not before the end of the file, ',', LF, CR LF, '"'   */
    DQ_CSV_LONE_CR = 3,            /* a CR outside quotes that no LF follows                                       */
    DQ_CSV_UNTERMINATED_QUOTE = 4  /* an odd number of quotes; the offset is that of the file's last quote          */
} dq_csv_refusal;
/* The class of one field's value, the host's _csv_field_type (Spark 2.2 CSVInferSchema): [+-]?[0-9]+ is INT, LONG or
 * DOUBLE by value range; [+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)? and the literals NaN, Infinity, -Infinity
 * are DOUBLE; a case-insensitive true / false is BOOLEAN; anything else is STRING. A value with a byte >= 0x80 or
 * ending in LF is AMBIGUOUS (Python's \d and $ accept more than ASCII digits): it is counted, not classified. */
#define DQ_CSV_CLASS_INT 1
#define DQ_CSV_CLASS_LONG 2
#define DQ_CSV_CLASS_DOUBLE 4
#define DQ_CSV_CLASS_BOOLEAN 8
#define DQ_CSV_CLASS_STRING 16
typedef struct dq_csv dq_csv; /* the index of one file: 8 bytes of device memory per (row, column) */
typedef struct dq_csv_result {
    int64_t nrows;          /* records after the skipped ones */
    int32_t refusal_kind;   /* dq_csv_refusal */
    int32_t reserved;
    int64_t refusal_offset; /* byte offset of the refusal */
} dq_csv_result;
typedef struct dq_csv_column_report {
    int32_t classes;             /* OR of DQ_CSV_CLASS_* over the column's unambiguous non-NULL fields */
    int32_t reserved;
    int64_t valid;               /* non-NULL fields */
    int64_t ambiguous;           /* ambiguous fields */
    int64_t first_ambiguous_row; /* the smallest row holding one, -1 without */
} dq_csv_column_report;
/* Index the nbytes (1 .. 2^31 - 1) of a file at `bytes` (device memory, 16-B aligned, no padding needed; it must stay
 * alive and unchanged until dq_csv_free): records, the first ncols field spans of every record after the first
 * skip_records (0 or 1: the header), and `reports` (ncols entries, host). Kernel launches do not depend on the input:
 * one each of DQ_KERNEL_CSV_QUOTES, _MARK, _ROWS and _FIELDS (the last two not for a refused file, the last not for a
 * file without rows). Single-device contexts only (DQ_ERR_UNSUPPORTED otherwise). */
int dq_csv_index(dq_ctx* ctx, const uint8_t* bytes, int64_t nbytes, int32_t ncols, int32_t skip_records, dq_csv** out,
                 dq_csv_result* result, dq_csv_column_report* reports);
/* One field of the index: the offset of its first content byte (after an opening quote), its unquoted length (0 =
 * NULL) and whether the content holds "" pairs to collapse. Host outputs; one 8-byte copy from the device. */
int dq_csv_field(dq_ctx* ctx, const dq_csv* csv, int64_t row, int32_t col, int64_t* start, int32_t* length,
                 int32_t* escaped);
/* Column `col` as spark_type. out_validity (device, ceil(nrows / 64) x 8 B, may be NULL) receives every word, bits at
 * and past nrows 0. DQ_TYPE_STRING: two calls, as dq_gather_rows: with out_values == NULL, writes out_offsets
 * (nrows + 1 int32, device), out_validity and *out_bytes; then with out_values (>= *out_bytes + 16 bytes) and the same
 * out_offsets, writes the unquoted bytes and zeroes the 16 bytes after them. DQ_TYPE_INT / LONG / DOUBLE / BOOLEAN
 * (int32 / int64 / double / one 0-1 byte per row, NULL cells 0): one call; every non-NULL field must be of a class the
 * type holds (reports). A DOUBLE is the correctly rounded value (dq_parse.h); a cell whose rounding the device cannot
 * decide (more than 19 significant digits on a boundary) fails the call with DQ_ERR_UNSUPPORTED. One launch per call,
 * counted under DQ_KERNEL_CSV_COLUMN. */
int dq_csv_column(dq_ctx* ctx, const dq_csv* csv, int32_t col, int32_t spark_type, void* out_values, uint8_t* out_validity,
                  int32_t* out_offsets, int64_t* out_bytes);
void dq_csv_free(dq_ctx* ctx, dq_csv* csv);

/* ---- CSV bodies written on the device (Table.to_csv of a device-resident table) ------------------------
 * The dialect is the reader's above. Every record, the last included, ends with LF (never CR LF); cells are separated
 * by ','. A NULL cell is zero bytes. A non-NULL cell is Spark 2.2's Cast(x AS STRING): BOOLEAN true / false; BYTE,
 * SHORT, INT, LONG decimal digits; FLOAT / DOUBLE Float.toString / Double.toString (shortest round-trip digits);
 * DECIMAL (precision <= 18) BigDecimal.toString; DATE yyyy-MM-dd; TIMESTAMP timestampToString in a UTC session zone.
 * A STRING cell is its bytes as they are (not validated as UTF-8), enclosed in quotes with every '"' doubled if and
 * only if it holds ',', '"', LF or CR or is the empty string; no other cell is ever quoted. The header is the caller's.
 *
 * Every column is a device column (DQ_COL_DEVICE) of nrows rows; DQ_COL_OFFSETS64 is honoured. DQ_TYPE_DECIMAL128 has
 * no text here: DQ_ERR_UNSUPPORTED naming the column. Single-device contexts only (DQ_ERR_UNSUPPORTED otherwise).
 * Two calls with the same columns:
 *   dq_csv_write_size  fills row_start (device, nrows + 1 int64, 8-B aligned) with the byte offset of every record in
 *                      the body, row_start[nrows] = *out_bytes = the body's size.
 *   dq_csv_write       writes the body into `out` (device, out_bytes bytes = that size, any alignment) from the same
 *                      columns and row_start; nothing outside [out, out + out_bytes) is written.
 * Kernel launches depend on the number and the types of the columns, never on the rows or the bytes: each call
 * launches DQ_CSV_WRITE_KERNEL_MARK once per STRING column (the C-ABI keeps no state between the calls), the first
 * DQ_CSV_WRITE_KERNEL_SIZES once, the second DQ_CSV_WRITE_KERNEL_WRITE once (not for nrows == 0). The write kernel
 * takes tiles of 256 consecutive rows: a tile whose bytes fit DQ_CSV_WRITE_STAGE_BYTES of LDS is assembled there and
 * flushed with aligned 16-byte stores (DQ_CSV_WRITE_ROUTE_STAGE), any other tile writes to `out` directly
 * (DQ_CSV_WRITE_ROUTE_DIRECT); the bytes are the same. */
#define DQ_CSV_WRITE_STAGE_BYTES 31744 /* 31 KiB: five workgroups of the write kernel fit a CU's 160 KiB of LDS */
typedef enum dq_csv_write_kernel {
    DQ_CSV_WRITE_KERNEL_MARK = 0,  /* csvw_mark_kernel: the quote bitmaps of one STRING column   */
    DQ_CSV_WRITE_KERNEL_SIZES = 1, /* csvw_sizes_kernel: the bytes of every record               */
    DQ_CSV_WRITE_KERNEL_WRITE = 2, /* csvw_write_kernel: the body                                */
    DQ_CSV_WRITE_KERNEL_COUNT = 3
} dq_csv_write_kernel;
typedef enum dq_csv_write_route {
    DQ_CSV_WRITE_ROUTE_STAGE = 0,  /* tiles assembled in LDS           */
    DQ_CSV_WRITE_ROUTE_DIRECT = 1, /* tiles written to global memory   */
    DQ_CSV_WRITE_ROUTE_COUNT = 2
} dq_csv_write_route;
int dq_csv_write_size(dq_ctx* ctx, const dq_column* columns, int32_t ncols, int64_t nrows, int64_t* row_start,
                      int64_t* out_bytes);
int dq_csv_write(dq_ctx* ctx, const dq_column* columns, int32_t ncols, int64_t nrows, const int64_t* row_start,
                 uint8_t* out, int64_t out_bytes);
/* Launches so far of one dq_csv_write_kernel / tiles so far that took one dq_csv_write_route; -1 for a bad index. */
int64_t dq_csv_write_launch_count(const dq_ctx* ctx, int32_t kernel);
int64_t dq_csv_write_route_count(const dq_ctx* ctx, int32_t route);

/* ---- Arrow buffers brought into the engine's layout on the device (Table.from_arrow(t, device=...)) ------------------
 * The caller uploads byte ranges of Arrow buffers as they are; these calls do the per-row work that remains. Every
 * pointer but `pieces` and the reports is device memory. A source is read inside [src, src + src_bytes) only: bytes
 * at and past src_bytes count as zero and are never loaded. No kernel uses an atomic on an output word, and no result
 * depends on the launch grid. Every call returns after its kernels have finished (a staging buffer may be released
 * when it returns). Single-device contexts only (DQ_ERR_UNSUPPORTED otherwise); DQ_ERR_ALIGNMENT for a source or
 * output that is not aligned as stated. */
typedef struct dq_ingest_piece {
    const uint8_t* src; /* LSB-first bits, 8-B aligned; NULL (validity only): the piece has no bitmap, every row is valid */
    int64_t src_bytes;  /* bytes uploaded at src */
    int64_t src_bit0;   /* the bit of the piece's first row (the Arrow offset modulo 8 when src starts at byte offset/8) */
    int64_t rows;       /* > 0 */
    int64_t out_row0;   /* the piece's first output row: 0 for the first piece, then the rows before it */
} dq_ingest_piece;
/* Bits of consecutive pieces (host array; they cover rows [0, nrows) in order) as one output, one launch:
 *   to_bytes == 0: the validity bitmap, (nrows + 63) / 64 words at `out` (8-B aligned), every word written, bits at
 *     and past nrows 0. A lane owns whole output words and assembles each from the source words of the pieces that
 *     cover its 64 rows, so pieces that meet inside a word need no atomics. DQ_KERNEL_INGEST_VALIDITY.
 *   to_bytes != 0: one byte (0 / 1) per row, nrows bytes at `out` (8-B aligned); src must not be NULL.
 *     DQ_KERNEL_INGEST_BOOL.
 * nrows == 0 launches nothing. DQ_ERR_INVALID_ARGUMENT for pieces that are empty, out of order, do not cover the rows
 * or whose source is shorter than their bits. */
int dq_ingest_bits(dq_ctx* ctx, const dq_ingest_piece* pieces, int32_t npieces, int64_t nrows, int32_t to_bytes,
                   void* out);
/* String offsets of one piece: out[i] = src[i] - src[0] + base for 0 <= i < rows, and for i == rows when write_last
 * (the column's last piece). src holds rows + 1 offsets of src_width 4 (int32) or 8 (int64: Arrow large_string) bytes,
 * aligned to their width; out is 4-B aligned. *out_of_range (host) = 1 when a written value lies outside [0, 2^31),
 * else 0; the values are then undefined. One launch, DQ_KERNEL_INGEST_OFFSETS. */
int dq_ingest_offsets(dq_ctx* ctx, const void* src, int64_t src_bytes, int32_t src_width, int64_t rows, int64_t base,
                      int32_t write_last, int32_t* out, int32_t* out_of_range);
typedef enum dq_ingest_kind {
    DQ_INGEST_DECIMAL_LOW = 1, /* 16-byte decimal128 cell -> its low 8 bytes (precision <= 18); a NULL cell -> 0 */
    DQ_INGEST_DECIMAL_WIDE = 2, /* 16-byte cell -> the same cell; a NULL cell -> 0                                */
    DQ_INGEST_TIME_MUL = 3,    /* int64 * param, wrapping modulo 2^64 (s, ms -> us)                               */
    DQ_INGEST_TIME_DIV = 4     /* int64 / param, truncated toward zero (ns -> us); param > 0                      */
} dq_ingest_kind;
/* One piece of fixed-width cells converted into its place in the final buffer: `rows` cells at src (16-B aligned for
 * the decimal kinds, else 8-B) to `out` (aligned to its cell). `validity` (8-B aligned, validity_bytes uploaded, the
 * first row at bit validity_bit0; NULL: no NULLs) is read by the decimal kinds only. One launch,
 * DQ_KERNEL_INGEST_CONVERT; rows == 0 launches nothing. */
int dq_ingest_convert(dq_ctx* ctx, int32_t kind, const void* src, int64_t src_bytes, const uint8_t* validity,
                      int64_t validity_bytes, int64_t validity_bit0, int64_t rows, int64_t param, void* out);
typedef struct dq_ingest_index_report {
    int64_t bad_row;   /* the smallest row of the piece whose index lies outside [0, n_dict) although it is valid; -1: none */
    int64_t bad_index; /* that row's index */
    int64_t null_rows; /* rows that are NULL after the fold (undefined when bad_row >= 0) */
} dq_ingest_index_report;
/* Dictionary indices of one piece (index_width 1 / 2 / 4 / 8 bytes, index_signed or not, aligned to 8 B at src)
 * -> int32 at out (4-B aligned). A row is NULL when its bit in `validity` (as in dq_ingest_convert) is clear or its
 * entry's bit in dict_validity (n_dict bits, NULL: no NULL entries) is clear; a NULL row's index is 0. The NULL rows go
 * to out_validity (8-B aligned, (rows + 63) / 64 words, the piece's first row at bit 0, bits past the rows 0; may be
 * NULL). An index outside [0, n_dict) counts on a valid row only (report). One launch, DQ_KERNEL_INGEST_INDICES. */
int dq_ingest_indices(dq_ctx* ctx, const void* src, int64_t src_bytes, int32_t index_width, int32_t index_signed,
                      const uint8_t* validity, int64_t validity_bytes, int64_t validity_bit0, int64_t rows, int64_t n_dict,
                      const uint8_t* dict_validity, int32_t* out, uint8_t* out_validity, dq_ingest_index_report* report);

/* Train / test row split (ConstraintSuggestionRunner.useTrainTestSplitWithTestsetRatio). Row r of this call is global
 * row g = row0 + r. h = XXH64 of the 8 little-endian bytes of g with seed `seed`: Spark's XXH64.hashLong(g, seed), the
 * function the HLL scan computes with seed 42. Row r is in the TEST set iff
 * (h >> 11) < (uint64_t)(test_ratio * 9007199254740992.0), otherwise in the TRAIN set: membership depends on
 * (seed, g, test_ratio) alone, not on how a table is cut into calls. Both bitmaps are device buffers, 8-B aligned,
 * LSB-first, (nrows + 63) / 64 words; EVERY word is written, and bits at and past nrows are 0. Either bitmap may be
 * NULL (that side is not wanted); the counts are always returned. One kernel launch per call (none for nrows == 0).
 * DQ_ERR_INVALID_ARGUMENT unless 0 < test_ratio < 1, nrows >= 0, row0 >= 0 and row0 + nrows fits an int64;
 * DQ_ERR_ALIGNMENT for a misaligned bitmap; DQ_ERR_UNSUPPORTED on a multi-device context. */
int dq_split_rows(dq_ctx* ctx, int64_t nrows, int64_t row0, uint64_t seed, double test_ratio, uint8_t* train_bits,
                  uint8_t* test_bits, int64_t* num_train, int64_t* num_test);
/* The same membership for one row, host only (no context, no device): 1 = test, 0 = train, < 0 = bad argument
 * (global_row < 0 or a ratio outside ]0, 1[). The same code as the kernel. */
int dq_split_row_is_test(int64_t global_row, uint64_t seed, double test_ratio);

/* Multi-GPU grouping: the canonical 64-bit keys (see DQ_FREQ_KEYS_VALUES) of one
 * fixed-width column's non-NULL rows, bucketed by owner rank = (mix64(key) >> 32) % nparts, written
 * contiguously per rank into keys_dev (capacity nrows, device memory) for an RCCL all-to-all; the
 * owner of a key builds its table from the keys it receives, so every group lives on exactly one
 * rank. part_counts (host, nparts entries) receives the bucket sizes; *null_rows the NULL rows.
 * Returns DQ_OK or an error. */
int dq_partition_keys(dq_ctx* ctx, const dq_column* column, int64_t nrows, int nparts, int64_t* keys_dev,
                      int64_t* part_counts, int64_t* null_rows);

/* Synthetic input generators for benches/tests (counter-based splitmix64). */
typedef enum dq_synth_kind {
    DQ_SYNTH_DYADIC = 1,   /* f64: k * 2^-8, k uniform in [-256, 256]                */
    DQ_SYNTH_UNIFORM = 2,  /* f64: U[0,1) on a 2^-53 grid                            */
    DQ_SYNTH_NORMAL = 3,   /* f64: 100 + 15 * (sum of 12 U[0,1) on a 2^-48 grid - 6)   */
    DQ_SYNTH_INT32R = 4,   /* i64: U[-2^31, 2^31)                                    */
    DQ_SYNTH_KEY30 = 5,    /* i64: splitmix64(row) mod 2^30                          */
    DQ_SYNTH_GAUSS01 = 6,  /* f64: sum of 12 U[0,1) on a 2^-48 grid - 6              */
    DQ_SYNTH_GAUSS_CORR = 7/* f64: 0.6 * GAUSS01(seed) + 0.8 * GAUSS01(seed ^ 0x5A5A5A5A5A5A5A5A):
                            *      correlated (rho ~ 0.6) with the GAUSS01 column of the same seed */
} dq_synth_kind;

int dq_synth_column(dq_ctx* ctx, int32_t kind, uint64_t seed, int64_t row0, int64_t nrows,
                    void* values_dev);
/* Config-C4 frequency keys: row r of a `total_rows` table gets key
 * mix64(j < distinct ? j : (j - distinct) mod (distinct / 2)) with j = (r * 0x9E3779B1) mod total_rows,
 * so exactly `distinct` keys exist when (total_rows - distinct) is a multiple of distinct / 2. */
int dq_synth_freq_keys(dq_ctx* ctx, int64_t total_rows, int64_t distinct, int64_t row0, int64_t nrows,
                       int64_t* keys_dev);
/* UTF-8 string columns of config C5. Two calls: with bytes_dev == NULL, writes the int32 Arrow
 * offsets (nrows + 1 entries, device) and *total_bytes; then with bytes_dev (>= total_bytes + 16 bytes) writes the
 * strings. Kinds: */
#define DQ_SYNTH_STR_CAT50 101  /* "cat_<0..49>"                                           */
#define DQ_SYNTH_STR_BOOL 102   /* "true" / "false"                                        */
#define DQ_SYNTH_STR_CAT100 103 /* "v<00..99>"                                             */
#define DQ_SYNTH_STR_INT 104    /* an integer in [-1e6, 1e6)                               */
#define DQ_SYNTH_STR_DEC 105    /* "<0..999>.<00..99>"                                     */
#define DQ_SYNTH_STR_MIXNUM 106 /* 70 %: an integer in [-5000, 5000); 30 %: "<+-int>.<ddd>" */
#define DQ_SYNTH_STR_TEXT 107   /* 1-20 characters of [a-z0-9 ]                           */
int dq_synth_strings(dq_ctx* ctx, int32_t kind, uint64_t seed, int64_t row0, int64_t nrows, int32_t* offsets_dev,
                     void* bytes_dev, int64_t* total_bytes);
/* Validity bitmap (ceil(nrows/64) words) with P(null) = null_permille / 1000. */
int dq_synth_validity(dq_ctx* ctx, uint64_t seed, int64_t row0, int64_t nrows, int32_t null_permille,
                      uint8_t* validity_dev);

#ifdef __cplusplus
}
#endif

#endif /* DEEQU_AMD_DQ_H */
