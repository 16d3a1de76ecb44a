// call_plans.h — the host plans of dq_row_outcomes and dq_dict_scan as plain data.
//
// As scan_plan.h: plan_row_outcomes and plan_dict_scan are pure functions of the call's arguments (no HIP call, no
// environment variable, no dq_ctx). Buffers are only tested for presence and alignment, every reference in a plan is an
// integer index, and dq_api.cpp resolves a plan into device descriptors once the addresses are known. Both run on the CPU
// under the host sanitizers (tests/sanitize_scan_plan).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "dq_dict.h"
#include "scan_plan.h"

namespace dq {

// ---- dq_row_outcomes ---------------------------------------------------------------------------------------------------
// Where a term's source (what must hold for it to pass) comes from; `index` names the bitmap, predicate or column.
enum RowSource : int {
    RP_BITS = 0,          // the caller's pass bitmap (DQ_ROW_BITS)
    RP_PRED = 1,          // predicate `index`: its TRUE bitmap from the predicate stage
    RP_INLINE = 2,        // inline predicate `index` of the launch
    RP_VALID_DEVICE = 3,  // column `index`: a device column's validity, read in place
    RP_VALID_SCAN = 4,    // ... a host column a predicate reads: where the predicate stage put it
    RP_VALID_CALL = 5,    // ... a host column no predicate reads: only its bitmap goes to the device, by this call
    RP_ONES = 6,          // ... a column without validity: every row holds
};
// The validity kinds, for any kernel that reads a column's validity after the predicate stage (dq_filter_validity too).
int validity_source(const dq_column& col, bool read_by_predicate);

struct RowPlanTerm {
    int term = -1;      // the caller's term: counters 2 i, 2 i + 1 of the launch go to term_counts[2 term], [2 term + 1]
    int src = RP_ONES;  // RowSource
    int index = -1;
    int where = -1;     // the rows it considers: predicate `where`'s TRUE bitmap, -1 = every row (RP_BITS: the caller's)
    int w_inline = -1;  // ... or inline predicate w_inline (then where is -1)
};
struct RowPlan {
    bool null_mode = false;
    std::vector<RowPlanTerm> term;          // sorted by check (stable)
    std::vector<int> term_begin, term_end;  // per check: its terms are term[term_begin .. term_end)
    std::vector<PredTerm> inl;              // `column <op> constant` predicates the launch evaluates itself (<= kRowInline)
    std::vector<int> inline_of;             // per predicate: its inline predicate, or -1 (it gets a pass)
    ScanOptions options;                    // of the predicate stage: the bitmap pass, without the inline predicates
    ScanUse use;                            // columns the predicates read (validate_scan of one Size(where = p) per predicate)
};
// One dummy Size(where = p) per predicate: how a call that only wants predicate bitmaps goes through the scan's stages.
std::vector<dq_op> size_where_ops(int npreds);
// Everything dq_row_outcomes decides before its first HIP call. DQ_OK, or the error code with its message in *msg.
int plan_row_outcomes(const dq_column* columns, int ncols, int64_t nrows, const dq_predicate* preds, int npreds,
                      const dq_row_term* terms, int nterms, const dq_row_check* checks, int nchecks, uint32_t flags, bool pred_vm,
                      RowPlan* plan, std::string* msg);

// ---- dq_dict_scan / dq_dict_counts -------------------------------------------------------------------------------------
// What dq_api.cpp reads from the environment per call (DQ_DICT_LDS_ENTRIES, DQ_DICT_LDS_COPIES).
struct DictOptions {
    int lds_entries = kDictLdsWords;  // dictionaries of up to this many entries count in LDS (clamped to [0, kDictLdsWords])
    int lds_copies = kDictLdsCopies;  // most LDS counter copies: 1, 2 or 4 lower it, anything else is ignored
};
// LDS counter copies of a slot, 0 = global atomics. A workgroup reads at most nrows / grid + 2 tiles of rows, which
// must stay below 2^31 so that no 32-bit LDS counter can wrap.
int dict_lds_copies(const DictOptions& options, int n_dict, int64_t nrows, int grid);
int check_dict_column(const dq_dict_column& d, int64_t nrows, int which, std::string* msg);

struct DictPlanSlot {
    int dict = -1, where = -1;  // one slot per (dictionary column, where)
    uint32_t flags = 0;         // StrFlags: what the fold computes
    int n_dict = 0, lds_copies = 0;
    size_t stats = 0, fold = 0, counts = 0, hll = 0;  // word offsets into the zero block
};
// A Compliance / PatternMatch op: its predicate runs over the slot's dictionary entries.
struct DictPlanPred {
    int pred = -1, slot = -1;
    std::vector<int32_t> code;  // the predicate's program with every DQ_P_COL reading column 0 = the dictionary
};
struct DictPlan {
    std::vector<DictPlanSlot> slots;
    std::vector<DictOpMap> opmap;    // one per op; sums is left null (op_pop names it)
    std::vector<int> op_pop;         // per op: its predicate op (its sums are at sums_off + 2 op_pop), or -1
    std::vector<DictPlanPred> pops;  // predicate ops
    std::vector<char> where_used;    // per predicate: some op's where, evaluated over the plain columns
    int max_entries = 0, nstatus = 0, lds_words = 0;
    // One zeroed block of 8-byte words: per slot stats, fold, counts and HLL registers, then two sums per predicate op.
    size_t sums_off = 0, zwords = 0;
    size_t pinned_bytes = 0;  // staging for every upload and read-back of the call
};
// A predicate op's program as run_predicate takes it (views the plan's code copy).
dq_predicate dict_pop_predicate(const DictPlan& plan, int q, const dq_predicate* preds);
// Everything dq_dict_scan decides before its first HIP call; grid: dict_counts_grid of the call.
int plan_dict_scan(const dq_column* columns, int ncols, const dq_dict_column* dicts, int ndicts, int64_t nrows, const dq_op* ops,
                   int nops, const dq_predicate* preds, int npreds, const DictOptions& options, int grid, DictPlan* plan,
                   std::string* msg);

}  // namespace dq
