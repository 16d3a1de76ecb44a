// scan_plan.h — the host plan of one fused-scan call (dq_scan) as plain data.
//
// validate_scan -> plan_scan -> plan_geometry -> layout_scan are pure functions of the call's arguments: no HIP call,
// no environment variable, no dq_ctx. Column and predicate buffers are only tested for presence (and, for host
// STRING columns, offsets[nrows] is read for the staged byte count), so the whole plan runs on the CPU under the
// host sanitizers (tests/sanitize_scan_plan). dq_api.cpp turns a plan and its layout into device descriptors once the
// arena's address is known; every reference in here is an integer index.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "dq_internal.h"

namespace dq {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// What dq_api.cpp reads from the environment per call (DQ_WHERE_MASKS, DQ_WHERE_FUSED, DQ_PRED_VM).
struct ScanOptions {
    bool where_masks = true;     // simple `where` filters are evaluated inside the scan (WhereOut)
    bool fused_producer = true;  // ... by the scan of the filter's own column where that is possible
    bool pred_vm = false;        // every predicate on the general VM: no masks, no simple-predicate kernel
    // Not from the environment: predicates the caller's own kernel evaluates from their column (dq_row_outcomes), which
    // get neither bitmaps nor a pass; their columns stay staged. Empty: none.
    std::vector<char> pred_inline;
};

// Which columns / predicates the call reads, and which ops go to the decimal128 launch (validate_scan).
struct ScanUse {
    std::vector<char> col_used, pred_used, wide_op;
};

// One column of a value slot: what ColDesc carries besides addresses.
struct PlanCol {
    int column = -1;
    int elem = ET_NONE;
    uint32_t flags = 0;  // ColFlags
    int hll_slot = -1;
    int pred_op = 0, pred_kind = FP_NONE;  // fused Compliance predicate `column <op> constant`
    int64_t pred_i = 0;
    double pred_d = 0.0;
    int mask_pred = -1, mask_index = -1;  // reads mask `mask_index` of masked filter `mask_pred` in place of its validity
};

enum BitsTag : int { BT_SIZE = 0, BT_COMPLETENESS = 1, BT_COMPLIANCE = 2 };

struct PlanSlot {
    int kind = SK_VALUES;  // SlotKind
    int where = -1;        // predicate whose TRUE / NOT-NULL bitmaps the slot's kernel reads; -1 once the filter is masked
    // SK_VALUES
    int ncols = 0, corr = 0, rows_per_load = 8;
    PlanCol col[2];
    int producer_of = -1;  // masked filter this slot's scan evaluates (fused producer)
    // SK_BITS
    int tag = BT_SIZE;     // BitsTag
    int ref = -1;          // BT_COMPLETENESS: column, BT_COMPLIANCE: predicate
};

struct PlanStrSlot {
    int column = -1, where = -1;
    uint32_t flags = 0;  // StrFlags
    int hll_slot = -1;
};

struct PlanD128Slot {
    int column = -1, where = -1;
    uint32_t flags = 0;  // D128Flags
    int hll_slot = -1;
};

// A `where` predicate evaluated inside the scan (WhereOut, dq_internal.h).
struct WherePlan {
    bool masked = false;
    int producer = -1;          // value slot evaluating the filter inside its scan, -1: where_masks_kernel
    int wslot = -1;             // slot holding the TRUE / NOT-NULL counts (the producer, or an SK_WHERE slot)
    bool bitmaps = false;       // bits / string / decimal128 slots still read the filter's bitmaps
    std::vector<int> mask_col;  // consumer columns, one mask each
    PredSimple prog;            // masked: the compiled filter
};

// One kernel launch: the slots of one shape.
struct PlanGroup {
    int kind, P, nc;
    bool f0, f1;
    int heavy;  // 0 light, 1 heavy, 2 heavy and branch-free (8-byte), 3 fused `where` producer
    int key;    // the shape as one integer (occupancy cache)
    std::vector<int32_t> slots;
};

struct ScanPlan {
    std::vector<PlanSlot> slots;
    std::vector<PlanStrSlot> sslots;
    std::vector<PlanD128Slot> dslots;
    std::vector<OpMap> opmap;        // one per op
    std::vector<StrOpMap> sopmap;    // MinLength / MaxLength / DataType
    std::vector<D128OpMap> dopmap;   // DECIMAL128 ops but ApproxCountDistinct
    std::vector<WherePlan> where;    // one per predicate
    std::vector<char> pred_used;     // the predicate gets TRUE / NOT-NULL bitmaps
    std::vector<char> pred_pass;     // a predicate pass writes them (a masked filter's come from its producer)
    int nstandalone = 0;             // masked filters without a fused producer
    int nhll = 0;                    // HLL register sets over value, string and decimal128 slots
    std::vector<PlanGroup> groups;   // launch order: fused producers first
    int nlaunch() const { return (int)groups.size() + (sslots.empty() ? 0 : 1); }  // launches that may run concurrently
};

struct ScanGeometry {
    int64_t ntiles = 0;
    std::vector<int> grid;  // per group
    int sgrid = 0, dgrid = 0, wgrid = 1;
    int gstride = 1;        // partials of a slot are gstride apart
    std::vector<int32_t> slot_nblocks, hll_nblocks;
};

// Offsets into the context arena of everything a call keeps there, in the order it is laid out. kNoOffset: absent.
constexpr size_t kNoOffset = ~(size_t)0;
struct PredOffsets {
    size_t t = kNoOffset, nn = kNoOffset;                    // bitmaps (pred_used)
    size_t wout = kNoOffset;                                 // WhereOut (masked)
    size_t mask0 = kNoOffset;                                // first consumer mask, the others follow mask_stride apart
    size_t prog = kNoOffset, code = kNoOffset, consts = kNoOffset, strings = kNoOffset;  // pred_pass
};
struct ScanLayout {
    struct Column { size_t values = kNoOffset, validity = kNoOffset, offsets = kNoOffset, vbytes = 0; };
    std::vector<Column> col;  // staged host columns
    std::vector<PredOffsets> pred;
    size_t mask_stride = 0;
    size_t pcols = 0, status = 0;
    size_t slots = 0, ops = 0, partials = 0, order = 0, slot_nblocks = 0, hll_nblocks = 0, finals = 0, hll_partials = 0,
           hll_final = 0, out = kNoOffset;
    size_t sslots = 0, spartials = 0, sops = 0;
    size_t dslots = 0, dpartials = 0, dops = 0;
    size_t arena_bytes = 0;
    size_t pinned_bytes = 0;  // staging for every upload and read-back of the call
};

// Returns `code` with the formatted message in *msg: how every plan function refuses a call.
int failf(std::string* msg, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
// DQ_OK, or the error code with its message in *msg (without the "predicate %d: " prefix). col_used (may be null):
// set for every column the program reads.
int validate_predicate(const dq_predicate& pr, const dq_column* columns, int ncols, std::string* msg, char* col_used = nullptr);
int validate_scan(const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops, const dq_predicate* preds,
                  int npreds, ScanUse* use, std::string* msg);
// Pinned staging bytes of one predicate's program pieces, as run_predicate uploads them.
size_t pred_stage_bytes(const dq_predicate& pr);
// Recognises the predicates pred_simple_kernel evaluates (see PredSimple): a symbolic run of the postfix program.
bool compile_simple_predicate(const dq_predicate& pr, const dq_column* columns, int ncols, PredSimple& out);
// Of a validated call. DQ_ERR_UNSUPPORTED when it needs more than kMaxSlots slots.
int plan_scan(const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops, const dq_predicate* preds,
              int npreds, const ScanUse& use, const ScanOptions& options, ScanPlan* plan, std::string* msg);
// Grids. occ[g]: workgroups per CU of plan.groups[g]; sgrid / dgrid: the string and decimal128 launches' full grids
// (0 without such slots); concurrent: the launches share the chip, each gets 1 / nlaunch of its grid.
ScanGeometry plan_geometry(const ScanPlan& plan, int cus, int64_t ntiles, int64_t grid_cap, bool concurrent, int sgrid,
                           int dgrid, const int* occ);
ScanLayout layout_scan(const ScanPlan& plan, const ScanGeometry& geo, const ScanUse& use, const dq_column* columns, int ncols,
                       int64_t nrows, int nops, const dq_predicate* preds, int npreds, bool out_device);

}  // namespace dq
