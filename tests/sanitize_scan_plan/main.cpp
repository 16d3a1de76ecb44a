// ASan + UBSan run of the fused scan's host plan (deequ_amd/csrc/scan_plan.cpp, -DDQ_HOST_ONLY: no HIP, no GPU):
// validate_scan -> plan_scan -> plan_geometry -> layout_scan checked field by field against the rules of dq_scan,
// and validate_predicate over rejected examples and 20 000 seeded random programs on exactly-sized heap buffers.
// Column buffers are presence flags only: nothing here is ever dereferenced by the plan.
// The same for the plans of dq_row_outcomes and dq_dict_scan (call_plans.cpp): plan_row_outcomes, plan_dict_scan,
// dict_lds_copies and every refusal's code and text.
// Built and run by tests/test_scan_plan.py; prints "scan_plan_checks: ok" and exits 0 when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "call_plans.h"
#include "scan_plan.h"

using namespace dq;

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++g_failed;                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
        }                                                                   \
    } while (0)

alignas(16) static char g_present[16];  // every "device buffer": aligned, never read

static dq_column column(int type, bool validity, int64_t nrows, int precision = 0, int scale = 0) {
    dq_column c;
    memset(&c, 0, sizeof(c));
    c.spark_type = type;
    c.flags = DQ_COL_DEVICE;
    c.length = nrows;
    c.values = g_present;
    c.validity = validity ? (const uint8_t*)g_present : nullptr;
    c.offsets = type == DQ_TYPE_STRING ? (const int32_t*)g_present : nullptr;
    c.decimal_precision = precision;
    c.decimal_scale = scale;
    return c;
}

enum { K = 0, L, D, G, I, F, B, S, W, NCOLS };
static std::vector<dq_column> table(int64_t nrows) {
    return {column(DQ_TYPE_LONG, true, nrows),   column(DQ_TYPE_LONG, false, nrows), column(DQ_TYPE_DOUBLE, true, nrows),
            column(DQ_TYPE_DOUBLE, true, nrows), column(DQ_TYPE_INT, true, nrows),   column(DQ_TYPE_FLOAT, true, nrows),
            column(DQ_TYPE_BYTE, true, nrows),   column(DQ_TYPE_STRING, true, nrows), column(DQ_TYPE_DECIMAL128, true, nrows, 38, 18)};
}

static dq_op op(int kind, int c0 = -1, int where = -1, int predicate = -1, int c1 = -1) {
    dq_op o;
    o.kind = kind;
    o.column[0] = c0;
    o.column[1] = c1;
    o.where = where;
    o.predicate = predicate;
    return o;
}

struct Pred {
    std::vector<int32_t> code;
    std::vector<dq_const> consts;
    std::vector<uint8_t> strings;
    dq_predicate view() const {
        dq_predicate p;
        p.code = code.data();
        p.code_len = (int32_t)code.size();
        p.n_consts = (int32_t)consts.size();
        p.consts = consts.data();
        p.strings = strings.data();
        p.strings_len = (int64_t)strings.size();
        return p;
    }
};
static dq_const long_const(int64_t v) {
    dq_const c;
    memset(&c, 0, sizeof(c));
    c.tag = DQ_V_LONG;
    c.i64 = v;
    return c;
}
// column <cmp> constant
static Pred compare(int col, int cmp, int64_t v) {
    Pred p;
    p.code = {DQ_P_COL, col, DQ_P_CONST, 0, cmp, 0};
    p.consts = {long_const(v)};
    return p;
}
// d > 40 AND k < 10
static Pred d_and_k() {
    Pred p;
    p.code = {DQ_P_COL, D, DQ_P_CONST, 0, DQ_P_GT, 0, DQ_P_COL, K, DQ_P_CONST, 1, DQ_P_LT, 0, DQ_P_AND, 0};
    p.consts = {long_const(40), long_const(10)};
    return p;
}

struct Run {
    int rc = 0;
    std::string msg;
    ScanUse use;
    ScanPlan plan;
};
static Run run(const std::vector<dq_column>& cols, int64_t nrows, const std::vector<dq_op>& ops, const std::vector<Pred>& preds,
               ScanOptions options = ScanOptions()) {
    std::vector<dq_predicate> pv;
    for (const Pred& p : preds) pv.push_back(p.view());
    Run r;
    r.rc = validate_scan(cols.data(), (int)cols.size(), nrows, ops.data(), (int)ops.size(), pv.data(), (int)pv.size(), &r.use, &r.msg);
    if (r.rc) return r;
    r.rc = plan_scan(cols.data(), (int)cols.size(), nrows, ops.data(), (int)ops.size(), pv.data(), (int)pv.size(), r.use, options,
                     &r.plan, &r.msg);
    return r;
}
static int count_kind(const ScanPlan& p, int kind) {
    int n = 0;
    for (const PlanSlot& s : p.slots) n += s.kind == kind;
    return n;
}
static bool any_mask(const ScanPlan& p) {
    for (const PlanSlot& s : p.slots)
        for (const PlanCol& c : s.col)
            if (c.mask_pred >= 0 || c.mask_index >= 0) return true;
    return false;
}

static const int64_t kRows = 50001;

static std::vector<dq_op> heavy_ops(int where) {
    return {op(DQ_OP_MEAN, K, where),      op(DQ_OP_SUM, K, where),
            op(DQ_OP_MINIMUM, K, where),   op(DQ_OP_MAXIMUM, K, where),
            op(DQ_OP_STANDARD_DEVIATION, K, where), op(DQ_OP_APPROX_COUNT_DISTINCT, K, where),
            op(DQ_OP_COMPLETENESS, K, where), op(DQ_OP_COMPLIANCE, -1, where, 0)};
}

static void case1_heavy2() {
    const Run r = run(table(kRows), kRows, heavy_ops(-1), {compare(K, DQ_P_LT, 25)});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(p.slots.size() == 1);  // every use of (k, no where) shares one value slot
    const PlanSlot& s = p.slots[0];
    CHECK(s.kind == SK_VALUES && s.ncols == 1 && s.corr == 0 && s.where == -1);
    CHECK(s.rows_per_load == 2);  // an 8-byte column loads 2 rows at a time
    CHECK(s.col[0].column == K && s.col[0].elem == ET_I64);
    CHECK(s.col[0].flags == (CF_STATS | CF_MOMENTS | CF_HLL));  // Mean..Maximum, StandardDeviation, ApproxCountDistinct
    CHECK(s.col[0].pred_kind == FP_LONG && s.col[0].pred_op == DQ_P_LT && s.col[0].pred_i == 25);  // Compliance rides in the scan
    CHECK(s.col[0].hll_slot == 0 && p.nhll == 1);  // one register set
    for (size_t i = 0; i < p.opmap.size(); ++i) {
        CHECK(p.opmap[i].slot == 0 && p.opmap[i].colpos == 0);  // every op is answered from that slot
        CHECK(p.opmap[i].wslot == -1 && p.opmap[i].has_where == 0);  // no where: no conditionalCount slot
    }
    CHECK(p.opmap[7].from_bits == 3);  // fused Compliance reads c.pt / c.n
    CHECK(p.opmap[5].hll_slot == 0);
    CHECK(count_kind(p, SK_BITS) == 0 && count_kind(p, SK_WHERE) == 0);  // nothing needs a bits-only pass
    CHECK(p.pred_used[0] == 0 && p.pred_pass[0] == 0);  // a fused Compliance predicate gets no bitmaps
    CHECK(p.groups.size() == 1);
    // 8-byte, stats + moments + HLL + a LONG compare, no where: the branch-free heavy kernel (DQ_KERNEL_HEAVY8_FULL)
    CHECK(p.groups[0].heavy == 2 && p.groups[0].kind == SK_VALUES && p.groups[0].P == 2 && p.groups[0].nc == 1);
    CHECK(!p.groups[0].f0 && !p.groups[0].f1);
    CHECK(p.groups[0].slots == std::vector<int32_t>{0});
    CHECK(p.sslots.empty() && p.dslots.empty() && p.sopmap.empty() && p.dopmap.empty());
}

static void case2_fused_producer() {
    std::vector<dq_op> ops = heavy_ops(0);
    ops.push_back(op(DQ_OP_SIZE, -1, 0));
    ops.push_back(op(DQ_OP_CORRELATION, D, -1, -1, G));  // a pair slot is planned first: the producer's group is made second
    const Run r = run(table(kRows), kRows, ops, {compare(K, DQ_P_LT, 25)});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(p.slots.size() == 2 && count_kind(p, SK_WHERE) == 0 && count_kind(p, SK_BITS) == 0);  // no SK_WHERE, no bits slot
    const int prod = 1;
    CHECK(p.slots[0].corr == 1 && p.slots[prod].col[0].column == K);
    const WherePlan& wp = p.where[0];
    CHECK(wp.masked);  // a simple predicate used as a where is evaluated inside the scan
    CHECK(wp.producer == prod && wp.wslot == prod);  // by the scan of its own 8-byte column
    CHECK(p.slots[prod].producer_of == 0 && p.slots[prod].where == -1);  // which reads no bitmap
    CHECK(wp.mask_col.empty() && !wp.bitmaps);  // nobody else is under the filter, nothing reads its bitmaps
    CHECK(wp.prog.nterms == 1 && wp.prog.t[0].col == K && wp.prog.t[0].op == DQ_P_LT && wp.prog.t[0].ci == 25);
    for (int i = 0; i < 9; ++i) CHECK(p.opmap[i].wslot == prod && p.opmap[i].has_where == 1);  // conditionalCount from the producer
    CHECK(p.opmap[8].slot == -1);  // Size(where) needs no slot of its own
    CHECK(p.opmap[7].from_bits == 3 && p.opmap[7].slot == prod);
    CHECK(p.pred_used[0] == 0 && p.pred_pass[0] == 0 && p.nstandalone == 0);  // no bitmaps, no predicate pass
    CHECK(p.groups.size() == 2);
    CHECK(p.groups[0].heavy == 3 && p.groups[0].slots == std::vector<int32_t>{prod});  // producers launch first
    CHECK(p.groups[1].heavy == 0 && p.groups[1].nc == 2 && p.groups[1].slots == std::vector<int32_t>{0});
    CHECK(!any_mask(p));
}

static void case3_pair_sharing() {
    const Run r = run(table(kRows), kRows,
                      {op(DQ_OP_CORRELATION, D, -1, -1, G), op(DQ_OP_CORRELATION, G, -1, -1, D), op(DQ_OP_MEAN, D), op(DQ_OP_MEAN, G)}, {});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(p.slots.size() == 1);  // (d, g) and (g, d) share one pair slot, which also carries both Means
    CHECK(p.slots[0].ncols == 2 && p.slots[0].corr == 1 && p.slots[0].rows_per_load == 2);
    CHECK(p.slots[0].col[0].column == D && p.slots[0].col[1].column == G);
    CHECK(p.opmap[0].slot == 0 && p.opmap[0].colpos == 0);
    CHECK(p.opmap[1].slot == 0 && p.opmap[1].colpos == 1);  // the swapped pair
    CHECK(p.opmap[2].slot == 0 && p.opmap[2].colpos == 0);  // Mean(d) at position 0
    CHECK(p.opmap[3].slot == 0 && p.opmap[3].colpos == 1);  // Mean(g) at position 1
    CHECK(p.slots[0].col[0].flags == CF_STATS && p.slots[0].col[1].flags == CF_STATS);
    CHECK(p.groups.size() == 1 && p.groups[0].nc == 2 && p.groups[0].f0 && p.groups[0].f1 && p.groups[0].heavy == 0);

    const Run q = run(table(kRows), kRows, {op(DQ_OP_CORRELATION, D, -1, -1, D), op(DQ_OP_MEAN, D)}, {});
    CHECK(q.rc == DQ_OK);
    CHECK(q.plan.slots.size() == 2);  // a (d, d) pair slot takes no use: Mean(d) gets its own slot
    CHECK(q.plan.opmap[0].slot == 0 && q.plan.opmap[1].slot == 1 && q.plan.opmap[1].colpos == 0);
    CHECK(q.plan.slots[0].col[0].flags == 0 && q.plan.slots[0].col[1].flags == 0);
    CHECK(q.plan.slots[1].ncols == 1 && q.plan.slots[1].col[0].flags == CF_STATS);
}

static void case4_mixed_sizes() {
    const Run r = run(table(kRows), kRows, {op(DQ_OP_CORRELATION, I, -1, -1, D)}, {});
    CHECK(r.rc == DQ_OK);
    CHECK(r.plan.slots.size() == 1 && r.plan.slots[0].rows_per_load == 8);  // element sizes differ: 8 rows per load
    CHECK(r.plan.slots[0].col[0].elem == ET_I32 && r.plan.slots[0].col[1].elem == ET_F64);
    CHECK(r.plan.groups.size() == 1 && r.plan.groups[0].P == 8 && !r.plan.groups[0].f0 && r.plan.groups[0].f1);
}

static void case5_standalone_where() {
    const Run r = run(table(kRows), kRows, {op(DQ_OP_MEAN, L, 0)}, {d_and_k()});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(p.slots.size() == 2 && p.slots[0].kind == SK_VALUES && p.slots[1].kind == SK_WHERE);  // the count slot comes last
    const WherePlan& wp = p.where[0];
    CHECK(wp.masked && wp.producer == -1 && wp.wslot == 1);  // the filter reads d and k, not l: where_masks_kernel
    CHECK(wp.mask_col == std::vector<int>{L} && !wp.bitmaps);  // one mask, for l
    CHECK(p.slots[0].col[0].mask_pred == 0 && p.slots[0].col[0].mask_index == 0 && p.slots[0].where == -1);
    CHECK(p.nstandalone == 1 && p.pred_used[0] == 0 && p.pred_pass[0] == 0);
    CHECK(p.opmap[0].slot == 0 && p.opmap[0].wslot == 1);
    CHECK(r.use.col_used[D] && r.use.col_used[K] && r.use.col_used[L] && !r.use.col_used[G]);  // the filter's columns are staged too
    CHECK(p.groups.size() == 1 && p.groups[0].slots == std::vector<int32_t>{0});  // an SK_WHERE slot is in no launch group

    const Run q = run(table(kRows), kRows, {op(DQ_OP_MEAN, L, 0), op(DQ_OP_MIN_LENGTH, S, 0)}, {d_and_k()});
    CHECK(q.rc == DQ_OK);
    CHECK(q.plan.sslots.size() == 1 && q.plan.sslots[0].column == S && q.plan.sslots[0].where == 0 && q.plan.sslots[0].flags == SF_LEN);
    CHECK(q.plan.where[0].bitmaps);  // the string scan reads the filter's TRUE bitmap
    CHECK(q.plan.pred_used[0] == 1 && q.plan.pred_pass[0] == 0);  // allocated, written by the producer
    CHECK(q.plan.sopmap.size() == 1 && q.plan.sopmap[0].op == 1 && q.plan.sopmap[0].kind == DQ_OP_MIN_LENGTH && q.plan.sopmap[0].slot == 0);
    CHECK(q.plan.nlaunch() == 2);
}

static void case6_fallback() {
    std::vector<dq_column> cols(35, column(DQ_TYPE_LONG, false, kRows));
    std::vector<dq_op> ops;
    for (int c = 0; c < 33; ++c) ops.push_back(op(DQ_OP_MEAN, c, 0));
    ops.push_back(op(DQ_OP_SIZE, -1, 0));
    ops.push_back(op(DQ_OP_COMPLETENESS, 34, 0));  // unread, no validity: from_bits == 2
    const Run r = run(cols, kRows, ops, {compare(33, DQ_P_LT, 5)});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(!p.where[0].masked && p.where[0].mask_col.empty() && p.where[0].wslot == -1);  // 33 > kWhereMasks consumers: the bitmap pass
    CHECK(p.pred_used[0] == 1 && p.pred_pass[0] == 1 && p.nstandalone == 0);
    CHECK(!any_mask(p));  // no slot keeps a mask assignment
    CHECK(p.slots.size() == 34 && count_kind(p, SK_BITS) == 1 && count_kind(p, SK_WHERE) == 0);
    const PlanSlot& bits = p.slots[33];
    CHECK(bits.kind == SK_BITS && bits.tag == BT_SIZE && bits.ref == -1 && bits.where == 0);
    CHECK(p.opmap[33].slot == 33 && p.opmap[33].wslot == 33);  // Size(where) gets its bits slot back
    CHECK(p.opmap[34].slot == 33 && p.opmap[34].from_bits == 2 && p.opmap[34].wslot == 33);  // and so does Completeness
    for (int c = 0; c < 33; ++c) {
        CHECK(p.slots[c].where == 0);  // value slots read the bitmaps again
        CHECK(p.opmap[c].slot == c && p.opmap[c].wslot == c);
    }
}

static void case7_two_constants() {
    const Run r = run(table(kRows), kRows, {op(DQ_OP_COMPLIANCE, -1, -1, 0), op(DQ_OP_COMPLIANCE, -1, -1, 1), op(DQ_OP_MEAN, K)},
                      {compare(K, DQ_P_LT, 25), compare(K, DQ_P_LT, 26)});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(p.slots.size() == 2);
    CHECK(p.slots[0].kind == SK_VALUES && p.slots[0].col[0].pred_i == 25);  // one fused predicate per column scan: the first
    CHECK(p.opmap[0].slot == 0 && p.opmap[0].from_bits == 3);
    CHECK(p.slots[1].kind == SK_BITS && p.slots[1].tag == BT_COMPLIANCE && p.slots[1].ref == 1 && p.slots[1].where == -1);
    CHECK(p.opmap[1].slot == 1 && p.opmap[1].from_bits == 0);  // the second goes through the predicate pass
    CHECK(p.pred_used[0] == 0 && p.pred_used[1] == 1 && p.pred_pass[1] == 1);
    CHECK(p.groups.size() == 2 && p.groups[0].heavy == 1 && p.groups[1].kind == SK_BITS);
}

static void case8_unread_completeness() {
    const Run r = run(table(kRows), kRows, {op(DQ_OP_COMPLETENESS, K)}, {});
    CHECK(r.rc == DQ_OK);
    CHECK(r.plan.slots.size() == 1 && r.plan.slots[0].kind == SK_BITS);  // a column nobody reads: pop-count its validity
    CHECK(r.plan.slots[0].tag == BT_COMPLETENESS && r.plan.slots[0].ref == K && r.plan.slots[0].where == -1);
    CHECK(r.plan.opmap[0].slot == 0 && r.plan.opmap[0].from_bits == 1);
    const Run q = run(table(kRows), kRows, {op(DQ_OP_COMPLETENESS, L)}, {});
    CHECK(q.rc == DQ_OK);
    CHECK(q.plan.slots.empty() && q.plan.groups.empty());  // no validity, no where: every row counts, nothing to scan
    CHECK(q.plan.opmap[0].slot == -1 && q.plan.opmap[0].from_bits == 2 && q.plan.opmap[0].nrows == kRows);
}

static void case9_hll_numbering() {
    const Run r = run(table(kRows), kRows,
                      {op(DQ_OP_APPROX_COUNT_DISTINCT, K), op(DQ_OP_APPROX_COUNT_DISTINCT, S), op(DQ_OP_APPROX_COUNT_DISTINCT, W),
                       op(DQ_OP_MEAN, W)}, {});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(p.nhll == 3);  // numbered value slots, then string slots, then decimal128 slots
    CHECK(p.opmap[0].hll_slot == 0 && p.slots.size() == 1 && p.slots[0].col[0].hll_slot == 0);
    CHECK(p.opmap[1].hll_slot == 1 && p.sslots.size() == 1 && p.sslots[0].hll_slot == 1 && p.sslots[0].flags == SF_HLL);
    CHECK(p.opmap[2].hll_slot == 2 && p.dslots.size() == 1 && p.dslots[0].hll_slot == 2);
    CHECK(r.use.wide_op == (std::vector<char>{0, 0, 1, 1}));  // DECIMAL128 ops go to the decimal128 launch
    CHECK(p.dslots[0].column == W && p.dslots[0].where == -1 && p.dslots[0].flags == (DF_HLL | DF_SUM));
    CHECK(p.dopmap.size() == 1 && p.dopmap[0].op == 3 && p.dopmap[0].kind == DQ_OP_MEAN && p.dopmap[0].slot == 0);  // not the HLL op
    CHECK(p.opmap[2].slot == -1 && p.opmap[3].slot == -1 && p.sopmap.empty());
}

static void case10_too_many_slots() {
    std::vector<dq_column> cols(257, column(DQ_TYPE_LONG, true, kRows));
    std::vector<dq_op> ops;
    for (int c = 0; c < 257; ++c) ops.push_back(op(DQ_OP_MEAN, c));
    const Run r = run(cols, kRows, ops, {});
    CHECK(r.rc == DQ_ERR_UNSUPPORTED && r.msg.find("too many slots") != std::string::npos);  // more than kMaxSlots
    ops.pop_back();
    CHECK(run(cols, kRows, ops, {}).rc == DQ_OK);  // exactly kMaxSlots fit
}

static bool same_plan(const ScanPlan& a, const ScanPlan& b) {
    if (a.slots.size() != b.slots.size() || a.groups.size() != b.groups.size() || a.opmap.size() != b.opmap.size()) return false;
    for (size_t s = 0; s < a.slots.size(); ++s) {
        const PlanSlot &x = a.slots[s], &y = b.slots[s];
        if (x.kind != y.kind || x.where != y.where || x.tag != y.tag || x.ref != y.ref || x.producer_of != y.producer_of) return false;
    }
    for (size_t g = 0; g < a.groups.size(); ++g)
        if (a.groups[g].key != b.groups[g].key || a.groups[g].slots != b.groups[g].slots) return false;
    return memcmp(a.opmap.data(), b.opmap.data(), sizeof(OpMap) * a.opmap.size()) == 0 && a.pred_used == b.pred_used &&
           a.pred_pass == b.pred_pass;
}

static void case11_options() {
    std::vector<dq_op> ops = heavy_ops(0);
    ops.push_back(op(DQ_OP_SIZE, -1, 0));
    ScanOptions off, vm, unfused;
    off.where_masks = false;
    vm.pred_vm = true;
    unfused.fused_producer = false;
    const Run a = run(table(kRows), kRows, ops, {compare(K, DQ_P_LT, 25)}, off);
    const Run b = run(table(kRows), kRows, ops, {compare(K, DQ_P_LT, 25)}, vm);
    CHECK(a.rc == DQ_OK && b.rc == DQ_OK);
    for (const Run* r : {&a, &b}) {
        const ScanPlan& p = r->plan;
        CHECK(!p.where[0].masked && !any_mask(p) && p.nstandalone == 0);  // nothing is masked
        CHECK(p.slots.size() == 2 && p.slots[0].where == 0 && p.slots[0].producer_of == -1);  // the value slot reads the bitmaps
        CHECK(p.slots[1].kind == SK_BITS && p.slots[1].tag == BT_SIZE && p.opmap[8].slot == 1);  // Size(where) pop-counts them
        CHECK(p.pred_used[0] == 1 && p.pred_pass[0] == 1);
        CHECK(p.groups[0].heavy == 1);  // under a where: not the branch-free variant
        for (int i = 0; i < 8; ++i) CHECK(p.opmap[i].wslot == 0);
        CHECK(p.opmap[8].wslot == 1);
    }
    CHECK(same_plan(a.plan, b.plan));  // both are the bitmap-pass plan
    const Run c = run(table(kRows), kRows, ops, {compare(K, DQ_P_LT, 25)}, unfused);
    CHECK(c.rc == DQ_OK && c.plan.where[0].masked && c.plan.where[0].producer == -1);  // masked, but from where_masks_kernel
    CHECK(c.plan.where[0].mask_col == std::vector<int>{K} && c.plan.nstandalone == 1 && c.plan.slots.back().kind == SK_WHERE);
}

static std::vector<int> stub_occ(const ScanPlan& p, int v) { return std::vector<int>(std::max<size_t>(p.groups.size(), 1), v); }

static void case12_zero_rows() {
    std::vector<dq_op> ops = heavy_ops(0);
    ops.push_back(op(DQ_OP_MEAN, L, 1));
    ops.push_back(op(DQ_OP_MIN_LENGTH, S, 1));
    ops.push_back(op(DQ_OP_SUM, W));
    const Run r = run(table(0), 0, ops, {compare(K, DQ_P_LT, 25), d_and_k()});
    CHECK(r.rc == DQ_OK);
    const std::vector<int> occ = stub_occ(r.plan, 2);
    for (bool concurrent : {false, true}) {
        const ScanGeometry g = plan_geometry(r.plan, 256, 0, INT64_MAX, concurrent, 1, 1, occ.data());
        for (int grid : g.grid) CHECK(grid == 1);  // no tiles: still one workgroup per launch
        CHECK(g.sgrid == 1 && g.dgrid == 1 && g.wgrid == 1 && g.gstride == 1);
        for (int32_t n : g.slot_nblocks) CHECK(n == 1);
        for (int32_t n : g.hll_nblocks) CHECK(n == 1);
        const std::vector<dq_column> cols = table(0);
        std::vector<dq_predicate> pv = {compare(K, DQ_P_LT, 25).view(), d_and_k().view()};
        Pred p0 = compare(K, DQ_P_LT, 25), p1 = d_and_k();
        pv = {p0.view(), p1.view()};
        const ScanLayout lay = layout_scan(r.plan, g, r.use, cols.data(), NCOLS, 0, (int)ops.size(), pv.data(), 2, false);
        CHECK(lay.arena_bytes > 0 && lay.out != kNoOffset && lay.pinned_bytes >= sizeof(dq_state) * ops.size());
    }
}

static void case13_geometry() {
    // two value groups (l under a standalone where, d without), a bits group, a string slot, a decimal128 slot
    const Run r = run(table(kRows), kRows,
                      {op(DQ_OP_MEAN, L, 0), op(DQ_OP_APPROX_COUNT_DISTINCT, D), op(DQ_OP_COMPLETENESS, K), op(DQ_OP_APPROX_COUNT_DISTINCT, S),
                       op(DQ_OP_APPROX_COUNT_DISTINCT, W)}, {d_and_k()});
    CHECK(r.rc == DQ_OK);
    const ScanPlan& p = r.plan;
    CHECK(p.groups.size() == 3 && p.nlaunch() == 4 && p.where[0].wslot == 3 && p.nhll == 3);
    const std::vector<int> occ = {2, 1, 3};
    ScanGeometry g = plan_geometry(p, 256, 100000, INT64_MAX, false, 700, 900, occ.data());
    CHECK(g.grid == (std::vector<int>{512, 256, 768}));  // cus * occupancy: the chip filled once
    CHECK(g.sgrid == 700 && g.dgrid == 900 && g.gstride == 900);  // gstride: the widest launch
    g = plan_geometry(p, 256, 300, INT64_MAX, false, 700, 0, occ.data());
    CHECK(g.grid == (std::vector<int>{300, 256, 300}));  // never more workgroups than tiles
    CHECK(g.gstride == 700 && g.wgrid == 300);  // wgrid: one workgroup per 4 chunks of 8 words = per tile, at most gstride
    g = plan_geometry(p, 256, 100000, 3, false, 700, 900, occ.data());
    CHECK(g.grid == (std::vector<int>{3, 3, 3}));  // the grid cap caps the groups only
    CHECK(g.sgrid == 700 && g.dgrid == 900);
    g = plan_geometry(p, 256, 100000, INT64_MAX, true, 700, 900, occ.data());
    CHECK(g.grid == (std::vector<int>{128, 64, 192}));  // concurrent: 1 / nlaunch of the chip each, rounded up
    CHECK(g.sgrid == 175 && g.dgrid == 900);  // the string launch shares, the decimal128 launch runs after the join
    CHECK(g.gstride == 900 && g.wgrid == 900);
    g = plan_geometry(p, 256, 100000, INT64_MAX, true, 701, 0, occ.data());
    CHECK(g.sgrid == 176 && g.gstride == 192 && g.wgrid == 192);  // max over groups, string and decimal128 grids
    CHECK(g.slot_nblocks.size() == 4);
    CHECK(g.slot_nblocks[p.groups[0].slots[0]] == 128 && g.slot_nblocks[p.groups[1].slots[0]] == 64 &&
          g.slot_nblocks[p.groups[2].slots[0]] == 192);  // a slot's partials: its group's grid
    CHECK(g.slot_nblocks[3] == g.wgrid);  // a standalone where's count slot is written by wgrid workgroups
    CHECK(g.hll_nblocks == (std::vector<int32_t>{g.slot_nblocks[p.opmap[1].slot], 176, 0}));  // value / string / decimal128 grid

    // the layout keeps every block apart, in order, 256-byte aligned, and sizes the staging for all of its uploads
    g = plan_geometry(p, 256, 25, INT64_MAX, false, 25, 25, occ.data());
    const std::vector<dq_column> cols = table(kRows);
    const Pred f = d_and_k();
    const dq_predicate pv = f.view();
    const ScanLayout lay = layout_scan(p, g, r.use, cols.data(), NCOLS, kRows, 5, &pv, 1, false);
    const size_t seq[] = {lay.pred[0].wout, lay.pred[0].mask0, lay.pcols, lay.status, lay.slots, lay.ops, lay.partials, lay.order,
                          lay.slot_nblocks, lay.hll_nblocks, lay.finals, lay.hll_partials, lay.hll_final, lay.out, lay.sslots,
                          lay.spartials, lay.sops, lay.dslots, lay.dpartials, lay.dops};
    for (size_t i = 0; i < sizeof(seq) / sizeof(seq[0]); ++i) {
        CHECK(seq[i] != kNoOffset && seq[i] % 256 == 0 && seq[i] < lay.arena_bytes);
        if (i) CHECK(seq[i] > seq[i - 1]);
    }
    CHECK(lay.pred[0].t == kNoOffset && lay.pred[0].prog == kNoOffset);  // masked, no bitmaps, no predicate pass
    CHECK(lay.pcols - lay.pred[0].mask0 >= lay.mask_stride && lay.mask_stride == (size_t)padded_words_for(kRows) * 8);
    CHECK(lay.partials - lay.ops >= sizeof(OpMap) * 5 && lay.order - lay.partials >= sizeof(SlotPartial) * 4 * g.gstride);
    CHECK(lay.arena_bytes - lay.dops >= sizeof(D128OpMap));
    CHECK(lay.pinned_bytes >= sizeof(WhereOut) + sizeof(SlotDesc) * 4 + sizeof(OpMap) * 5 + sizeof(dq_state) * 5 + sizeof(StrSlot) + sizeof(D128Slot));
    for (const ScanLayout::Column& c : lay.col) CHECK(c.values == kNoOffset);  // device columns are read in place
}

// ---- validate_predicate ---------------------------------------------------------------------------------------------
static std::vector<uint8_t> regex_image() {  // header {magic, ninstr, nclasses, nranges, ...} + one instruction
    const int32_t words[11] = {0, 1, 0, 0, 0, 0, 0, 0, 13, 0, 0};
    std::vector<uint8_t> b(sizeof(words));
    memcpy(b.data(), words, sizeof(words));
    return b;
}
static dq_const string_const(int64_t off, int32_t len) {
    dq_const c;
    memset(&c, 0, sizeof(c));
    c.tag = DQ_V_STRING;
    c.str_offset = off;
    c.str_len = len;
    return c;
}

static void expect_reject(const Pred& p, const std::vector<dq_column>& cols, int code, const char* text) {
    std::string msg;
    const dq_predicate v = p.view();
    const int rc = validate_predicate(v, cols.data(), (int)cols.size(), &msg);
    if (rc != code || msg.find(text) == std::string::npos) {
        ++g_failed;
        printf("FAILED: expected %d \"%s\", got %d \"%s\"\n", code, text, rc, msg.c_str());
    }
}

static void case14_rejected_examples() {
    std::vector<dq_column> cols = table(kRows);
    cols.push_back(column(DQ_TYPE_DECIMAL, true, kRows, 18, 19));  // index NCOLS: a scale validate_scan would refuse
    Pred p;
    expect_reject(p, cols, DQ_ERR_PREDICATE, "empty or odd-length program");
    p.code = {DQ_P_COL, K, DQ_P_NOT};
    expect_reject(p, cols, DQ_ERR_PREDICATE, "empty or odd-length program");
    Pred rx;
    rx.strings = regex_image();
    rx.consts = {string_const(0, 44)};
    rx.code = {DQ_P_COL, S, DQ_P_REGEX, 0};
    std::string msg;
    CHECK(validate_predicate(rx.view(), cols.data(), (int)cols.size(), &msg) == DQ_OK);  // the well-formed [COL, REGEX]
    rx.consts = {string_const(0, 40)};  // the header's counts no longer add up to the length
    expect_reject(rx, cols, DQ_ERR_PREDICATE, "malformed REGEX program");
    rx.consts = {string_const(0, 44)};
    rx.code = {DQ_P_COL, S, DQ_P_REGEX, 1};
    expect_reject(rx, cols, DQ_ERR_PREDICATE, "malformed REGEX program");
    rx.code = {DQ_P_COL, W, DQ_P_REGEX, 0};
    expect_reject(rx, cols, DQ_ERR_UNSUPPORTED, "PatternMatch over this column type is not supported");
    rx.code = {DQ_P_COL, NCOLS, DQ_P_REGEX, 0};
    expect_reject(rx, cols, DQ_ERR_UNSUPPORTED, "PatternMatch over a DECIMAL of scale 19");
    rx.code = {DQ_P_COL, S, DQ_P_REGEX, 0, DQ_P_NOT, 0};
    expect_reject(rx, cols, DQ_ERR_PREDICATE, "REGEX is only supported as [COL, REGEX]");
    rx.code = {DQ_P_COL, S, DQ_P_RLIKE, 0};
    CHECK(validate_predicate(rx.view(), cols.data(), (int)cols.size(), &msg) == DQ_OK);
    rx.consts = {string_const(2, 44)};  // not 4-byte aligned in the pool
    expect_reject(rx, cols, DQ_ERR_PREDICATE, "malformed RLIKE program");
    rx.consts = {string_const(4, 44)};  // past the pool
    expect_reject(rx, cols, DQ_ERR_PREDICATE, "malformed RLIKE program");
    Pred q = compare(K, DQ_P_LT, 25);
    q.code[1] = 99;
    expect_reject(q, cols, DQ_ERR_PREDICATE, "bad column 99");
    q.code[1] = -1;
    expect_reject(q, cols, DQ_ERR_PREDICATE, "bad column -1");
    q.code[1] = W;
    expect_reject(q, cols, DQ_ERR_UNSUPPORTED, "a predicate cannot read DECIMAL128 column");
    q = compare(K, DQ_P_LT, 25);
    q.code[3] = 1;
    expect_reject(q, cols, DQ_ERR_PREDICATE, "bad constant");
    q.code = {DQ_P_COL, K, DQ_P_CASE, 1};
    expect_reject(q, cols, DQ_ERR_PREDICATE, "CASE without WHEN");
    q.code = {DQ_P_COL, S, DQ_P_LIKE, 1};
    expect_reject(q, cols, DQ_ERR_PREDICATE, "bad LIKE pattern");
    q.code = {DQ_P_COL, K, DQ_P_LT, 0};
    expect_reject(q, cols, DQ_ERR_PREDICATE, "stack underflow");
    q.code = {DQ_P_COL, K, DQ_P_COL, K};
    expect_reject(q, cols, DQ_ERR_PREDICATE, "malformed program");  // two values left
    q.code.clear();
    for (int i = 0; i < kPredStack + 1; ++i) { q.code.push_back(DQ_P_COL); q.code.push_back(K); }
    for (int i = 0; i < kPredStack; ++i) { q.code.push_back(DQ_P_AND); q.code.push_back(0); }
    expect_reject(q, cols, DQ_ERR_PREDICATE, "malformed program");  // deeper than the VM's stack
    q.code.erase(q.code.begin(), q.code.begin() + 2);
    q.code.resize(q.code.size() - 2);
    CHECK(validate_predicate(q.view(), cols.data(), (int)cols.size(), &msg) == DQ_OK);  // exactly kPredStack deep
}

static uint64_t g_rng = 0x5EED0014u;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 11) % n);
}

// The test's own model of the VM's stack: operands popped per instruction, one value pushed.
static int pops_of(int op, int arg) {
    switch (op) {
        case DQ_P_COL: case DQ_P_CONST: case DQ_P_NULL: return 0;
        case DQ_P_NOT: case DQ_P_IS_NULL: case DQ_P_IS_NOT_NULL: case DQ_P_NEG: case DQ_P_LIKE: case DQ_P_LENGTH:
        case DQ_P_CAST_DOUBLE: case DQ_P_CAST_LONG: case DQ_P_CAST_STRING_NUM: case DQ_P_RLIKE: case DQ_P_LOWER: case DQ_P_UPPER:
        case DQ_P_TRIM: case DQ_P_ISNAN: case DQ_P_ABS: case DQ_P_YEAR: case DQ_P_MONTH: case DQ_P_DAY: return 1;
        case DQ_P_IN: return arg + 1;
        case DQ_P_COALESCE: case DQ_P_CASE: return arg;
        case DQ_P_SUBSTR: return 3;
        default: return 2;
    }
}

static void case14_random_programs() {
    static const int kOpcodes[] = {DQ_P_COL, DQ_P_CONST, DQ_P_NULL, DQ_P_EQ, DQ_P_NE, DQ_P_LT, DQ_P_LE, DQ_P_GT, DQ_P_GE,
                                   DQ_P_EQ_NULLSAFE, DQ_P_AND, DQ_P_OR, DQ_P_NOT, DQ_P_IS_NULL, DQ_P_IS_NOT_NULL, DQ_P_IN,
                                   DQ_P_COALESCE, DQ_P_ADD, DQ_P_SUB, DQ_P_MUL, DQ_P_DIV, DQ_P_MOD, DQ_P_NEG, DQ_P_LIKE,
                                   DQ_P_LENGTH, DQ_P_CAST_DOUBLE, DQ_P_CAST_LONG, DQ_P_CAST_STRING_NUM, DQ_P_REGEX, DQ_P_RLIKE,
                                   DQ_P_LOWER, DQ_P_UPPER, DQ_P_TRIM, DQ_P_CASE, DQ_P_ISNAN, DQ_P_ABS, DQ_P_SUBSTR, DQ_P_YEAR,
                                   DQ_P_MONTH, DQ_P_DAY, DQ_P_NANVL};
    const int nopcodes = (int)(sizeof(kOpcodes) / sizeof(kOpcodes[0]));
    const std::vector<dq_column> cols = table(kRows);
    const std::vector<uint8_t> image = regex_image();
    int accepted = 0;
    for (int iter = 0; iter < 20000; ++iter) {
        const int ninstr = 1 + (int)rnd(20);  // 2 .. 40 words
        const int nconsts = (int)rnd(4);
        // exactly-sized heap buffers: a read past any of them is an ASan report
        std::unique_ptr<int32_t[]> code(new int32_t[2 * ninstr]);
        std::unique_ptr<dq_const[]> consts(new dq_const[std::max(nconsts, 1)]);
        std::unique_ptr<uint8_t[]> strings(new uint8_t[image.size()]);
        memcpy(strings.get(), image.data(), image.size());
        for (int k = 0; k < nconsts; ++k)
            consts[k] = rnd(3) == 0 ? string_const(4 * (int64_t)rnd(2), 44 - 4 * (int32_t)rnd(2)) : long_const((int64_t)rnd(100));
        int depth = 0;
        for (int i = 0; i < ninstr; ++i) {
            int opc, arg;
            const int left = ninstr - 1 - i;
            if (rnd(10) < 9) {  // a well-formed step: push while there is room to fold back to one value, else fold
                const bool can_push = depth < kPredStack && depth + 1 - left <= 1;
                if (depth == 0 || (can_push && (depth < 2 || rnd(2)))) {
                    opc = rnd(3) ? DQ_P_COL : (nconsts ? DQ_P_CONST : DQ_P_NULL);
                    arg = opc == DQ_P_COL ? (int)rnd(W) : (int)rnd((uint32_t)std::max(nconsts, 1));
                } else if (depth >= 2 && (depth - left >= 1 || rnd(2))) {
                    static const int bin[] = {DQ_P_EQ, DQ_P_LT, DQ_P_AND, DQ_P_OR, DQ_P_ADD, DQ_P_NANVL, DQ_P_EQ_NULLSAFE};
                    opc = bin[rnd(7)];
                    arg = 0;
                } else {
                    static const int un[] = {DQ_P_NOT, DQ_P_IS_NULL, DQ_P_NEG, DQ_P_LENGTH, DQ_P_ABS, DQ_P_CAST_DOUBLE};
                    opc = un[rnd(6)];
                    arg = 0;
                }
            } else {  // anything: every opcode, and a few values that are none, with an argument around the valid range
                opc = rnd(8) ? kOpcodes[rnd((uint32_t)nopcodes)] : (int)rnd(70) - 5;
                arg = (int)rnd(14) - 3;
            }
            code[2 * i] = opc;
            code[2 * i + 1] = arg;
            depth += 1 - pops_of(opc, arg);
        }
        dq_predicate pr;
        pr.code = code.get();
        pr.code_len = 2 * ninstr;
        pr.n_consts = nconsts;
        pr.consts = consts.get();
        pr.strings = strings.get();
        pr.strings_len = (int64_t)image.size();
        std::string msg;
        std::vector<char> used(cols.size(), 0);
        const int rc = validate_predicate(pr, cols.data(), (int)cols.size(), &msg, used.data());
        CHECK(rc == DQ_OK || rc == DQ_ERR_PREDICATE || rc == DQ_ERR_UNSUPPORTED);
        CHECK((rc == DQ_OK) == msg.empty());
        if (rc != DQ_OK) continue;
        ++accepted;
        if (pr.code_len == 4 && code[2] == DQ_P_REGEX) continue;  // [COL, REGEX] runs on the regex kernel, not the VM
        int d = 0;
        bool ok = true;
        for (int i = 0; i < ninstr; ++i) {  // an accepted program keeps the VM's stack within 1 .. kPredStack
            d += 1 - pops_of(code[2 * i], code[2 * i + 1]);
            ok &= d >= 1 && d <= kPredStack;
            if (code[2 * i] == DQ_P_COL) ok &= code[2 * i + 1] >= 0 && code[2 * i + 1] < (int)cols.size() && used[code[2 * i + 1]];
            if (code[2 * i] == DQ_P_CONST || code[2 * i] == DQ_P_LIKE || code[2 * i] == DQ_P_RLIKE)
                ok &= code[2 * i + 1] >= 0 && code[2 * i + 1] < nconsts;  // and indexes nothing outside its tables
        }
        CHECK(ok && d == 1);  // and ends with exactly its result
    }
    printf("random programs accepted: %d of 20000\n", accepted);
    CHECK(accepted >= 200);  // the property above is not vacuous
}

// ---- plan_row_outcomes (call_plans.cpp) -----------------------------------------------------------------------------------
static dq_column host_column(int type, bool validity, int64_t nrows) {
    dq_column c = column(type, validity, nrows);
    c.flags = 0;
    return c;
}
static dq_row_term row_term(int kind, int index, int where, int check) {
    dq_row_term t;
    memset(&t, 0, sizeof(t));
    t.kind = kind;
    t.index = index;
    t.where = where;
    t.check = check;
    if (kind == DQ_ROW_BITS) t.pass_bits = t.considered_bits = (const uint8_t*)g_present;
    return t;
}
static dq_row_check row_check() {
    dq_row_check c;
    c.pass_bits = c.values = c.validity = (uint8_t*)g_present;
    return c;
}
struct RowRun {
    int rc = 0;
    std::string msg;
    RowPlan plan;
};
static RowRun row_run(const std::vector<dq_column>& cols, int64_t nrows, const std::vector<Pred>& preds,
                      const std::vector<dq_row_term>& terms, const std::vector<dq_row_check>& checks, uint32_t flags = 0,
                      bool pred_vm = false) {
    std::vector<dq_predicate> pv;
    for (const Pred& p : preds) pv.push_back(p.view());
    RowRun r;
    r.rc = plan_row_outcomes(cols.data(), (int)cols.size(), nrows, pv.data(), (int)pv.size(), terms.data(), (int)terms.size(),
                             checks.data(), (int)checks.size(), flags, pred_vm, &r.plan, &r.msg);
    return r;
}
static void expect_row_reject(const RowRun& r, int code, const char* text) {
    if (r.rc != code || r.msg != text) {
        ++g_failed;
        printf("FAILED: expected %d \"%s\", got %d \"%s\"\n", code, text, r.rc, r.msg.c_str());
    }
}

static void case15_row_term_order() {
    const int check_of[] = {2, 0, 1, 0, 2, 1, 0};
    std::vector<dq_row_term> terms;
    for (int c : check_of) terms.push_back(row_term(DQ_ROW_NOT_NULL, K, -1, c));
    const RowRun r = row_run(table(kRows), kRows, {}, terms, {row_check(), row_check(), row_check()});
    CHECK(r.rc == DQ_OK);
    const RowPlan& p = r.plan;
    CHECK(p.term.size() == terms.size() && p.term_begin.size() == 3 && p.term_end.size() == 3);
    CHECK(p.term_begin[0] == 0 && p.term_end[2] == (int)terms.size());  // the ranges partition the sorted terms
    for (int c = 0; c < 3; ++c) {
        if (c > 0) CHECK(p.term_begin[c] == p.term_end[c - 1]);
        CHECK(p.term_end[c] - p.term_begin[c] == (c == 0 ? 3 : 2));
        for (int i = p.term_begin[c]; i < p.term_end[c]; ++i) {
            CHECK(terms[p.term[i].term].check == c);
            if (i > p.term_begin[c]) CHECK(p.term[i].term > p.term[i - 1].term);  // stable
        }
    }
    // the read-back: counter pair i goes to the caller's term p.term[i].term, every term exactly once
    std::vector<int64_t> counts(2 * terms.size(), -1);
    for (size_t i = 0; i < p.term.size(); ++i) {
        CHECK(counts[2 * p.term[i].term] == -1);
        counts[2 * p.term[i].term] = 100 + (int64_t)i;
        counts[2 * p.term[i].term + 1] = 200 + (int64_t)i;
    }
    for (size_t t = 0; t < terms.size(); ++t) {
        const int64_t i = counts[2 * t] - 100;
        CHECK(i >= p.term_begin[check_of[t]] && i < p.term_end[check_of[t]] && counts[2 * t + 1] == 200 + i);
    }
}

static void case16_row_inline() {
    std::vector<Pred> preds;
    for (int i = 0; i < kRowInline + 1; ++i) preds.push_back(compare(K, DQ_P_LT, i));
    std::vector<dq_predicate> pv;
    for (const Pred& p : preds) pv.push_back(p.view());
    const std::vector<dq_row_term> terms = {row_term(DQ_ROW_PREDICATE, 0, 1, 0), row_term(DQ_ROW_PREDICATE, kRowInline, kRowInline, 0)};
    for (int vm = 0; vm < 2; ++vm) {
        std::vector<dq_column> cols = table(kRows);
        cols[K] = host_column(DQ_TYPE_LONG, true, kRows);  // an inline predicate's column is still staged
        const RowRun r = row_run(cols, kRows, preds, terms, {row_check()}, 0, vm != 0);
        CHECK(r.rc == DQ_OK);
        const RowPlan& p = r.plan;
        CHECK((int)p.inl.size() == (vm ? 0 : kRowInline));  // exactly 16 inline; none under pred_vm
        CHECK(p.use.col_used[K] == 1);
        for (int i = 0; i <= kRowInline; ++i) {
            const bool inl = !vm && i < kRowInline;
            CHECK(p.inline_of[i] == (inl ? i : -1));
            CHECK(p.options.pred_inline[i] == (inl ? 1 : 0));
            if (inl) CHECK(p.inl[i].col == K && p.inl[i].op == DQ_P_LT && p.inl[i].ci == i);
        }
        CHECK(!p.options.where_masks && p.options.pred_vm == (vm != 0));
        // the scan plan, made once: the 17th gets a pass, an inline predicate neither a pass nor bitmaps
        const std::vector<dq_op> ops = size_where_ops((int)pv.size());
        ScanPlan sp;
        std::string msg;
        CHECK(plan_scan(cols.data(), (int)cols.size(), kRows, ops.data(), (int)ops.size(), pv.data(), (int)pv.size(), p.use, p.options,
                        &sp, &msg) == DQ_OK);
        for (int i = 0; i <= kRowInline; ++i) {
            const bool inl = !vm && i < kRowInline;
            CHECK(sp.pred_pass[i] == (inl ? 0 : 1) && sp.pred_used[i] == (inl ? 0 : 1));
        }
        CHECK(p.term[0].src == (vm ? RP_PRED : RP_INLINE) && p.term[0].index == 0);
        CHECK(p.term[0].w_inline == (vm ? -1 : 1) && p.term[0].where == (vm ? 1 : -1));
        CHECK(p.term[1].src == RP_PRED && p.term[1].index == kRowInline && p.term[1].where == kRowInline && p.term[1].w_inline == -1);
    }
    const RowRun c = row_run(table(kRows), kRows, {d_and_k()}, {row_term(DQ_ROW_PREDICATE, 0, -1, 0)}, {row_check()});
    CHECK(c.rc == DQ_OK && c.plan.inl.empty() && c.plan.inline_of[0] == -1);  // a compound predicate is never inline
    CHECK(c.plan.term[0].src == RP_PRED && c.plan.term[0].index == 0 && c.plan.term[0].where == -1);
}

static void case17_row_sources() {
    // 0: device, 1: host and read by the predicate, 2: host, read by nobody, 3: the same without validity, 4: device without
    const std::vector<dq_column> cols = {column(DQ_TYPE_LONG, true, kRows), host_column(DQ_TYPE_LONG, true, kRows),
                                         host_column(DQ_TYPE_LONG, true, kRows), host_column(DQ_TYPE_LONG, false, kRows),
                                         column(DQ_TYPE_LONG, false, kRows)};
    std::vector<dq_row_term> terms = {row_term(DQ_ROW_BITS, 0, 0, 0)};
    for (int c = 0; c < 5; ++c) terms.push_back(row_term(DQ_ROW_NOT_NULL, c, -1, 0));
    Pred both = d_and_k();  // compound: reads columns 1 and 1
    both.code[1] = both.code[7] = 1;
    const RowRun r = row_run(cols, kRows, {both}, terms, {row_check()}, DQ_ROW_FILTERED_NULL);
    CHECK(r.rc == DQ_OK && r.plan.null_mode);
    const RowPlan& p = r.plan;
    CHECK(p.term[0].src == RP_BITS && p.term[0].term == 0 && p.term[0].where == -1 && p.term[0].w_inline == -1);
    const int want[] = {RP_VALID_DEVICE, RP_VALID_SCAN, RP_VALID_CALL, RP_ONES, RP_ONES};
    for (int c = 0; c < 5; ++c) CHECK(p.term[1 + c].src == want[c] && p.term[1 + c].index == c && p.term[1 + c].where == -1);
    CHECK(validity_source(cols[2], true) == RP_VALID_SCAN && validity_source(cols[0], false) == RP_VALID_DEVICE);
    // without predicates nothing is validated as a scan's column and nothing is read by one
    const RowRun n = row_run(cols, kRows, {}, {row_term(DQ_ROW_NOT_NULL, 1, -1, 0)}, {row_check()});
    CHECK(n.rc == DQ_OK && n.plan.term[0].src == RP_VALID_CALL && n.plan.inl.empty());
}

static void case18_row_refusals() {
    const std::vector<dq_column> cols = table(kRows);
    const std::vector<Pred> preds = {compare(K, DQ_P_LT, 25)};
    const std::vector<dq_row_check> one = {row_check()};
    auto reject = [&](const dq_row_term& t, int code, const char* text) { expect_row_reject(row_run(cols, kRows, preds, {t}, one), code, text); };
    reject(row_term(DQ_ROW_NOT_NULL, K, -1, 3), DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 names check 3");
    reject(row_term(DQ_ROW_NOT_NULL, K, -1, -1), DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 names check -1");
    reject(row_term(DQ_ROW_PREDICATE, 5, -1, 0), DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 names predicate 5");
    reject(row_term(DQ_ROW_NOT_NULL, 99, -1, 0), DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 names column 99");
    reject(row_term(DQ_ROW_NOT_NULL, K, 7, 0), DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 names predicate 7 as its where");
    reject(row_term(DQ_ROW_NOT_NULL, K, -2, 0), DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 names predicate -2 as its where");
    reject(row_term(9, K, -1, 0), DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 has kind 9");
    dq_row_term bits = row_term(DQ_ROW_BITS, 0, 0, 0);
    bits.considered_bits = nullptr;
    reject(bits, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term 0 has no bitmaps");
    bits.considered_bits = (const uint8_t*)g_present + 4;
    reject(bits, DQ_ERR_ALIGNMENT, "dq_row_outcomes: bitmaps must be 8-B aligned (term 0)");
    // output buffers
    const dq_row_term ok = row_term(DQ_ROW_NOT_NULL, K, -1, 0);
    const char* lacks = "dq_row_outcomes: check 0 lacks an output buffer";
    const char* misaligned = "dq_row_outcomes: check 0: bitmaps must be 8-B, the byte column 16-B aligned";
    dq_row_check ck = row_check();
    ck.pass_bits = nullptr;
    expect_row_reject(row_run(cols, kRows, preds, {ok}, {ck}), DQ_ERR_INVALID_ARGUMENT, lacks);
    ck = row_check();
    ck.values = nullptr;
    expect_row_reject(row_run(cols, kRows, preds, {ok}, {ck}), DQ_ERR_INVALID_ARGUMENT, lacks);
    ck = row_check();
    ck.validity = nullptr;
    CHECK(row_run(cols, kRows, preds, {ok}, {ck}).rc == DQ_OK);  // read in null mode only
    expect_row_reject(row_run(cols, kRows, preds, {ok}, {ck}, DQ_ROW_FILTERED_NULL), DQ_ERR_INVALID_ARGUMENT, lacks);
    ck = row_check();
    ck.pass_bits = (uint8_t*)g_present + 4;
    expect_row_reject(row_run(cols, kRows, preds, {ok}, {ck}), DQ_ERR_ALIGNMENT, misaligned);
    ck = row_check();
    ck.values = (uint8_t*)g_present + 8;
    expect_row_reject(row_run(cols, kRows, preds, {ok}, {ck}), DQ_ERR_ALIGNMENT, misaligned);
    ck = row_check();
    ck.validity = (uint8_t*)g_present + 4;
    CHECK(row_run(cols, kRows, preds, {ok}, {ck}).rc == DQ_OK);
    expect_row_reject(row_run(cols, kRows, preds, {ok}, {ck}, DQ_ROW_FILTERED_NULL), DQ_ERR_ALIGNMENT, misaligned);
    // a NOT_NULL column: device validity 8-B aligned, as many rows as the batch
    std::vector<dq_column> bad = cols;
    bad[L].validity = (const uint8_t*)g_present + 4;
    expect_row_reject(row_run(bad, kRows, {}, {row_term(DQ_ROW_NOT_NULL, L, -1, 0)}, one), DQ_ERR_ALIGNMENT,
                      "dq_row_outcomes: bitmaps must be 8-B aligned (column 1)");
    bad = cols;
    bad[L].length = 5;
    expect_row_reject(row_run(bad, kRows, {}, {row_term(DQ_ROW_NOT_NULL, L, -1, 0)}, one), DQ_ERR_INVALID_ARGUMENT,
                      "column 1 has 5 rows, batch has 50001");
    // the predicates as dq_scan validates them
    Pred broken = compare(K, DQ_P_LT, 25);
    broken.code[1] = 99;
    expect_row_reject(row_run(cols, kRows, {broken}, {ok}, one), DQ_ERR_PREDICATE, "predicate 0: bad column 99");
    // more than a launch takes
    const std::vector<dq_row_term> many(DQ_ROW_MAX_TERMS + 1, ok);
    expect_row_reject(row_run(cols, kRows, preds, many, one), DQ_ERR_UNSUPPORTED,
                      "dq_row_outcomes: 65 terms over 1 checks, at most 64 terms and 16 checks per call");
    expect_row_reject(row_run(cols, kRows, preds, {ok}, std::vector<dq_row_check>(DQ_ROW_MAX_CHECKS + 1, row_check())), DQ_ERR_UNSUPPORTED,
                      "dq_row_outcomes: 1 terms over 17 checks, at most 64 terms and 16 checks per call");
    CHECK(row_run(cols, kRows, preds, std::vector<dq_row_term>(DQ_ROW_MAX_TERMS, ok),
                  std::vector<dq_row_check>(DQ_ROW_MAX_CHECKS, row_check())).rc == DQ_OK);
}

// ---- plan_dict_scan, dict_lds_copies (call_plans.cpp) ----------------------------------------------------------------------
static dq_dict_column dict_column(int n_dict, int64_t nrows) {
    dq_dict_column d;
    memset(&d, 0, sizeof(d));
    d.flags = DQ_COL_DEVICE;
    d.length = nrows;
    d.indices = (const int32_t*)g_present;
    d.validity = (const uint8_t*)g_present;
    d.dictionary = column(DQ_TYPE_STRING, true, (int64_t)n_dict + 1);
    return d;
}
struct DictRun {
    int rc = 0;
    std::string msg;
    DictPlan plan;
};
static DictRun dict_run(const std::vector<dq_column>& cols, const std::vector<dq_dict_column>& dicts, int64_t nrows,
                        const std::vector<dq_op>& ops, const std::vector<Pred>& preds) {
    std::vector<dq_predicate> pv;
    for (const Pred& p : preds) pv.push_back(p.view());
    DictRun r;
    r.rc = plan_dict_scan(cols.data(), (int)cols.size(), dicts.data(), (int)dicts.size(), nrows, ops.data(), (int)ops.size(), pv.data(),
                          (int)pv.size(), DictOptions(), 64, &r.plan, &r.msg);
    return r;
}
static void expect_dict_reject(const DictRun& r, int code, const char* text) {
    if (r.rc != code || r.msg != text) {
        ++g_failed;
        printf("FAILED: expected %d \"%s\", got %d \"%s\"\n", code, text, r.rc, r.msg.c_str());
    }
}
// entry = 'abc'-shaped: [COL c, CONST 0, EQ]
static Pred entry_equals(int col) {
    Pred p = compare(col, DQ_P_EQ, 0);
    p.consts = {string_const(0, 3)};
    p.strings = {'a', 'b', 'c'};
    return p;
}
static size_t up16(size_t n) { return (n + 15) / 16 * 16; }
// The staging of one run_predicate, from the uploads it makes (an empty piece is not uploaded).
static size_t program_staging(const Pred& p) {
    return up16(4 * p.code.size()) + (p.consts.empty() ? 0 : up16(sizeof(dq_const) * p.consts.size())) +
           (p.strings.empty() ? 0 : up16(p.strings.size())) + up16(sizeof(PredProgram));
}

static void case19_dict_plan() {
    const std::vector<dq_column> cols = table(kRows);
    const std::vector<dq_dict_column> dicts = {dict_column(64, kRows), dict_column(1000, kRows)};
    const int D0 = NCOLS, D1 = NCOLS + 1;
    const std::vector<Pred> preds = {compare(K, DQ_P_LT, 25), d_and_k(), entry_equals(D1)};
    const std::vector<int32_t> callers_code = preds[2].code;
    const std::vector<dq_op> ops = {op(DQ_OP_MIN_LENGTH, D0),       op(DQ_OP_DATATYPE, D0),          op(DQ_OP_COMPLETENESS, D0, 0),
                                    op(DQ_OP_MAX_LENGTH, D0, 1),    op(DQ_OP_APPROX_COUNT_DISTINCT, D1), op(DQ_OP_COMPLIANCE, D1, -1, 2),
                                    op(DQ_OP_COMPLIANCE, D0, 0, 2)};
    const DictRun r = dict_run(cols, dicts, kRows, ops, preds);
    CHECK(r.rc == DQ_OK);
    const DictPlan& p = r.plan;
    // two ops on (dictionary 0, no where) share a slot with their flags OR-ed; the same dictionary under two filters: two more
    CHECK(p.slots.size() == 4);
    CHECK(p.opmap[0].slot == 0 && p.opmap[1].slot == 0 && p.slots[0].flags == (SF_LEN | SF_DTYPE));
    CHECK(p.opmap[2].slot == 1 && p.opmap[3].slot == 2 && p.opmap[6].slot == 1);
    CHECK(p.slots[1].dict == 0 && p.slots[1].where == 0 && p.slots[1].flags == 0);
    CHECK(p.slots[2].dict == 0 && p.slots[2].where == 1 && p.slots[2].flags == SF_LEN);
    CHECK(p.slots[3].dict == 1 && p.slots[3].where == -1 && p.slots[3].flags == SF_HLL && p.slots[3].n_dict == 1000);
    for (size_t i = 0; i < ops.size(); ++i) {
        const DictOpMap& m = p.opmap[i];
        CHECK(m.op == (int)i && m.kind == ops[i].kind && m.has_where == (ops[i].where >= 0) && m.sums == nullptr);
    }
    CHECK(p.where_used[0] && p.where_used[1] && !p.where_used[2]);
    // a Compliance op: a predicate op whose program copy reads column 0, the caller's program untouched
    CHECK(p.pops.size() == 2 && p.op_pop[5] == 0 && p.op_pop[6] == 1 && p.op_pop[0] == -1);
    CHECK(p.pops[0].pred == 2 && p.pops[0].slot == 3 && p.pops[1].pred == 2 && p.pops[1].slot == 1);
    for (const DictPlanPred& pop : p.pops) {
        CHECK(pop.code.size() == callers_code.size());
        for (size_t k = 0; k + 1 < pop.code.size(); k += 2)
            CHECK(pop.code[k] == callers_code[k] && pop.code[k + 1] == (pop.code[k] == DQ_P_COL ? 0 : callers_code[k + 1]));
    }
    CHECK(preds[2].code == callers_code && callers_code[1] == D1);
    std::vector<dq_predicate> pv;
    for (const Pred& q : preds) pv.push_back(q.view());
    const dq_predicate rewritten = dict_pop_predicate(p, 1, pv.data());
    CHECK(rewritten.code == p.pops[1].code.data() && rewritten.code_len == pv[2].code_len && rewritten.consts == pv[2].consts);
    CHECK(p.max_entries == 1000 && p.nstatus == 3 + 2);
    CHECK(p.slots[0].lds_copies == 8 && p.slots[3].lds_copies == 8 && p.lds_words == 8000);
    // the zero block: every slot's four ranges and the sums are disjoint and tile [0, zwords)
    std::vector<std::pair<size_t, size_t>> ranges = {{p.sums_off, 2 * p.pops.size()}};
    for (const DictPlanSlot& s : p.slots) {
        ranges.push_back({s.stats, (size_t)DS_COUNT});
        ranges.push_back({s.fold, (size_t)DF_COUNT});
        ranges.push_back({s.counts, (size_t)s.n_dict});
        ranges.push_back({s.hll, (size_t)kHllRegs * 4 / 8});
    }
    std::sort(ranges.begin(), ranges.end());
    size_t at = 0;
    for (const auto& rg : ranges) {
        CHECK(rg.first == at);
        at += rg.second;
    }
    CHECK(at == p.zwords);
    // staging: no smaller than every upload and read-back of the call, each 16-byte aligned, summed independently
    const size_t nslots = p.slots.size(), npops = p.pops.size(), nops = ops.size();
    size_t need = up16(sizeof(PredColumn) * (cols.size() + npops)) + program_staging(preds[0]) + program_staging(preds[1]) +
                  up16(sizeof(DictSlot) * nslots) + 2 * program_staging(preds[2]) + up16(sizeof(DictPredOp) * npops) +
                  up16(sizeof(DictOpMap) * nops) + up16(sizeof(dq_state) * nops) + up16(sizeof(int32_t) * p.nstatus) +
                  up16(sizeof(int64_t) * DS_COUNT * nslots);
    CHECK(p.pinned_bytes >= need);
    CHECK(p.pinned_bytes <= need + 64);  // and sized from them, not from a slack
    // no predicate op: the sums still get their two words, the status words their slot
    const DictRun n = dict_run(cols, dicts, kRows, {op(DQ_OP_COMPLETENESS, D0)}, {});
    CHECK(n.rc == DQ_OK && n.plan.pops.empty() && n.plan.zwords == n.plan.sums_off + 2 && n.plan.nstatus == 2);
}

static void case20_dict_refusals() {
    const std::vector<dq_column> cols = table(kRows);
    const std::vector<dq_dict_column> one = {dict_column(64, kRows)};
    const int D0 = NCOLS;
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLETENESS, K)}, {}), DQ_ERR_INVALID_ARGUMENT,
                       "op 0: column 0 names no dictionary column");
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLETENESS, D0 + 1)}, {}), DQ_ERR_INVALID_ARGUMENT,
                       "op 0: column 10 names no dictionary column");
    const std::string mean = "op 0: kind " + std::to_string((int)DQ_OP_MEAN) + " is not answered from a dictionary column";
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_MEAN, D0)}, {}), DQ_ERR_UNSUPPORTED, mean.c_str());
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLIANCE, D0)}, {}), DQ_ERR_INVALID_ARGUMENT,
                       "op 0: Compliance needs a predicate");
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLETENESS, D0, 1)}, {compare(K, DQ_P_LT, 25)}), DQ_ERR_INVALID_ARGUMENT,
                       "op 0: bad where index");
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLETENESS, D0, 0)}, {entry_equals(D0)}), DQ_ERR_UNSUPPORTED,
                       "op 0: its where reads a dictionary column");
    const char* plain = "dq_dict_scan: column 0 of a where must be a device column of the batch's rows";
    std::vector<dq_column> bad = cols;
    bad[K] = host_column(DQ_TYPE_LONG, true, kRows);
    expect_dict_reject(dict_run(bad, one, kRows, {op(DQ_OP_COMPLETENESS, D0, 0)}, {compare(K, DQ_P_LT, 25)}), DQ_ERR_UNSUPPORTED, plain);
    bad = cols;
    bad[S].flags |= DQ_COL_OFFSETS64;
    Pred s_null;
    s_null.code = {DQ_P_COL, S, DQ_P_IS_NULL, 0};
    expect_dict_reject(dict_run(bad, one, kRows, {op(DQ_OP_COMPLETENESS, D0, 0)}, {s_null}), DQ_ERR_UNSUPPORTED,
                       "dq_dict_scan: column 7 of a where must be a device column of the batch's rows");
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLETENESS, D0, 0)}, {compare(W, DQ_P_LT, 25)}), DQ_ERR_UNSUPPORTED,
                       "dq_dict_scan: column 8 of a where must be a device column of the batch's rows");
    bad = cols;
    bad[K].length = 5;
    expect_dict_reject(dict_run(bad, one, kRows, {op(DQ_OP_COMPLETENESS, D0, 0)}, {compare(K, DQ_P_LT, 25)}), DQ_ERR_UNSUPPORTED, plain);
    Pred broken = compare(K, DQ_P_LT, 25);
    broken.code[3] = 1;
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLETENESS, D0, 0)}, {broken}), DQ_ERR_PREDICATE,
                       "dq_dict_scan: predicate 0: bad constant");
    expect_dict_reject(dict_run(cols, one, kRows, {op(DQ_OP_COMPLIANCE, D0, -1, 0)}, {broken}), DQ_ERR_PREDICATE,
                       "dq_dict_scan: predicate 0: bad constant");
    // one slot per dictionary column: kMaxSlots pass, one more does not
    std::vector<dq_dict_column> many(kMaxSlots + 1, dict_column(4, kRows));
    std::vector<dq_op> many_ops;
    for (int d = 0; d <= kMaxSlots; ++d) many_ops.push_back(op(DQ_OP_COMPLETENESS, NCOLS + d));
    expect_dict_reject(dict_run(cols, many, kRows, many_ops, {}), DQ_ERR_UNSUPPORTED, "dq_dict_scan: more than 256 slots");
    many_ops.pop_back();
    CHECK(dict_run(cols, many, kRows, many_ops, {}).rc == DQ_OK);
    // check_dict_column, case by case
    const std::vector<dq_op> ops = {op(DQ_OP_COMPLETENESS, D0)};
    auto reject = [&](const dq_dict_column& d, int code, const char* text) { expect_dict_reject(dict_run(cols, {d}, kRows, ops, {}), code, text); };
    const char* device = "dictionary column 0: device buffers with int32 offsets only";
    const char* shape = "dictionary column 0: the dictionary is a STRING column of n_dict + 1 entries (the last one NULL) "
                        "with offsets, a validity bitmap and bytes";
    const char* align = "dictionary column 0: misaligned buffer";
    dq_dict_column d = dict_column(64, kRows);
    d.flags = 0;
    reject(d, DQ_ERR_UNSUPPORTED, device);
    d = dict_column(64, kRows);
    d.dictionary.flags = 0;
    reject(d, DQ_ERR_UNSUPPORTED, device);
    d = dict_column(64, kRows);
    d.dictionary.flags |= DQ_COL_OFFSETS64;
    reject(d, DQ_ERR_UNSUPPORTED, device);
    d = dict_column(64, 5);
    reject(d, DQ_ERR_INVALID_ARGUMENT, "dictionary column 0 has 5 rows, batch has 50001");
    d = dict_column(64, kRows);
    d.indices = nullptr;
    reject(d, DQ_ERR_INVALID_ARGUMENT, "dictionary column 0 has 50001 rows, batch has 50001");
    d = dict_column(64, kRows);
    d.dictionary.spark_type = DQ_TYPE_LONG;
    reject(d, DQ_ERR_INVALID_ARGUMENT, shape);
    d = dict_column(64, kRows);
    d.dictionary.length = 0;
    reject(d, DQ_ERR_INVALID_ARGUMENT, shape);
    d.dictionary.length = INT32_MAX;
    reject(d, DQ_ERR_INVALID_ARGUMENT, shape);
    d = dict_column(64, kRows);
    d.dictionary.offsets = nullptr;
    reject(d, DQ_ERR_INVALID_ARGUMENT, shape);
    d = dict_column(64, kRows);
    d.dictionary.validity = nullptr;
    reject(d, DQ_ERR_INVALID_ARGUMENT, shape);
    d = dict_column(64, kRows);
    d.dictionary.values = nullptr;
    reject(d, DQ_ERR_INVALID_ARGUMENT, shape);
    d = dict_column(64, kRows);
    d.indices = (const int32_t*)(g_present + 2);
    reject(d, DQ_ERR_ALIGNMENT, align);
    d = dict_column(64, kRows);
    d.validity = (const uint8_t*)g_present + 4;
    reject(d, DQ_ERR_ALIGNMENT, align);
    d = dict_column(64, kRows);
    d.dictionary.values = g_present + 2;
    reject(d, DQ_ERR_ALIGNMENT, align);
    d = dict_column(64, kRows);
    d.dictionary.offsets = (const int32_t*)(g_present + 2);
    reject(d, DQ_ERR_ALIGNMENT, align);
    d = dict_column(64, kRows);
    d.dictionary.validity = (const uint8_t*)g_present + 4;
    reject(d, DQ_ERR_ALIGNMENT, align);
    d = dict_column(64, kRows);
    d.validity = nullptr;  // all rows valid
    CHECK(dict_run(cols, {d}, kRows, ops, {}).rc == DQ_OK);
    std::string msg;
    CHECK(check_dict_column(dict_column(1, 0), 0, 0, &msg) == DQ_OK && msg.empty());
}

static void case21_dict_lds_copies() {
    const DictOptions dflt;
    CHECK(dflt.lds_entries == kDictLdsWords && dflt.lds_copies == kDictLdsCopies);
    CHECK(dict_lds_copies(dflt, 0, kRows, 64) == 0);
    CHECK(dict_lds_copies(dflt, 10, kRows, 64) == 8);
    DictOptions o;
    o.lds_entries = 100;
    CHECK(dict_lds_copies(o, 100, kRows, 64) == 8 && dict_lds_copies(o, 101, kRows, 64) == 0);
    o.lds_entries = 0;
    CHECK(dict_lds_copies(o, 1, kRows, 64) == 0);
    o.lds_entries = 1 << 20;  // never more than the LDS holds
    CHECK(dict_lds_copies(o, kDictLdsWords, kRows, 64) == 1 && dict_lds_copies(o, kDictLdsWords + 1, kRows, 64) == 0);
    // copies halve until they fit kDictLdsCopyWords = 8192 words
    CHECK(dict_lds_copies(dflt, 1024, kRows, 64) == 8 && dict_lds_copies(dflt, 1025, kRows, 64) == 4);
    CHECK(dict_lds_copies(dflt, 2048, kRows, 64) == 4 && dict_lds_copies(dflt, 2049, kRows, 64) == 2);
    CHECK(dict_lds_copies(dflt, 4097, kRows, 64) == 1 && dict_lds_copies(dflt, kDictLdsWords, kRows, 64) == 1);
    CHECK(dict_lds_copies(dflt, kDictLdsWords + 1, kRows, 64) == 0);
    // a workgroup's rows, nrows / grid + 2 tiles, stay below 2^31
    const int64_t cut = ((int64_t)1 << 31) - 2 * kDictTileRows;
    CHECK(dict_lds_copies(dflt, 10, cut - 1, 1) == 8 && dict_lds_copies(dflt, 10, cut, 1) == 0);
    CHECK(dict_lds_copies(dflt, 10, 64 * cut - 1, 64) == 8 && dict_lds_copies(dflt, 10, 64 * cut, 64) == 0);
    for (int c : {1, 2, 4}) {
        o = DictOptions();
        o.lds_copies = c;
        CHECK(dict_lds_copies(o, 10, kRows, 64) == c);
        CHECK(dict_lds_copies(o, 4097, kRows, 64) == 1);
    }
    for (int c : {3, 0, -1, 16}) {  // ignored
        o = DictOptions();
        o.lds_copies = c;
        CHECK(dict_lds_copies(o, 10, kRows, 64) == 8);
    }
}

int main() {
    case1_heavy2();
    case2_fused_producer();
    case3_pair_sharing();
    case4_mixed_sizes();
    case5_standalone_where();
    case6_fallback();
    case7_two_constants();
    case8_unread_completeness();
    case9_hll_numbering();
    case10_too_many_slots();
    case11_options();
    case12_zero_rows();
    case13_geometry();
    case14_rejected_examples();
    case14_random_programs();
    case15_row_term_order();
    case16_row_inline();
    case17_row_sources();
    case18_row_refusals();
    case19_dict_plan();
    case20_dict_refusals();
    case21_dict_lds_copies();
    if (g_failed) {
        printf("scan_plan_checks: %d FAILED\n", g_failed);
        return 1;
    }
    printf("scan_plan_checks: ok\n");
    return 0;
}
