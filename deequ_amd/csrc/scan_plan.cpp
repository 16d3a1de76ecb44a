// scan_plan.cpp — validation, slot plan, launch geometry and arena layout of dq_scan as pure host functions
// (scan_plan.h). Also built with -DDQ_HOST_ONLY under ASan / UBSan by tests/sanitize_scan_plan.
#include "scan_plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <utility>

namespace dq {

int failf(std::string* msg, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (msg) *msg = buf;
    return code;
}

namespace {

bool is_numeric_type(int t) {
    // Preconditions.isNumeric (A/Analyzer.scala:329-343)
    return t == DQ_TYPE_BYTE || t == DQ_TYPE_SHORT || t == DQ_TYPE_INT || t == DQ_TYPE_LONG ||
           t == DQ_TYPE_FLOAT || t == DQ_TYPE_DOUBLE || t == DQ_TYPE_DECIMAL;
}

// A STRING constant holding a compiled regex image, 4-byte aligned inside the string pool.
bool regex_const_ok(const dq_predicate& pr, int k) {
    if (k < 0 || k >= pr.n_consts) return false;
    const dq_const& c = pr.consts[k];
    return c.tag == DQ_V_STRING && c.str_offset >= 0 && !(c.str_offset & 3) && c.str_offset + c.str_len <= pr.strings_len &&
           rx::rx_image_ok(pr.strings + c.str_offset, c.str_len);
}

bool is_regex_program(const dq_predicate& pr) { return pr.code_len == 4 && pr.code[2] == DQ_P_REGEX; }

}  // namespace

int validate_predicate(const dq_predicate& pr, const dq_column* columns, int ncols, std::string* msg, char* col_used) {
    auto col_ok = [&](int c) { return c >= 0 && c < ncols; };
    if (pr.code_len <= 0 || (pr.code_len & 1) || !pr.code) return failf(msg, DQ_ERR_PREDICATE, "empty or odd-length program");
    if (is_regex_program(pr)) {
        const int c = pr.code[1];
        if (pr.code[0] != DQ_P_COL || !col_ok(c) || !regex_const_ok(pr, pr.code[3]))
            return failf(msg, DQ_ERR_PREDICATE, "malformed REGEX program");
        const int t = columns[c].spark_type;
        if (t < DQ_TYPE_BOOLEAN || t > DQ_TYPE_DECIMAL)
            return failf(msg, DQ_ERR_UNSUPPORTED, "PatternMatch over this column type is not supported");
        if (t == DQ_TYPE_DECIMAL && (columns[c].decimal_scale < 0 || columns[c].decimal_scale > 18))
            return failf(msg, DQ_ERR_UNSUPPORTED, "PatternMatch over a DECIMAL of scale %d", columns[c].decimal_scale);
        if (col_used) col_used[c] = 1;
        return DQ_OK;
    }
    int depth = 0, maxd = 0;  // the VM's stack, simulated
    for (int k = 0; k < pr.code_len; k += 2) {
        const int op = pr.code[k], arg = pr.code[k + 1];
        if (op == DQ_P_COL) {
            if (!col_ok(arg)) return failf(msg, DQ_ERR_PREDICATE, "bad column %d", arg);
            if (columns[arg].spark_type == DQ_TYPE_DECIMAL128)
                return failf(msg, DQ_ERR_UNSUPPORTED, "a predicate cannot read DECIMAL128 column %d", arg);
            if (col_used) col_used[arg] = 1;
            ++depth;
        } else if (op == DQ_P_CONST || op == DQ_P_NULL) {
            if (op == DQ_P_CONST && (arg < 0 || arg >= pr.n_consts)) return failf(msg, DQ_ERR_PREDICATE, "bad constant");
            ++depth;
        } else if (op == DQ_P_REGEX) {
            return failf(msg, DQ_ERR_PREDICATE, "REGEX is only supported as [COL, REGEX]");
        } else if (op == DQ_P_IN) {
            depth -= arg;
        } else if (op == DQ_P_COALESCE) {
            depth -= arg - 1;
        } else if (op == DQ_P_CASE) {
            if (arg < 2) return failf(msg, DQ_ERR_PREDICATE, "CASE without WHEN");
            depth -= arg - 1;  // 2 * #WHEN + has ELSE operands -> 1
        } else if (op == DQ_P_SUBSTR) {
            depth -= 2;
        } else if (op == DQ_P_NOT || op == DQ_P_IS_NULL || op == DQ_P_IS_NOT_NULL || op == DQ_P_NEG ||
                   op == DQ_P_LIKE || op == DQ_P_LENGTH || op == DQ_P_CAST_DOUBLE || op == DQ_P_CAST_LONG ||
                   op == DQ_P_CAST_STRING_NUM || op == DQ_P_RLIKE || op == DQ_P_LOWER || op == DQ_P_UPPER ||
                   op == DQ_P_TRIM || op == DQ_P_ISNAN || op == DQ_P_ABS || op == DQ_P_YEAR || op == DQ_P_MONTH ||
                   op == DQ_P_DAY) {
            if (op == DQ_P_LIKE && (arg < 0 || arg >= pr.n_consts)) return failf(msg, DQ_ERR_PREDICATE, "bad LIKE pattern");
            if (op == DQ_P_RLIKE && !regex_const_ok(pr, arg)) return failf(msg, DQ_ERR_PREDICATE, "malformed RLIKE program");
        } else {
            --depth;
        }
        if (depth < 1) return failf(msg, DQ_ERR_PREDICATE, "stack underflow");
        maxd = std::max(maxd, depth);
    }
    if (depth != 1 || maxd > kPredStack) return failf(msg, DQ_ERR_PREDICATE, "malformed program");
    return DQ_OK;
}

int validate_scan(const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops, const dq_predicate* preds,
                  int npreds, ScanUse* use, std::string* msg) {
    for (int c = 0; c < ncols; ++c) {
        const dq_column& col = columns[c];
        if (col.length != nrows)
            return failf(msg, DQ_ERR_INVALID_ARGUMENT, "column %d has %lld rows, batch has %lld", c, (long long)col.length,
                         (long long)nrows);
        if (col.spark_type < DQ_TYPE_BOOLEAN || col.spark_type > DQ_TYPE_DECIMAL128)
            return failf(msg, DQ_ERR_UNSUPPORTED, "column %d: unknown spark type %d", c, col.spark_type);
        const bool wide = col.spark_type == DQ_TYPE_DECIMAL128;
        if (wide && (col.decimal_precision < 19 || col.decimal_precision > 38 || col.decimal_scale < 0 ||
                     col.decimal_scale > col.decimal_precision))
            return failf(msg, DQ_ERR_UNSUPPORTED, "column %d: DECIMAL128 needs 19 <= precision <= 38 and 0 <= scale <= precision", c);
        if (col.spark_type == DQ_TYPE_STRING && nrows > 0 && !col.offsets)
            return failf(msg, DQ_ERR_INVALID_ARGUMENT, "string column %d without offsets", c);
        if (col.flags & DQ_COL_OFFSETS64)
            return failf(msg, DQ_ERR_UNSUPPORTED, "column %d: int64 string offsets are for the grouping builds only", c);
        if (col.spark_type == DQ_TYPE_DECIMAL && (col.decimal_precision > 18 || col.decimal_scale < 0 || col.decimal_scale > 18))
            return failf(msg, DQ_ERR_UNSUPPORTED, "column %d: decimal precision > 18 unsupported", c);
        if ((col.flags & DQ_COL_DEVICE) && nrows > 0) {
            const int e = elem_of(col.spark_type);
            // strings: 4-byte aligned UTF-8 (read as dwords), padded by 16 bytes past offsets[length]
            const size_t va = wide ? 16 : (e == ET_NONE ? 4 : (elem_size(e) == 1 ? 8 : 16));
            if (((uintptr_t)col.values % va) != 0 || ((uintptr_t)col.validity % 8) != 0)
                return failf(msg, DQ_ERR_ALIGNMENT, "device column %d: values must be %zu-byte and validity 8-byte aligned", c, va);
        }
    }
    auto col_ok = [&](int c) { return c >= 0 && c < ncols; };
    std::vector<char>& pred_used = use->pred_used;
    std::vector<char>& col_used = use->col_used;
    pred_used.assign(npreds, 0);
    col_used.assign(ncols, 0);
    // ops over a DECIMAL128 column: answered by the decimal128 launch, never by a value / bits / string slot
    use->wide_op.assign(nops, 0);
    for (int i = 0; i < nops; ++i) {
        const dq_op& op = ops[i];
        if (op.where >= npreds || op.where < -1) return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: bad where index", i);
        if (op.where >= 0) pred_used[op.where] = 1;
        if (op.kind != DQ_OP_SIZE && op.kind != DQ_OP_COMPLIANCE) {
            const bool w0 = col_ok(op.column[0]) && columns[op.column[0]].spark_type == DQ_TYPE_DECIMAL128;
            const bool w1 = op.kind == DQ_OP_CORRELATION && col_ok(op.column[1]) &&
                            columns[op.column[1]].spark_type == DQ_TYPE_DECIMAL128;
            if (w0 || w1) {
                const bool ok = op.kind == DQ_OP_COMPLETENESS || op.kind == DQ_OP_MEAN || op.kind == DQ_OP_SUM ||
                                op.kind == DQ_OP_MINIMUM || op.kind == DQ_OP_MAXIMUM ||
                                op.kind == DQ_OP_STANDARD_DEVIATION || op.kind == DQ_OP_APPROX_COUNT_DISTINCT;
                if (!ok) return failf(msg, DQ_ERR_UNSUPPORTED, "op %d: kind %d is not supported over a DECIMAL128 column", i, op.kind);
                use->wide_op[i] = 1;
                col_used[op.column[0]] = 1;
                continue;
            }
        }
        switch (op.kind) {
            case DQ_OP_SIZE: break;
            case DQ_OP_COMPLIANCE:
                if (op.predicate < 0 || op.predicate >= npreds)
                    return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: Compliance needs a predicate", i);
                pred_used[op.predicate] = 1;
                break;
            case DQ_OP_COMPLETENESS:
                if (!col_ok(op.column[0])) return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: bad column", i);
                col_used[op.column[0]] = 1;
                break;
            case DQ_OP_MEAN: case DQ_OP_SUM: case DQ_OP_MINIMUM: case DQ_OP_MAXIMUM: case DQ_OP_STANDARD_DEVIATION:
                if (!col_ok(op.column[0])) return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: bad column", i);
                if (!is_numeric_type(columns[op.column[0]].spark_type))
                    return failf(msg, DQ_ERR_UNSUPPORTED, "op %d: column %d is not numeric", i, op.column[0]);
                col_used[op.column[0]] = 1;
                break;
            case DQ_OP_CORRELATION:
                if (!col_ok(op.column[0]) || !col_ok(op.column[1]))
                    return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: bad column", i);
                if (!is_numeric_type(columns[op.column[0]].spark_type) || !is_numeric_type(columns[op.column[1]].spark_type))
                    return failf(msg, DQ_ERR_UNSUPPORTED, "op %d: correlation needs numeric columns", i);
                col_used[op.column[0]] = col_used[op.column[1]] = 1;
                break;
            case DQ_OP_APPROX_COUNT_DISTINCT:
            case DQ_OP_DATATYPE:
                if (!col_ok(op.column[0])) return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: bad column", i);
                col_used[op.column[0]] = 1;
                break;
            case DQ_OP_MIN_LENGTH: case DQ_OP_MAX_LENGTH:
                if (!col_ok(op.column[0])) return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: bad column", i);
                if (columns[op.column[0]].spark_type != DQ_TYPE_STRING)
                    return failf(msg, DQ_ERR_UNSUPPORTED, "op %d: MinLength/MaxLength need a string column", i);
                col_used[op.column[0]] = 1;
                break;
            default:
                return failf(msg, DQ_ERR_UNSUPPORTED, "op %d: kind %d not implemented by the fused scan", i, op.kind);
        }
    }
    for (int p = 0; p < npreds; ++p) {
        if (!pred_used[p]) continue;
        std::string why;
        const int rc = validate_predicate(preds[p], columns, ncols, &why, col_used.data());
        if (rc) return failf(msg, rc, "predicate %d: %s", p, why.c_str());
    }
    return DQ_OK;
}

size_t pred_stage_bytes(const dq_predicate& pr) {
    return align_up(sizeof(PredProgram), 16) + align_up(sizeof(int32_t) * (size_t)pr.code_len, 16) +
           align_up(sizeof(dq_const) * (size_t)std::max(pr.n_consts, 0), 16) + align_up((size_t)std::max<int64_t>(pr.strings_len, 0), 16);
}

bool compile_simple_predicate(const dq_predicate& pr, const dq_column* columns, int ncols, PredSimple& out) {
    memset(&out, 0, sizeof(out));
    enum { E_COL, E_CONST, E_BOOL };
    struct Ent { int kind, idx; bool neg = false; };  // neg: a constant under unary minus (`x < -1`)
    std::vector<Ent> st;
    auto fixed_numeric = [&](int c) {
        if (c < 0 || c >= ncols) return false;
        switch (columns[c].spark_type) {
            case DQ_TYPE_BOOLEAN: case DQ_TYPE_BYTE: case DQ_TYPE_SHORT: case DQ_TYPE_INT: case DQ_TYPE_DATE:
            case DQ_TYPE_LONG: case DQ_TYPE_TIMESTAMP: case DQ_TYPE_FLOAT: case DQ_TYPE_DOUBLE: return true;
            default: return false;
        }
    };
    auto emit = [&](int b) {
        if (out.nb >= kPredBCode) return false;
        out.b[out.nb++] = (int8_t)b;
        return true;
    };
    auto term = [&](int col, int op, int k, bool neg = false) -> int {  // k: constant index, or -1 for IS [NOT] NULL
        if (out.nterms >= kPredTerms) return -1;
        PredTerm& q = out.t[out.nterms];
        q.col = col;
        q.op = op;
        if (k >= 0) {
            const dq_const& c = pr.consts[k];
            const int ty = columns[col].spark_type;
            q.dbl = (ty == DQ_TYPE_FLOAT || ty == DQ_TYPE_DOUBLE || c.tag == DQ_V_DOUBLE) ? 1 : 0;
            // Spark's UnaryMinus on a literal: a Long negates with wrap-around, a Double flips its sign
            q.ci = neg ? (int64_t)(0ull - (uint64_t)c.i64) : c.i64;
            q.cd = c.tag == DQ_V_DOUBLE ? (neg ? -c.f64 : c.f64) : (double)q.ci;
        }
        return out.nterms++;
    };
    auto flip = [](int op) {
        switch (op) {
            case DQ_P_LT: return (int)DQ_P_GT;
            case DQ_P_LE: return (int)DQ_P_GE;
            case DQ_P_GT: return (int)DQ_P_LT;
            case DQ_P_GE: return (int)DQ_P_LE;
            default: return op;
        }
    };
    auto const_ok = [&](int k) {
        if (k < 0 || k >= pr.n_consts) return false;
        const int tag = pr.consts[k].tag;
        return tag == DQ_V_BOOL || tag == DQ_V_LONG || tag == DQ_V_DOUBLE;
    };
    for (int pc = 0; pc + 1 < pr.code_len; pc += 2) {
        const int op = pr.code[pc], arg = pr.code[pc + 1];
        switch (op) {
            case DQ_P_COL:
                if (!fixed_numeric(arg)) return false;
                st.push_back({E_COL, arg});
                break;
            case DQ_P_CONST:
                if (!const_ok(arg)) return false;
                st.push_back({E_CONST, arg});
                break;
            case DQ_P_EQ: case DQ_P_NE: case DQ_P_LT: case DQ_P_LE: case DQ_P_GT: case DQ_P_GE: {
                if (st.size() < 2) return false;
                const Ent b = st.back(); st.pop_back();
                const Ent a = st.back(); st.pop_back();
                int k;
                if (a.kind == E_COL && b.kind == E_CONST) k = term(a.idx, op, b.idx, b.neg);
                else if (a.kind == E_CONST && b.kind == E_COL) k = term(b.idx, flip(op), a.idx, a.neg);
                else return false;
                if (k < 0 || !emit(k)) return false;
                st.push_back({E_BOOL, 0});
                break;
            }
            case DQ_P_IS_NULL: case DQ_P_IS_NOT_NULL: {
                if (st.empty() || st.back().kind != E_COL) return false;
                const int k = term(st.back().idx, op, -1);
                st.pop_back();
                if (k < 0 || !emit(k)) return false;
                st.push_back({E_BOOL, 0});
                break;
            }
            case DQ_P_AND: case DQ_P_OR: {
                if (st.size() < 2 || st[st.size() - 1].kind != E_BOOL || st[st.size() - 2].kind != E_BOOL) return false;
                st.pop_back();
                if (!emit(op == DQ_P_AND ? kPB_AND : kPB_OR)) return false;
                break;
            }
            case DQ_P_NOT:
                if (st.empty() || st.back().kind != E_BOOL || !emit(kPB_NOT)) return false;
                break;
            case DQ_P_NEG: {  // -constant (a LONG / DOUBLE literal): folded into the leaf's constant
                if (st.empty() || st.back().kind != E_CONST) return false;
                const int tag = pr.consts[st.back().idx].tag;
                if (tag != DQ_V_LONG && tag != DQ_V_DOUBLE) return false;
                st.back().neg = !st.back().neg;
                break;
            }
            case DQ_P_IN: {  // x IN (c1..cn) with non-NULL constants == (x = c1) OR ... OR (x = cn)
                const int n = arg;
                if (n < 1 || (int)st.size() < n + 1) return false;
                const size_t base = st.size() - n - 1;
                if (st[base].kind != E_COL) return false;
                for (int i = 0; i < n; ++i) {
                    if (st[base + 1 + i].kind != E_CONST) return false;
                    const int k = term(st[base].idx, DQ_P_EQ, st[base + 1 + i].idx, st[base + 1 + i].neg);
                    if (k < 0 || !emit(k)) return false;
                    if (i > 0 && !emit(kPB_OR)) return false;
                }
                st.resize(base);
                st.push_back({E_BOOL, 0});
                break;
            }
            default:
                return false;
        }
        if (st.size() > 24) return false;
    }
    return st.size() == 1 && st[0].kind == E_BOOL && out.nterms > 0;
}

namespace {

// A (column, where) pair's share of a value slot.
struct Use {
    uint32_t flags = 0;
    int slot = -1, pos = 0, hll = -1;
    int pred_op = 0, pred_kind = FP_NONE;  // fused `col <op> const` Compliance predicate
    int64_t pred_i = 0;
    double pred_d = 0.0;
};
using UseMap = std::map<std::pair<int, int>, Use>;  // (column, where) -> use

// `col <op> const` (or its mirror) on a non-decimal numeric column: Compliance evaluated inside that column's scan.
// Returns the column, -1 when the predicate is not of that form or the column's scan already carries another one.
int fuse_compliance(const dq_predicate& pr, const dq_column* columns, int where, UseMap& uses) {
    if (pr.code_len != 6) return -1;
    int a = pr.code[0], aa = pr.code[1], b = pr.code[2], ba = pr.code[3], cmp = pr.code[4];
    if (cmp < DQ_P_EQ || cmp > DQ_P_GE) return -1;
    if (a == DQ_P_CONST && b == DQ_P_COL) {  // const <op> col  ->  col <op'> const
        std::swap(a, b);
        std::swap(aa, ba);
        if (cmp == DQ_P_LT) cmp = DQ_P_GT;
        else if (cmp == DQ_P_GT) cmp = DQ_P_LT;
        else if (cmp == DQ_P_LE) cmp = DQ_P_GE;
        else if (cmp == DQ_P_GE) cmp = DQ_P_LE;
    }
    if (a != DQ_P_COL || b != DQ_P_CONST || ba < 0 || ba >= pr.n_consts) return -1;
    const dq_const& k = pr.consts[ba];
    const int t = columns[aa].spark_type;
    if (!(t >= DQ_TYPE_BYTE && t <= DQ_TYPE_DOUBLE) || (k.tag != DQ_V_LONG && k.tag != DQ_V_DOUBLE)) return -1;
    Use& u = uses[std::make_pair(aa, where)];
    const int kind = k.tag == DQ_V_LONG ? FP_LONG : FP_DOUBLE;
    if (u.pred_kind != FP_NONE &&
        !(u.pred_op == cmp && u.pred_kind == kind && u.pred_i == k.i64 && (kind == FP_LONG || u.pred_d == k.f64)))
        return -1;  // one fused predicate per column scan; others use the predicate VM
    u.pred_op = cmp;
    u.pred_kind = kind;
    u.pred_i = k.i64;
    u.pred_d = k.f64;
    return aa;
}

int new_slot(ScanPlan& plan, int kind) {
    PlanSlot s;
    s.kind = kind;
    plan.slots.push_back(s);
    return (int)plan.slots.size() - 1;
}

// Column uses -> value slots: Correlation pairs first (both columns' uses ride in the pair slot), then one slot per
// remaining (column, where). op_slot: the Correlation ops' (slot, colpos), colpos 1 = the pair is stored swapped.
void plan_value_slots(ScanPlan& plan, const dq_column* columns, const dq_op* ops, int nops, UseMap& uses,
                      std::vector<std::pair<int, int>>& op_slot) {
    std::map<std::tuple<int, int, int>, int> pair_slots;  // (x, y, where) -> slot with corr
    for (int i = 0; i < nops; ++i) {
        const dq_op& op = ops[i];
        if (op.kind != DQ_OP_CORRELATION) continue;
        const int x = op.column[0], y = op.column[1], w = op.where;
        auto it = pair_slots.find(std::make_tuple(x, y, w));
        if (it != pair_slots.end()) { op_slot[i] = {it->second, 0}; continue; }
        it = pair_slots.find(std::make_tuple(y, x, w));
        if (it != pair_slots.end()) { op_slot[i] = {it->second, 1}; continue; }
        const int ex = elem_of(columns[x].spark_type), ey = elem_of(columns[y].spark_type);
        const int s = new_slot(plan, SK_VALUES);
        PlanSlot& sl = plan.slots[s];
        sl.ncols = 2;
        sl.corr = 1;
        sl.rows_per_load = elem_size(ex) == elem_size(ey) ? rows_per_load_of(ex) : 8;
        sl.col[0].column = x;
        sl.col[0].elem = ex;
        sl.col[1].column = y;
        sl.col[1].elem = ey;
        sl.where = w;
        if (x != y) {
            auto ux = uses.find({x, w}), uy = uses.find({y, w});
            if (ux != uses.end() && ux->second.slot < 0) { ux->second.slot = s; ux->second.pos = 0; }
            if (uy != uses.end() && uy->second.slot < 0) { uy->second.slot = s; uy->second.pos = 1; }
        }
        pair_slots[std::make_tuple(x, y, w)] = s;
        op_slot[i] = {s, 0};
    }
    for (auto& kv : uses) {
        if (kv.second.slot >= 0) continue;
        const int s = new_slot(plan, SK_VALUES);
        PlanSlot& sl = plan.slots[s];
        sl.ncols = 1;
        sl.col[0].column = kv.first.first;
        sl.col[0].elem = elem_of(columns[kv.first.first].spark_type);
        sl.rows_per_load = rows_per_load_of(sl.col[0].elem);
        sl.where = kv.first.second;
        kv.second.slot = s;
        kv.second.pos = 0;
    }
    for (auto& kv : uses) {
        PlanCol& pc = plan.slots[kv.second.slot].col[kv.second.pos];
        pc.flags |= kv.second.flags;
        pc.pred_op = kv.second.pred_op;
        pc.pred_kind = kv.second.pred_kind;
        pc.pred_i = kv.second.pred_i;
        pc.pred_d = kv.second.pred_d;
        if (kv.second.flags & CF_HLL) pc.hll_slot = kv.second.hll = plan.nhll++;
    }
}

// String-shaped ops -> string slots (column, where): MinLength / MaxLength, DataType, string HLL.
void plan_string_slots(ScanPlan& plan, const dq_column* columns, const dq_op* ops, int nops, const ScanUse& use,
                       std::vector<int>& op_sslot) {
    std::map<std::pair<int, int>, int> sslot_of;
    for (int i = 0; i < nops; ++i) {
        const dq_op& op = ops[i];
        if (use.wide_op[i]) continue;
        const bool str_hll = op.kind == DQ_OP_APPROX_COUNT_DISTINCT && columns[op.column[0]].spark_type == DQ_TYPE_STRING;
        if (!(op.kind == DQ_OP_MIN_LENGTH || op.kind == DQ_OP_MAX_LENGTH || op.kind == DQ_OP_DATATYPE || str_hll)) continue;
        const auto key = std::make_pair((int)op.column[0], (int)op.where);
        auto it = sslot_of.find(key);
        if (it == sslot_of.end()) {
            PlanStrSlot ss;
            ss.column = op.column[0];
            ss.where = op.where;
            plan.sslots.push_back(ss);
            it = sslot_of.emplace(key, (int)plan.sslots.size() - 1).first;
        }
        PlanStrSlot& ss = plan.sslots[it->second];
        if (op.kind == DQ_OP_DATATYPE) ss.flags |= SF_DTYPE;
        else if (str_hll) {
            ss.flags |= SF_HLL;
            if (ss.hll_slot < 0) ss.hll_slot = plan.nhll++;
        } else ss.flags |= SF_LEN;
        op_sslot[i] = it->second;
    }
    for (int i = 0; i < nops; ++i) {
        if (op_sslot[i] < 0 || ops[i].kind == DQ_OP_APPROX_COUNT_DISTINCT) continue;
        plan.sopmap.push_back(StrOpMap{i, ops[i].kind, op_sslot[i], 0});
    }
}

// DECIMAL128 ops -> decimal128 slots (column, where), one launch for all of them (decimal128.hip).
void plan_decimal128_slots(ScanPlan& plan, const dq_op* ops, int nops, const ScanUse& use, std::vector<int>& op_dslot) {
    std::map<std::pair<int, int>, int> dslot_of;
    for (int i = 0; i < nops; ++i) {
        if (!use.wide_op[i]) continue;
        const dq_op& op = ops[i];
        const auto key = std::make_pair((int)op.column[0], (int)op.where);
        auto it = dslot_of.find(key);
        if (it == dslot_of.end()) {
            PlanD128Slot ds;
            ds.column = op.column[0];
            ds.where = op.where;
            plan.dslots.push_back(ds);
            it = dslot_of.emplace(key, (int)plan.dslots.size() - 1).first;
        }
        PlanD128Slot& ds = plan.dslots[it->second];
        op_dslot[i] = it->second;
        switch (op.kind) {
            case DQ_OP_MEAN: case DQ_OP_SUM: ds.flags |= DF_SUM; break;
            case DQ_OP_MINIMUM: case DQ_OP_MAXIMUM: ds.flags |= DF_MINMAX; break;
            case DQ_OP_STANDARD_DEVIATION: ds.flags |= DF_MOMENTS; break;
            case DQ_OP_APPROX_COUNT_DISTINCT:
                ds.flags |= DF_HLL;
                if (ds.hll_slot < 0) ds.hll_slot = plan.nhll++;
                break;
            default: break;
        }
        if (op.kind != DQ_OP_APPROX_COUNT_DISTINCT)  // the HLL state is packed by finalize_kernel
            plan.dopmap.push_back(D128OpMap{i, op.kind, it->second, op.where >= 0});
    }
}

// The bits-only slot of (tag, column / predicate, where), created on first use.
struct BitsSlots {
    ScanPlan& plan;
    std::map<std::tuple<int, int, int>, int> of;
    int get(int tag, int ref, int w) {
        const auto key = std::make_tuple(tag, ref, w);
        auto it = of.find(key);
        if (it != of.end()) return it->second;
        const int s = new_slot(plan, SK_BITS);
        plan.slots[s].where = w;
        plan.slots[s].tag = tag;
        plan.slots[s].ref = ref;
        of[key] = s;
        return s;
    }
};

// Masked `where` plan of filter p: the producer (a one-column 8-byte value slot under the filter whose terms read only
// that column, else where_masks_kernel), the consumer masks, and whether bits / string / decimal128 slots still read
// the filter's bitmaps. More than kWhereMasks consumer columns: the filter goes back to the bitmap pass.
void plan_where(ScanPlan& plan, int p, const dq_column* columns, bool fused_producer) {
    WherePlan& wp = plan.where[p];
    int depth = 0, maxd = 0;
    for (int i = 0; i < wp.prog.nb; ++i) {
        depth += wp.prog.b[i] >= 0 ? 1 : (wp.prog.b[i] == kPB_NOT ? 0 : -1);
        maxd = std::max(maxd, depth);
    }
    const int nslots = (int)plan.slots.size();
    for (int s = 0; s < nslots && wp.producer < 0 && maxd <= kWhereStack && fused_producer; ++s) {
        const PlanSlot& sl = plan.slots[s];
        if (sl.kind != SK_VALUES || sl.ncols != 1 || sl.where != p) continue;
        const int x = sl.col[0].column;
        const int t = columns[x].spark_type;
        if (!(t == DQ_TYPE_LONG || t == DQ_TYPE_TIMESTAMP || t == DQ_TYPE_DOUBLE)) continue;
        bool own = true;
        for (int k = 0; k < wp.prog.nterms; ++k) own &= wp.prog.t[k].col == x;
        if (own) wp.producer = s;
    }
    for (int s = 0; s < nslots; ++s) {
        PlanSlot& sl = plan.slots[s];
        if (sl.kind == SK_BITS && (sl.where == p || (sl.tag == BT_COMPLIANCE && sl.ref == p))) wp.bitmaps = true;
        if (sl.kind != SK_VALUES || sl.where != p || s == wp.producer) continue;
        for (int k = 0; k < sl.ncols; ++k) {
            auto it = std::find(wp.mask_col.begin(), wp.mask_col.end(), sl.col[k].column);
            sl.col[k].mask_pred = p;
            sl.col[k].mask_index = (int)(it - wp.mask_col.begin());
            if (it == wp.mask_col.end()) wp.mask_col.push_back(sl.col[k].column);
        }
    }
    for (const PlanStrSlot& ss : plan.sslots) wp.bitmaps |= ss.where == p;
    for (const PlanD128Slot& ds : plan.dslots) wp.bitmaps |= ds.where == p;
    if ((int)wp.mask_col.size() > kWhereMasks) {
        wp = WherePlan();
        for (PlanSlot& sl : plan.slots)
            for (PlanCol& c : sl.col)
                if (c.mask_pred == p) c.mask_pred = c.mask_index = -1;
    }
}

// Launch groups: one kernel launch per slot shape, fused `where` producers first (the other launches read their masks).
void plan_groups(ScanPlan& plan) {
    // heavy 2 (8-byte columns only): every column carries stats, moments, HLL and a fused compare the heavy kernel
    // evaluates on its fast path, pairs carry the correlation, and there is no `where` -> the branch-free variant
    auto full_col = [](const PlanCol& c) {
        const bool fl = c.elem == ET_F64;
        const uint32_t all = CF_STATS | CF_MOMENTS | CF_HLL;
        const bool fast_pred = fl ? (c.pred_kind != FP_NONE && (c.pred_kind == FP_LONG || c.pred_d == c.pred_d))
                                  : c.pred_kind == FP_LONG;
        return (c.flags & all) == all && fast_pred;
    };
    std::map<int, int> group_of;
    for (int s = 0; s < (int)plan.slots.size(); ++s) {
        const PlanSlot& sl = plan.slots[s];
        if (sl.kind == SK_WHERE) continue;
        const bool values = sl.kind == SK_VALUES;
        const bool f0 = values && (sl.col[0].elem == ET_F32 || sl.col[0].elem == ET_F64);
        const bool f1 = values && sl.ncols > 1 && (sl.col[1].elem == ET_F32 || sl.col[1].elem == ET_F64);
        const int P = values ? sl.rows_per_load : 8;
        const int nc = values ? sl.ncols : 1;
        // HLL registers or a fused predicate need the larger (HEAVY) kernel instantiation.
        int heavy = 0;
        for (int k = 0; values && k < sl.ncols; ++k)
            if ((sl.col[k].flags & CF_HLL) || sl.col[k].pred_kind != FP_NONE) heavy = 1;
        if (heavy && P == 2 && sl.where < 0 && (sl.ncols == 1 || sl.corr)) {
            bool full = true;
            for (int k = 0; k < sl.ncols; ++k) full &= full_col(sl.col[k]);
            if (full) heavy = 2;
        }
        if (sl.producer_of >= 0) heavy = 3;
        const int key = (((((sl.kind * 16 + P) * 4 + nc) * 2 + f0) * 2 + f1) * 4 + heavy);
        auto it = group_of.find(key);
        if (it == group_of.end()) {
            plan.groups.push_back(PlanGroup{sl.kind, P, nc, f0, f1, heavy, key, {}});
            it = group_of.emplace(key, (int)plan.groups.size() - 1).first;
        }
        plan.groups[it->second].slots.push_back(s);
    }
    std::stable_sort(plan.groups.begin(), plan.groups.end(),
                     [](const PlanGroup& a, const PlanGroup& b) { return (a.heavy == 3) > (b.heavy == 3); });
}

}  // namespace

int plan_scan(const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops, const dq_predicate* preds,
              int npreds, const ScanUse& use, const ScanOptions& options, ScanPlan* out, std::string* msg) {
    ScanPlan& plan = *out;
    plan = ScanPlan();
    plan.slots.reserve((size_t)nops + npreds);
    auto col_ok = [&](int c) { return c >= 0 && c < ncols; };
    UseMap uses;
    std::vector<int> fused_col(nops, -1);  // Compliance ops answered inside a value slot
    for (int i = 0; i < nops; ++i) {
        const dq_op& op = ops[i];
        if (use.wide_op[i]) continue;
        const auto key = std::make_pair((int)op.column[0], (int)op.where);
        switch (op.kind) {
            case DQ_OP_MEAN: case DQ_OP_SUM: case DQ_OP_MINIMUM: case DQ_OP_MAXIMUM: uses[key].flags |= CF_STATS; break;
            case DQ_OP_STANDARD_DEVIATION: uses[key].flags |= CF_MOMENTS; break;
            case DQ_OP_APPROX_COUNT_DISTINCT:
                if (columns[op.column[0]].spark_type != DQ_TYPE_STRING) uses[key].flags |= CF_HLL;
                break;
            case DQ_OP_COMPLIANCE: fused_col[i] = fuse_compliance(preds[op.predicate], columns, op.where, uses); break;
            default: break;
        }
    }
    std::vector<std::pair<int, int>> op_slot(nops, {-1, 0});
    std::vector<int> op_sslot(nops, -1), op_dslot(nops, -1);
    plan_value_slots(plan, columns, ops, nops, uses, op_slot);
    plan_string_slots(plan, columns, ops, nops, use, op_sslot);
    plan_decimal128_slots(plan, ops, nops, use, op_dslot);

    // `where` filters evaluated inside the scan (WhereOut, dq_internal.h): every simple predicate used as a `where`
    plan.where.assign(npreds, WherePlan());
    const bool masks_on = options.where_masks && !options.pred_vm;
    for (int i = 0; i < nops && masks_on; ++i) {
        const int p = ops[i].where;
        if (p < 0 || plan.where[p].masked || is_regex_program(preds[p])) continue;
        plan.where[p].masked = compile_simple_predicate(preds[p], columns, ncols, plan.where[p].prog);
    }

    // Ops -> OpMap; bits-only slots for Size(where), Completeness of unread columns, Compliance.
    plan.opmap.resize(nops);
    BitsSlots bits{plan, {}};
    for (int i = 0; i < nops; ++i) {
        const dq_op& op = ops[i];
        OpMap& m = plan.opmap[i];
        memset(&m, 0, sizeof(m));
        m.kind = op.kind;
        m.slot = -1;
        m.hll_slot = -1;
        m.has_where = op.where >= 0;
        m.nrows = nrows;
        const int c = op.column[0];
        if (op.kind != DQ_OP_SIZE && op.kind != DQ_OP_COMPLIANCE && col_ok(c)) {
            const int t = columns[c].spark_type;
            m.is_float = (t == DQ_TYPE_FLOAT || t == DQ_TYPE_DOUBLE);
            m.decimal_scale = t == DQ_TYPE_DECIMAL ? columns[c].decimal_scale : 0;
        }
        m.wslot = -1;
        if (use.wide_op[i]) {  // written by finalize_decimal128_kernel; the HLL words by finalize_kernel
            if (op.kind == DQ_OP_APPROX_COUNT_DISTINCT) m.hll_slot = plan.dslots[op_dslot[i]].hll_slot;
            continue;
        }
        const bool masked_where = op.where >= 0 && plan.where[op.where].masked;
        switch (op.kind) {
            case DQ_OP_SIZE:
                if (op.where >= 0 && !masked_where) m.slot = bits.get(BT_SIZE, -1, op.where);
                break;
            case DQ_OP_COMPLIANCE:
                if (fused_col[i] >= 0) {
                    const Use& u = uses.at({fused_col[i], op.where});
                    m.slot = u.slot;
                    m.colpos = u.pos;
                    m.from_bits = 3;  // fused predicate: matches = c.pt, non-null rows = c.n
                } else {
                    m.slot = bits.get(BT_COMPLIANCE, op.predicate, op.where);
                }
                break;
            case DQ_OP_COMPLETENESS: {
                auto it = uses.find({c, op.where});
                if (it != uses.end()) {
                    m.slot = it->second.slot;
                    m.colpos = it->second.pos;
                } else if (columns[c].validity == nullptr) {
                    m.from_bits = 2;  // all rows valid: matches = conditionalCount
                    if (op.where >= 0 && !masked_where) m.slot = bits.get(BT_SIZE, -1, op.where);
                } else {
                    m.slot = bits.get(BT_COMPLETENESS, c, op.where);
                    m.from_bits = 1;
                }
                break;
            }
            case DQ_OP_CORRELATION:
                m.slot = op_slot[i].first;
                m.colpos = op_slot[i].second;
                break;
            case DQ_OP_MIN_LENGTH: case DQ_OP_MAX_LENGTH: case DQ_OP_DATATYPE:
                break;  // written by finalize_strings_kernel
            default: {
                if (op_sslot[i] >= 0) {  // ApproxCountDistinct of a string column
                    m.hll_slot = plan.sslots[op_sslot[i]].hll_slot;
                    break;
                }
                const Use& u = uses.at({c, op.where});
                m.slot = u.slot;
                m.colpos = u.pos;
                m.hll_slot = u.hll;
                break;
            }
        }
    }
    for (int p = 0; p < npreds; ++p)
        if (plan.where[p].masked) plan_where(plan, p, columns, options.fused_producer);
    // Size(where) / from_bits == 2 Completeness were planned without a bits slot for masked filters: give back the
    // bits slots to filters that fell back to the bitmap pass.
    for (int i = 0; i < nops; ++i) {
        const dq_op& op = ops[i];
        if (op.where < 0 || plan.where[op.where].masked || plan.opmap[i].slot >= 0) continue;
        if (op.kind == DQ_OP_SIZE || (op.kind == DQ_OP_COMPLETENESS && plan.opmap[i].from_bits == 2))
            plan.opmap[i].slot = bits.get(BT_SIZE, -1, op.where);
    }
    // The masked filters' count slots; their value slots read masks (or produce them), no bitmaps.
    for (int p = 0; p < npreds; ++p) {
        WherePlan& wp = plan.where[p];
        if (!wp.masked) continue;
        if (wp.producer >= 0) {
            wp.wslot = wp.producer;
            plan.slots[wp.producer].producer_of = p;
        } else {
            wp.wslot = new_slot(plan, SK_WHERE);
            ++plan.nstandalone;
        }
        for (PlanSlot& sl : plan.slots)
            if (sl.kind == SK_VALUES && sl.where == p) sl.where = -1;
    }
    for (int i = 0; i < nops; ++i) {
        const int p = ops[i].where;
        if (p >= 0) plan.opmap[i].wslot = plan.where[p].masked ? plan.where[p].wslot : plan.opmap[i].slot;
    }
    const int nslots = (int)plan.slots.size();
    if (nslots > kMaxSlots) return failf(msg, DQ_ERR_UNSUPPORTED, "too many slots (%d)", nslots);
    // Predicates that get bitmaps: `where` filters and Compliance predicates not fused into a value scan; a masked
    // filter only when something reads its bitmaps, and then its producer writes them, not a predicate pass.
    plan.pred_used.assign(npreds, 0);
    for (int i = 0; i < nops; ++i) {
        if (ops[i].where >= 0) plan.pred_used[ops[i].where] = 1;
        if (ops[i].kind == DQ_OP_COMPLIANCE && fused_col[i] < 0) plan.pred_used[ops[i].predicate] = 1;
    }
    plan.pred_pass = plan.pred_used;
    for (int p = 0; p < npreds; ++p) {
        if (!plan.where[p].masked) continue;
        plan.pred_pass[p] = 0;
        if (!plan.where[p].bitmaps) plan.pred_used[p] = 0;
    }
    for (size_t p = 0; p < options.pred_inline.size(); ++p)
        if (options.pred_inline[p]) plan.pred_used[p] = plan.pred_pass[p] = 0;
    plan_groups(plan);
    return DQ_OK;
}

ScanGeometry plan_geometry(const ScanPlan& plan, int cus, int64_t ntiles, int64_t grid_cap, bool concurrent, int sgrid,
                           int dgrid, const int* occ) {
    ScanGeometry g;
    g.ntiles = ntiles;
    // concurrent launches: each shape gets its share of the chip so the launches are co-resident
    const int nlaunch = plan.nlaunch();
    auto share = [&](int grid) { return concurrent ? std::max(1, (grid + nlaunch - 1) / nlaunch) : grid; };
    g.grid.resize(plan.groups.size());
    for (size_t i = 0; i < plan.groups.size(); ++i) {  // a grid that fills the chip once
        const int64_t planned = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(ntiles, 1), (int64_t)cus * occ[i]));
        g.grid[i] = share((int)std::min(planned, grid_cap));
        g.gstride = std::max(g.gstride, g.grid[i]);
    }
    g.sgrid = sgrid ? share(sgrid) : 0;
    g.dgrid = dgrid;  // runs on the ctx stream after the other launches joined: the whole chip
    g.gstride = std::max(g.gstride, std::max(g.sgrid, g.dgrid));
    g.slot_nblocks.assign(std::max<size_t>(plan.slots.size(), 1), 1);
    for (size_t i = 0; i < plan.groups.size(); ++i)
        for (int32_t s : plan.groups[i].slots) g.slot_nblocks[s] = g.grid[i];
    const int64_t wchunks = (std::max<int64_t>(ntiles, 1) * (kTileRows / 64) + 7) / 8;  // where_masks_kernel: 8 words per wave, 4 waves
    g.wgrid = (int)std::max<int64_t>(1, std::min<int64_t>((wchunks + 3) / 4, g.gstride));
    for (const WherePlan& wp : plan.where)
        if (wp.masked && wp.producer < 0) g.slot_nblocks[wp.wslot] = g.wgrid;
    g.hll_nblocks.assign(std::max(plan.nhll, 1), 1);
    for (size_t s = 0; s < plan.slots.size(); ++s)
        for (const PlanCol& c : plan.slots[s].col)
            if (c.hll_slot >= 0) g.hll_nblocks[c.hll_slot] = g.slot_nblocks[s];
    for (const PlanStrSlot& ss : plan.sslots)
        if (ss.hll_slot >= 0) g.hll_nblocks[ss.hll_slot] = g.sgrid;
    for (const PlanD128Slot& ds : plan.dslots)
        if (ds.hll_slot >= 0) g.hll_nblocks[ds.hll_slot] = g.dgrid;
    return g;
}

ScanLayout layout_scan(const ScanPlan& plan, const ScanGeometry& geo, const ScanUse& use, const dq_column* columns, int ncols,
                       int64_t nrows, int nops, const dq_predicate* preds, int npreds, bool out_device) {
    ScanLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) {  // device only
        off = align_up(off, 256);
        const size_t at = off;
        off += bytes;
        return at;
    };
    auto staged = [&](size_t bytes) {  // uploaded through (or read back into) pinned staging, 16-byte aligned there
        L.pinned_bytes += align_up(bytes, 16);
        return take(bytes);
    };
    const size_t bitmap_bytes = (size_t)(nrows + 7) / 8;
    const size_t pbytes = (size_t)padded_words_for(nrows) * 8;
    const size_t nslots = std::max<size_t>(plan.slots.size(), 1), nsslots = std::max<size_t>(plan.sslots.size(), 1),
                 ndslots = std::max<size_t>(plan.dslots.size(), 1), gstride = (size_t)geo.gstride;
    L.col.resize(ncols);
    for (int c = 0; c < ncols; ++c) {
        const dq_column& col = columns[c];
        if (!use.col_used[c] || (col.flags & DQ_COL_DEVICE)) continue;
        ScanLayout::Column& lc = L.col[c];
        if (col.spark_type == DQ_TYPE_STRING) lc.vbytes = nrows > 0 ? (size_t)col.offsets[nrows] : 0;
        else if (col.spark_type == DQ_TYPE_DECIMAL128) lc.vbytes = (size_t)nrows * 16;
        else lc.vbytes = (size_t)nrows * elem_size(elem_of(col.spark_type));
        lc.values = take(lc.vbytes + 16);
        if (col.validity) lc.validity = take(align_up(bitmap_bytes, 8) + 8);
        if (col.spark_type == DQ_TYPE_STRING) lc.offsets = take(((size_t)nrows + 1) * 4);
    }
    L.pred.resize(npreds);
    L.mask_stride = pbytes;  // whole tiles: a multiple of the 256-byte alignment, so the masks are contiguous
    for (int p = 0; p < npreds; ++p) {
        if (!plan.pred_used[p]) continue;
        L.pred[p].t = take(pbytes);
        L.pred[p].nn = take(pbytes);
    }
    for (int p = 0; p < npreds; ++p) {
        if (!plan.where[p].masked) continue;
        L.pred[p].wout = staged(sizeof(WhereOut));
        for (size_t m = 0; m < plan.where[p].mask_col.size(); ++m) {
            const size_t at = take(pbytes);
            if (m == 0) L.pred[p].mask0 = at;
        }
    }
    L.pcols = staged(sizeof(PredColumn) * std::max(ncols, 1));
    L.status = staged(sizeof(int32_t) * std::max(npreds, 1));
    for (int p = 0; p < npreds; ++p) {
        if (!plan.pred_pass[p]) continue;
        L.pred[p].prog = staged(sizeof(PredProgram));
        L.pred[p].code = staged(sizeof(int32_t) * preds[p].code_len);
        L.pred[p].consts = staged(sizeof(dq_const) * std::max(preds[p].n_consts, 1));
        L.pred[p].strings = staged(std::max<int64_t>(preds[p].strings_len, 1));
    }
    L.slots = staged(sizeof(SlotDesc) * nslots);
    L.ops = staged(sizeof(OpMap) * nops);
    L.partials = take(sizeof(SlotPartial) * nslots * gstride);
    L.order = staged(sizeof(int32_t) * nslots);
    L.slot_nblocks = staged(sizeof(int32_t) * geo.slot_nblocks.size());
    L.hll_nblocks = staged(sizeof(int32_t) * geo.hll_nblocks.size());
    L.finals = take(sizeof(SlotPartial) * nslots);
    L.hll_partials = take((size_t)std::max(plan.nhll, 1) * gstride * kHllRegs);
    L.hll_final = take((size_t)std::max(plan.nhll, 1) * kHllRegs);
    if (!out_device) L.out = staged(sizeof(dq_state) * nops);
    L.sslots = staged(sizeof(StrSlot) * nsslots);
    L.spartials = take(sizeof(StrPartial) * nsslots * gstride);
    L.sops = staged(sizeof(StrOpMap) * std::max<size_t>(plan.sopmap.size(), 1));
    L.dslots = staged(sizeof(D128Slot) * ndslots);
    L.dpartials = take(sizeof(D128Partial) * ndslots * gstride);
    L.dops = staged(sizeof(D128OpMap) * std::max<size_t>(plan.dopmap.size(), 1));
    L.arena_bytes = off;
    return L;
}

}  // namespace dq
