// call_plans.cpp — the host plans of dq_row_outcomes and dq_dict_scan as pure host functions (call_plans.h). Also built
// with -DDQ_HOST_ONLY under ASan / UBSan by tests/sanitize_scan_plan.
#include "call_plans.h"

#include <algorithm>
#include <map>
#include <utility>

namespace dq {

// ---- dq_row_outcomes ---------------------------------------------------------------------------------------------------
int validity_source(const dq_column& col, bool read_by_predicate) {
    if (col.flags & DQ_COL_DEVICE) return col.validity ? RP_VALID_DEVICE : RP_ONES;
    if (!col.validity) return RP_ONES;
    return read_by_predicate ? RP_VALID_SCAN : RP_VALID_CALL;
}

std::vector<dq_op> size_where_ops(int npreds) {
    std::vector<dq_op> ops((size_t)std::max(npreds, 0));
    for (int p = 0; p < npreds; ++p) ops[p] = dq_op{DQ_OP_SIZE, {-1, -1}, p, -1};
    return ops;
}

int plan_row_outcomes(const dq_column* columns, int ncols, int64_t nrows, const dq_predicate* preds, int npreds,
                      const dq_row_term* terms, int nterms, const dq_row_check* checks, int nchecks, uint32_t flags, bool pred_vm,
                      RowPlan* out, std::string* msg) {
    RowPlan& plan = *out;
    plan = RowPlan();
    if (nterms > DQ_ROW_MAX_TERMS || nchecks > DQ_ROW_MAX_CHECKS)
        return failf(msg, DQ_ERR_UNSUPPORTED, "dq_row_outcomes: %d terms over %d checks, at most %d terms and %d checks per call",
                     nterms, nchecks, DQ_ROW_MAX_TERMS, DQ_ROW_MAX_CHECKS);
    plan.null_mode = (flags & DQ_ROW_FILTERED_NULL) != 0;
    for (int t = 0; t < nterms; ++t) {
        const dq_row_term& tm = terms[t];
        if (tm.check < 0 || tm.check >= nchecks)
            return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term %d names check %d", t, tm.check);
        if (tm.kind == DQ_ROW_BITS) {
            if (!tm.pass_bits || !tm.considered_bits)
                return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term %d has no bitmaps", t);
            if (((uintptr_t)tm.pass_bits | (uintptr_t)tm.considered_bits) & 7)
                return failf(msg, DQ_ERR_ALIGNMENT, "dq_row_outcomes: bitmaps must be 8-B aligned (term %d)", t);
            continue;
        }
        if (tm.where < -1 || tm.where >= npreds)
            return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term %d names predicate %d as its where", t, tm.where);
        if (tm.kind == DQ_ROW_PREDICATE) {
            if (tm.index < 0 || tm.index >= npreds)
                return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term %d names predicate %d", t, tm.index);
        } else if (tm.kind == DQ_ROW_NOT_NULL) {
            if (tm.index < 0 || tm.index >= ncols)
                return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term %d names column %d", t, tm.index);
            const dq_column& col = columns[tm.index];
            if (col.length != nrows)
                return failf(msg, DQ_ERR_INVALID_ARGUMENT, "column %d has %lld rows, batch has %lld", tm.index, (long long)col.length,
                             (long long)nrows);
            if ((col.flags & DQ_COL_DEVICE) && ((uintptr_t)col.validity & 7))
                return failf(msg, DQ_ERR_ALIGNMENT, "dq_row_outcomes: bitmaps must be 8-B aligned (column %d)", tm.index);
        } else {
            return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: term %d has kind %d", t, tm.kind);
        }
    }
    for (int c = 0; c < nchecks; ++c) {
        const dq_row_check& ck = checks[c];
        if (!ck.pass_bits || !ck.values || (plan.null_mode && !ck.validity))
            return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: check %d lacks an output buffer", c);
        if (((uintptr_t)ck.pass_bits & 7) || ((uintptr_t)ck.values & 15) || (plan.null_mode && ((uintptr_t)ck.validity & 7)))
            return failf(msg, DQ_ERR_ALIGNMENT, "dq_row_outcomes: check %d: bitmaps must be 8-B, the byte column 16-B aligned", c);
    }
    // the predicates as dq_scan validates them; without predicates the columns are not a scan's: only NOT_NULL ones are read
    if (npreds > 0) {
        const std::vector<dq_op> ops = size_where_ops(npreds);
        const int rc = validate_scan(columns, ncols, nrows, ops.data(), npreds, preds, npreds, &plan.use, msg);
        if (rc) return rc;
    } else {
        plan.use.col_used.assign((size_t)std::max(ncols, 1), 0);
    }
    // `column <op> constant` predicates are evaluated by the row_outcomes launch itself: no pass, no bitmaps
    plan.options.where_masks = false;  // the bitmap pass: TRUE / NOT-NULL bitmaps from a predicate launch
    plan.options.pred_vm = pred_vm;
    plan.options.pred_inline.assign((size_t)npreds, 0);
    plan.inline_of.assign((size_t)std::max(npreds, 1), -1);
    for (int p = 0; p < npreds && (int)plan.inl.size() < kRowInline && !pred_vm; ++p) {
        PredSimple ps;
        if (!compile_simple_predicate(preds[p], columns, ncols, ps) || ps.nterms != 1 || ps.nb != 1 || ps.b[0] != 0 ||
            ps.t[0].op < DQ_P_EQ || ps.t[0].op > DQ_P_GE)
            continue;
        plan.inline_of[p] = (int)plan.inl.size();
        plan.inl.push_back(ps.t[0]);
        plan.options.pred_inline[p] = 1;
    }
    // terms sorted by check
    std::vector<int> order((size_t)nterms);
    for (int t = 0; t < nterms; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return terms[a].check < terms[b].check; });
    plan.term_begin.resize(nchecks);
    plan.term_end.resize(nchecks);
    for (int i = 0, c = 0; c < nchecks; ++c) {
        plan.term_begin[c] = i;
        while (i < nterms && terms[order[i]].check == c) ++i;
        plan.term_end[c] = i;
    }
    plan.term.resize(nterms);
    for (int i = 0; i < nterms; ++i) {
        const dq_row_term& tm = terms[order[i]];
        RowPlanTerm& pt = plan.term[i];
        pt.term = order[i];
        if (tm.kind == DQ_ROW_BITS) {
            pt.src = RP_BITS;
            continue;
        }
        if (tm.where >= 0 && plan.inline_of[tm.where] >= 0) pt.w_inline = plan.inline_of[tm.where];
        else pt.where = tm.where;
        if (tm.kind == DQ_ROW_PREDICATE) {
            const int k = plan.inline_of[tm.index];
            pt.src = k >= 0 ? RP_INLINE : RP_PRED;
            pt.index = k >= 0 ? k : tm.index;
        } else {
            pt.src = validity_source(columns[tm.index], plan.use.col_used[tm.index] != 0);
            pt.index = tm.index;
        }
    }
    return DQ_OK;
}

// ---- dq_dict_scan / dq_dict_counts -------------------------------------------------------------------------------------
int dict_lds_copies(const DictOptions& options, int n_dict, int64_t nrows, int grid) {
    const int entries = std::max(0, std::min(options.lds_entries, kDictLdsWords));
    if (n_dict <= 0 || n_dict > entries) return 0;
    if (nrows / grid + 2 * kDictTileRows >= ((int64_t)1 << 31)) return 0;
    int c = kDictLdsCopies;
    if (options.lds_copies == 1 || options.lds_copies == 2 || options.lds_copies == 4) c = options.lds_copies;
    while (c > 1 && (int64_t)c * n_dict > kDictLdsCopyWords) c >>= 1;
    return c;
}

int check_dict_column(const dq_dict_column& d, int64_t nrows, int which, std::string* msg) {
    const dq_column& e = d.dictionary;
    if (!(d.flags & DQ_COL_DEVICE) || !(e.flags & DQ_COL_DEVICE) || (e.flags & DQ_COL_OFFSETS64))
        return failf(msg, DQ_ERR_UNSUPPORTED, "dictionary column %d: device buffers with int32 offsets only", which);
    if (d.length != nrows || nrows < 0 || (nrows > 0 && !d.indices))
        return failf(msg, DQ_ERR_INVALID_ARGUMENT, "dictionary column %d has %lld rows, batch has %lld", which, (long long)d.length,
                     (long long)nrows);
    if (e.spark_type != DQ_TYPE_STRING || e.length < 1 || e.length > INT32_MAX - 1 || !e.offsets || !e.validity || !e.values)
        return failf(msg, DQ_ERR_INVALID_ARGUMENT,
                     "dictionary column %d: the dictionary is a STRING column of n_dict + 1 entries (the last one NULL) "
                     "with offsets, a validity bitmap and bytes", which);
    if (((uintptr_t)d.indices & 3) || ((uintptr_t)d.validity & 7) || ((uintptr_t)e.values & 3) || ((uintptr_t)e.offsets & 3) ||
        ((uintptr_t)e.validity & 7))
        return failf(msg, DQ_ERR_ALIGNMENT, "dictionary column %d: misaligned buffer", which);
    return DQ_OK;
}

dq_predicate dict_pop_predicate(const DictPlan& plan, int q, const dq_predicate* preds) {
    dq_predicate pr = preds[plan.pops[q].pred];
    pr.code = pr.code ? plan.pops[q].code.data() : nullptr;
    return pr;
}

int plan_dict_scan(const dq_column* columns, int ncols, const dq_dict_column* dicts, int ndicts, int64_t nrows, const dq_op* ops,
                   int nops, const dq_predicate* preds, int npreds, const DictOptions& options, int grid, DictPlan* out,
                   std::string* msg) {
    DictPlan& plan = *out;
    plan = DictPlan();
    for (int d = 0; d < ndicts; ++d) {
        const int rc = check_dict_column(dicts[d], nrows, d, msg);
        if (rc) return rc;
    }
    // one slot per (dictionary column, where); one predicate op per Compliance
    std::map<std::pair<int, int>, int> slot_of;
    plan.opmap.resize(nops);
    plan.op_pop.assign(nops, -1);
    plan.where_used.assign((size_t)std::max(npreds, 1), 0);
    for (int i = 0; i < nops; ++i) {
        const dq_op& op = ops[i];
        const int d = op.column[0] - ncols;
        if (d < 0 || d >= ndicts) return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: column %d names no dictionary column", i, op.column[0]);
        if (op.where < -1 || op.where >= npreds) return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: bad where index", i);
        uint32_t flag = 0;
        switch (op.kind) {
            case DQ_OP_COMPLETENESS: break;
            case DQ_OP_MIN_LENGTH: case DQ_OP_MAX_LENGTH: flag = SF_LEN; break;
            case DQ_OP_DATATYPE: flag = SF_DTYPE; break;
            case DQ_OP_APPROX_COUNT_DISTINCT: flag = SF_HLL; break;
            case DQ_OP_COMPLIANCE:
                if (op.predicate < 0 || op.predicate >= npreds)
                    return failf(msg, DQ_ERR_INVALID_ARGUMENT, "op %d: Compliance needs a predicate", i);
                break;
            default:
                return failf(msg, DQ_ERR_UNSUPPORTED, "op %d: kind %d is not answered from a dictionary column", i, op.kind);
        }
        if (op.where >= 0) {
            plan.where_used[op.where] = 1;
            const dq_predicate& w = preds[op.where];
            for (int k = 0; k + 1 < w.code_len; k += 2)
                if (w.code[k] == DQ_P_COL && (w.code[k + 1] < 0 || w.code[k + 1] >= ncols))
                    return failf(msg, DQ_ERR_UNSUPPORTED, "op %d: its where reads a dictionary column", i);
        }
        const auto key = std::make_pair(d, (int)op.where);
        auto it = slot_of.find(key);
        if (it == slot_of.end()) {
            DictPlanSlot s;
            s.dict = d;
            s.where = op.where;
            s.n_dict = (int)(dicts[d].dictionary.length - 1);
            it = slot_of.emplace(key, (int)plan.slots.size()).first;
            plan.slots.push_back(s);
        }
        plan.slots[it->second].flags |= flag;
        plan.opmap[i] = DictOpMap{i, op.kind, it->second, op.where >= 0, nullptr};
        if (op.kind == DQ_OP_COMPLIANCE) {
            plan.op_pop[i] = (int)plan.pops.size();
            plan.pops.push_back(DictPlanPred{op.predicate, it->second, {}});
        }
    }
    const int nslots = (int)plan.slots.size(), npops = (int)plan.pops.size();
    if (nslots > kMaxSlots) return failf(msg, DQ_ERR_UNSUPPORTED, "dq_dict_scan: more than %d slots", kMaxSlots);
    for (int c = 0; c < ncols; ++c) {  // the plain columns a where reads
        bool used = false;
        for (int p = 0; p < npreds && !used; ++p)
            for (int k = 0; plan.where_used[p] && k + 1 < preds[p].code_len; k += 2)
                used |= preds[p].code[k] == DQ_P_COL && preds[p].code[k + 1] == c;
        if (!used) continue;
        if (!(columns[c].flags & DQ_COL_DEVICE) || (columns[c].flags & DQ_COL_OFFSETS64) || columns[c].length != nrows ||
            columns[c].spark_type == DQ_TYPE_DECIMAL128)
            return failf(msg, DQ_ERR_UNSUPPORTED, "dq_dict_scan: column %d of a where must be a device column of the batch's rows", c);
    }
    // every program as dq_scan validates it: the filters over the plain columns, each Compliance predicate rewritten
    // to read column 0 = its slot's dictionary
    std::string why;
    for (int p = 0; p < npreds; ++p) {
        if (!plan.where_used[p]) continue;
        const int rc = validate_predicate(preds[p], columns, ncols, &why);
        if (rc) return failf(msg, rc, "dq_dict_scan: predicate %d: %s", p, why.c_str());
    }
    for (int q = 0; q < npops; ++q) {
        DictPlanPred& pop = plan.pops[q];
        const dq_predicate& src = preds[pop.pred];
        if (src.code && src.code_len > 0) pop.code.assign(src.code, src.code + src.code_len);
        for (size_t k = 0; k + 1 < pop.code.size(); k += 2)
            if (pop.code[k] == DQ_P_COL) pop.code[k + 1] = 0;
        const int rc = validate_predicate(dict_pop_predicate(plan, q, preds), &dicts[plan.slots[pop.slot].dict].dictionary, 1, &why);
        if (rc) return failf(msg, rc, "dq_dict_scan: predicate %d: %s", pop.pred, why.c_str());
    }
    // the zero block, the LDS counters, and the staging of every upload and read-back the call makes
    for (DictPlanSlot& s : plan.slots) {
        s.stats = plan.zwords;
        s.fold = s.stats + DS_COUNT;
        s.counts = s.fold + DF_COUNT;
        s.hll = s.counts + (size_t)s.n_dict;
        plan.zwords = s.hll + kHllRegs / 2;
        s.lds_copies = dict_lds_copies(options, s.n_dict, nrows, grid);
        plan.max_entries = std::max(plan.max_entries, s.n_dict);
        plan.lds_words = std::max(plan.lds_words, s.lds_copies * s.n_dict);
    }
    plan.sums_off = plan.zwords;
    plan.zwords += 2 * (size_t)std::max(npops, 1);
    plan.nstatus = std::max(npreds, 1) + std::max(npops, 1);
    auto staged = [&](size_t bytes) { plan.pinned_bytes += align_up(bytes, 16); };
    staged(sizeof(PredColumn) * (size_t)(std::max(ncols, 1) + std::max(npops, 1)));
    for (int p = 0; p < npreds; ++p)
        if (plan.where_used[p]) plan.pinned_bytes += pred_stage_bytes(preds[p]);
    staged(sizeof(DictSlot) * nslots);
    for (int q = 0; q < npops; ++q) plan.pinned_bytes += pred_stage_bytes(preds[plan.pops[q].pred]);
    staged(sizeof(DictPredOp) * npops);
    staged(sizeof(DictOpMap) * nops);
    staged(sizeof(dq_state) * nops);                 // the states' read-back
    staged(sizeof(int32_t) * plan.nstatus);          // the status words'
    staged(sizeof(int64_t) * DS_COUNT * nslots);     // every slot's row statistics'
    return DQ_OK;
}

}  // namespace dq
