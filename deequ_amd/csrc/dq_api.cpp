// dq_api.cpp — host runtime behind include/dq.h.
//
// Plans a batch of deequ ops into fused-scan slots (one HBM read per column), evaluates `where`
// / Compliance predicates into bitmaps, launches the kernels on the context's stream and turns
// the final slot partials into per-op states. Mirrors, per entry point:
//   dq_scan            runScanningAnalyzers            R/AnalysisRunner.scala:289-336
//   dq_state_merge     State.sum / Analyzers.merge     A/Analyzer.scala:367-386 (+ each state's sum)
//   dq_hll_count       DeequHyperLogLogPlusPlusUtils   C/StatefulHyperloglogPlus.scala:210-298
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "call_plans.h"
#include "dq_common.h"
#include "dq_dict.h"
#include "dq_internal.h"
#include "rx_engine.h"
#include "scan_plan.h"

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

namespace {
// DQ_SEGV_TRACE=1: a host-side fault of the library prints its native backtrace (addresses into libdq.so, resolved
// with addr2line against the same build) before the process dies -- the host code's equivalent of a GPU printf.
void dq_segv_trace(int sig) {
    void* frames[64];
    const int n = backtrace(frames, 64);
    const char msg[] = "[dq] fatal signal, native backtrace:\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
struct DqSegvTrace {
    DqSegvTrace() {
        if (getenv("DQ_SEGV_TRACE")) signal(SIGSEGV, dq_segv_trace);
    }
} dq_segv_trace_init;
}  // namespace

using namespace dq;

namespace {

int fail(dq_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define DQ_HIP(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((ctx), DQ_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

// DQ_PRED_VM=1: every predicate on the general VM (A/B and cross-checks of the simple-predicate kernel).
bool pred_vm_forced() {
    const char* e = getenv("DQ_PRED_VM");
    return e && e[0] == '1';
}

// DQ_SCAN_CONCURRENT=1: the scan's launch shapes run concurrently on side streams (read per call).
bool scan_concurrency() {
    const char* e = getenv("DQ_SCAN_CONCURRENT");
    return e && e[0] == '1';
}

// DQ_SCAN_GRID=g (g >= 1): caps every scan group's grid at g workgroups, never raises it (read per call; tests/).
int64_t scan_grid_cap() {
    const char* e = getenv("DQ_SCAN_GRID");
    const long v = e ? atol(e) : 0;
    return v >= 1 ? (int64_t)v : INT64_MAX;
}

// Which kernel a launch group runs (mirrors values_kernel_for in scan.hip).
int scan_kernel_family(int kind, int P, int nc, int heavy) {
    if (kind == SK_BITS) return DQ_KERNEL_BITS;
    if (heavy == 3) return DQ_KERNEL_WHERE_FUSED;
    if ((heavy || nc == 2) && P == 2) return heavy == 2 ? DQ_KERNEL_HEAVY8_FULL : DQ_KERNEL_HEAVY8;
    return heavy ? DQ_KERNEL_STRIPED_HEAVY : DQ_KERNEL_STRIPED;
}

int ensure_side_streams(dq_ctx* ctx) {
    if (ctx->fork_ev) return DQ_OK;
    for (int i = 0; i < dq_ctx::kSide; ++i) {
        DQ_HIP(ctx, hipStreamCreateWithPriority(&ctx->side[i], hipStreamNonBlocking, ctx->hip_priority));
        DQ_HIP(ctx, hipEventCreateWithFlags(&ctx->join_ev[i], hipEventDisableTiming));
    }
    DQ_HIP(ctx, hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming));
    return DQ_OK;
}

int ensure_arena(dq_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->arena_cap) return DQ_OK;
    if (ctx->arena) {
        DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        DQ_HIP(ctx, hipFree(ctx->arena));
        ctx->arena = nullptr;
        ctx->arena_cap = 0;
    }
    size_t cap = std::max(bytes, (size_t)64 << 20);
    if (hipMalloc(&ctx->arena, cap) != hipSuccess) {
        ctx->arena = nullptr;
        return fail(ctx, DQ_ERR_OUT_OF_MEMORY, "device arena allocation of %zu bytes failed", cap);
    }
    ctx->arena_cap = cap;
    return DQ_OK;
}

int ensure_pinned(dq_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->pinned_cap) return DQ_OK;
    if (ctx->pinned) {
        DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        DQ_HIP(ctx, hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_cap = 0;
    }
    size_t cap = std::max(bytes, (size_t)1 << 20);
    DQ_HIP(ctx, hipHostMalloc((void**)&ctx->pinned, cap, hipHostMallocDefault));
    ctx->pinned_cap = cap;
    return DQ_OK;
}

// Pinned staging of one call's uploads and read-backs (the buffer is free: the caller synchronised the stream). The
// callers size ctx->pinned from what they stage; a piece that does not fit fails the call instead of being written.
struct Stager {
    dq_ctx* ctx;
    size_t off = 0;
    void* take(size_t n) {
        off = align_up(off, 16);
        if (off + n > ctx->pinned_cap) return nullptr;
        void* h = ctx->pinned + off;
        off += n;
        return h;
    }
    int upload(void* dst, const void* src, size_t n) {
        if (!n) return DQ_OK;
        void* h = take(n);
        if (!h) return fail(ctx, DQ_ERR_DEVICE, "pinned staging of %zu bytes cannot hold %zu more", ctx->pinned_cap, n);
        memcpy(h, src, n);
        DQ_HIP(ctx, hipMemcpyAsync(dst, h, n, hipMemcpyHostToDevice, ctx->stream));
        return DQ_OK;
    }
    // Queues the copy of n device bytes into staging; *h is readable once the stream is synchronised.
    int download(void** h, const void* src, size_t n) {
        *h = take(n);
        if (!*h) return fail(ctx, DQ_ERR_DEVICE, "pinned staging of %zu bytes cannot hold %zu more", ctx->pinned_cap, n);
        DQ_HIP(ctx, hipMemcpyAsync(*h, src, n, hipMemcpyDeviceToHost, ctx->stream));
        return DQ_OK;
    }
};

PredColumn pred_column(const dq_column& col, const void* values, const void* validity, const void* offsets) {
    PredColumn pc;
    memset(&pc, 0, sizeof(pc));
    pc.values = values;
    pc.validity = (const uint64_t*)validity;
    pc.offsets = (const int32_t*)offsets;
    pc.spark_type = col.spark_type;
    pc.elem = elem_of(col.spark_type);
    pc.decimal_scale = col.decimal_scale;
    return pc;
}

// Device addresses of one predicate's program pieces (the arena layout in dq_scan, ScratchBuffers in dq_dict_scan).
struct PredDevice {
    void *prog, *code, *consts, *strings;
};

// Upload and dispatch of one validated predicate over `columns` (pcols_dev: their PredColumn records on the device,
// pc: the same on the host) into TRUE / NOT-NULL bitmaps of `pwords` words: PatternMatch, the simple-predicate kernel
// or the general VM. *status (device, zeroed) is set by a row the device cannot evaluate (regex backtracking budget,
// inexact string -> double); *may_set_status tells whether this predicate can do that.
int run_predicate(dq_ctx* ctx, Stager& up, const dq_predicate& pr, const dq_column* columns, int ncols, const PredColumn* pc,
                  const PredColumn* pcols_dev, const PredDevice& d, int64_t nrows, int64_t pwords, uint64_t* pt, uint64_t* pn,
                  int32_t* status, bool vm_forced, bool* may_set_status) {
    int rc = up.upload(d.code, pr.code, sizeof(int32_t) * (size_t)pr.code_len);
    if (rc) return rc;
    if (pr.n_consts > 0 && (rc = up.upload(d.consts, pr.consts, sizeof(dq_const) * (size_t)pr.n_consts))) return rc;
    if (pr.strings_len > 0 && (rc = up.upload(d.strings, pr.strings, (size_t)pr.strings_len))) return rc;
    PredProgram pg;
    pg.code = (const int32_t*)d.code;
    pg.consts = (const dq_const*)d.consts;
    pg.strings = (const uint8_t*)d.strings;
    pg.code_len = pr.code_len;
    pg.n_consts = pr.n_consts;
    if ((rc = up.upload(d.prog, &pg, sizeof(pg)))) return rc;
    if (pr.code_len == 4 && pr.code[2] == DQ_P_REGEX) {
        const dq_const& k = pr.consts[pr.code[3]];
        launch_regex(pc[pr.code[1]], (const int32_t*)((const uint8_t*)d.strings + k.str_offset), nrows, pwords, pt, pn, status,
                     ctx->stream);
        ctx->kernel_launches[DQ_KERNEL_REGEX]++;
        *may_set_status = true;
    } else if (PredSimple ps; !vm_forced && compile_simple_predicate(pr, columns, ncols, ps)) {
        launch_pred_simple(ps, pcols_dev, nrows, pwords, pt, pn, ctx->stream);
        ctx->kernel_launches[DQ_KERNEL_PRED_SIMPLE]++;
        *may_set_status = false;
    } else {
        // rx: the program holds RLIKE; str: it has a string operand, which a comparison, arithmetic or CAST may have to
        // convert to DOUBLE (a conversion the device cannot round exactly sets status)
        bool rx = false, str = false;
        for (int k = 0; k + 1 < pr.code_len; k += 2) {
            const int a = pr.code[k + 1];
            rx |= pr.code[k] == DQ_P_RLIKE;
            str |= pr.code[k] == DQ_P_COL && a >= 0 && a < ncols && columns[a].spark_type == DQ_TYPE_STRING;
            str |= pr.code[k] == DQ_P_CONST && a >= 0 && a < pr.n_consts && pr.consts[a].tag == DQ_V_STRING;
        }
        launch_predicate((const PredProgram*)d.prog, rx, status, pcols_dev, nrows, pwords, pt, pn, ctx->stream);
        ctx->kernel_launches[DQ_KERNEL_PRED_VM]++;
        *may_set_status = rx || str;
    }
    DQ_HIP(ctx, hipGetLastError());
    return DQ_OK;
}

// One dq_scan call on a single device: its arguments, its plan (scan_plan.h) and, once the arena is sized, the device
// addresses the plan's indices resolve to.
struct ScanCall {
    dq_ctx* ctx;
    const dq_column* columns;
    int ncols;
    int64_t nrows;
    const dq_op* ops;
    int nops;
    const dq_predicate* preds;
    int npreds;
    ScanOptions options;
    ScanUse use;
    ScanPlan plan;
    ScanGeometry geo;
    ScanLayout L;
    bool concurrent = false;
    std::vector<const void*> val, valid, offs;  // per column: device values / validity / string offsets
    std::vector<PredColumn> pc;                 // per column, host copy of the records at L.pcols
    bool any_status = false;                    // some predicate may set its status word: read the words back

    template <class T>
    T* at(size_t off) const { return off == kNoOffset ? nullptr : (T*)(ctx->arena + off); }
    uint64_t* pred_t(int p) const { return p >= 0 ? at<uint64_t>(L.pred[p].t) : nullptr; }
    uint64_t* pred_nn(int p) const { return p >= 0 ? at<uint64_t>(L.pred[p].nn) : nullptr; }
    uint64_t* mask(int p, int m) const { return (uint64_t*)(ctx->arena + L.pred[p].mask0 + (size_t)m * L.mask_stride); }
    int64_t pwords() const { return padded_words_for(nrows); }
};

// ---- resolve: plan record + device addresses -> device descriptor ---------------------------------------------------
SlotDesc resolve_slot(const ScanCall& sc, const PlanSlot& sl) {
    SlotDesc sd;
    memset(&sd, 0, sizeof(sd));
    sd.kind = sl.kind;
    sd.ncols = 1;
    sd.rows_per_load = 8;
    sd.col[0].hll_slot = sd.col[1].hll_slot = -1;
    sd.col[1].elem = ET_NONE;
    sd.where_t = sc.pred_t(sl.where);
    sd.where_nn = sc.pred_nn(sl.where);
    if (sl.kind == SK_VALUES) {
        sd.ncols = sl.ncols;
        sd.corr = sl.corr;
        sd.rows_per_load = sl.rows_per_load;
        for (int k = 0; k < sl.ncols; ++k) {
            const PlanCol& c = sl.col[k];
            ColDesc& cd = sd.col[k];
            cd.values = sc.val[c.column];
            // a consumer of a masked filter reads its mask, valid & where TRUE, in place of its validity
            cd.validity = c.mask_pred >= 0 ? sc.mask(c.mask_pred, c.mask_index) : (const uint64_t*)sc.valid[c.column];
            cd.spark_type = sc.columns[c.column].spark_type;
            cd.elem = c.elem;
            cd.flags = c.flags;
            cd.hll_slot = c.hll_slot;
            cd.pred_op = c.pred_op;
            cd.pred_kind = c.pred_kind;
            cd.pred_i = c.pred_i;
            cd.pred_d = c.pred_d;
        }
        sd.wout = sl.producer_of >= 0 ? sc.at<WhereOut>(sc.L.pred[sl.producer_of].wout) : nullptr;
    } else if (sl.kind == SK_BITS) {
        if (sl.tag == BT_COMPLETENESS) sd.bits_valid = (const uint64_t*)sc.valid[sl.ref];
        if (sl.tag == BT_COMPLIANCE) {
            sd.pred_t = sc.pred_t(sl.ref);
            sd.pred_nn = sc.pred_nn(sl.ref);
        }
    }
    return sd;
}

StrSlot resolve_str_slot(const ScanCall& sc, const PlanStrSlot& ps) {
    StrSlot ss;
    memset(&ss, 0, sizeof(ss));
    ss.data = (const uint8_t*)sc.val[ps.column];
    ss.offsets = (const int32_t*)sc.offs[ps.column];
    ss.values = sc.val[ps.column];
    ss.validity = (const uint64_t*)sc.valid[ps.column];
    ss.where_t = sc.pred_t(ps.where);
    ss.spark_type = sc.columns[ps.column].spark_type;
    ss.decimal_scale = sc.columns[ps.column].decimal_scale;
    ss.flags = ps.flags;
    ss.hll_slot = ps.hll_slot;
    return ss;
}

D128Slot resolve_d128_slot(const ScanCall& sc, const PlanD128Slot& pd) {
    D128Slot ds;
    memset(&ds, 0, sizeof(ds));
    ds.values = sc.val[pd.column];
    ds.validity = (const uint64_t*)sc.valid[pd.column];
    ds.where_t = sc.pred_t(pd.where);
    ds.where_nn = sc.pred_nn(pd.where);
    ds.flags = pd.flags;
    ds.hll_slot = pd.hll_slot;
    ds.scale = sc.columns[pd.column].decimal_scale;
    return ds;
}

WhereOut resolve_where_out(const ScanCall& sc, int p) {
    const WherePlan& wp = sc.plan.where[p];
    WhereOut wo;
    memset(&wo, 0, sizeof(wo));
    wo.prog = wp.prog;
    wo.nmasks = (int)wp.mask_col.size();
    wo.bitmaps = wp.bitmaps ? 1 : 0;
    wo.where_t = sc.pred_t(p);
    wo.where_nn = sc.pred_nn(p);
    for (int m = 0; m < wo.nmasks; ++m) {
        wo.valid[m] = (const uint64_t*)sc.valid[wp.mask_col[m]];
        wo.mask[m] = sc.mask(p, m);
    }
    return wo;
}

// ---- the stages of dq_scan, in call order -----------------------------------------------------------------------------
// A multi-device context: host columns are row-sharded over the devices (multi.cpp).
int scan_multi_device(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops,
                      const dq_predicate* preds, int npreds, dq_state* out, uint32_t flags) {
    if (flags & DQ_SCAN_OUT_DEVICE)
        return fail(ctx, DQ_ERR_UNSUPPORTED, "a multi-device context returns host states (no DQ_SCAN_OUT_DEVICE)");
    for (int c = 0; c < ncols; ++c) {
        if (columns[c].spark_type == DQ_TYPE_DECIMAL128)
            return fail(ctx, DQ_ERR_UNSUPPORTED, "column %d: DECIMAL128 columns need a single-device context", c);
        if (columns[c].flags & DQ_COL_DEVICE)
            return fail(ctx, DQ_ERR_UNSUPPORTED, "device columns of a multi-device context go through dq_scan_sharded");
        if (columns[c].length != nrows)
            return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "column %d has %lld rows, batch has %lld", c,
                        (long long)columns[c].length, (long long)nrows);
    }
    const int n = (int)ctx->subs.size();
    std::vector<std::vector<dq_column>> cols(n, std::vector<dq_column>(std::max(ncols, 1)));
    std::vector<std::vector<std::vector<int32_t>>> scratch(n);
    std::vector<const dq_column*> ptrs(n);
    std::vector<int64_t> rows(n);
    for (int i = 0; i < n; ++i) {
        int64_t r0 = 0;
        shard_bounds(nrows, n, i, &r0, &rows[i]);
        shard_columns(columns, ncols, r0, rows[i], cols[i].data(), scratch[i]);
        ptrs[i] = cols[i].data();
    }
    return multi_scan(ctx, ptrs.data(), rows.data(), ncols, ops, nops, preds, npreds, out);
}

// Grids of the plan's launches: occupancy per shape (cached on the context), the chip shared between concurrent launches.
int scan_geometry(ScanCall& sc) {
    dq_ctx* ctx = sc.ctx;
    std::vector<int> occ;
    occ.reserve(sc.plan.groups.size());
    for (const PlanGroup& g : sc.plan.groups) {
        auto oc = ctx->occupancy.find(g.key);
        if (oc == ctx->occupancy.end())
            oc = ctx->occupancy.emplace(g.key, std::max(1, scan_group_blocks_per_cu(g.kind, g.P, g.nc, g.f0, g.f1, g.heavy))).first;
        occ.push_back(oc->second);
    }
    sc.concurrent = scan_concurrency() && sc.plan.nlaunch() > 1 && ensure_side_streams(ctx) == DQ_OK;
    const int sgrid = sc.plan.sslots.empty() ? 0 : string_scan_grid(ctx->cus, sc.nrows);
    const int dgrid = sc.plan.dslots.empty() ? 0 : decimal128_scan_grid(ctx->cus, sc.nrows);
    sc.geo = plan_geometry(sc.plan, ctx->cus, (sc.nrows + kTileRows - 1) / kTileRows, scan_grid_cap(), sc.concurrent, sgrid,
                           dgrid, occ.data());
    return DQ_OK;
}

// Host columns are copied into the arena; device columns are read in place.
int stage_columns(ScanCall& sc) {
    dq_ctx* ctx = sc.ctx;
    const size_t bitmap_bytes = (size_t)(sc.nrows + 7) / 8;
    sc.val.assign(sc.ncols, nullptr);
    sc.valid.assign(sc.ncols, nullptr);
    sc.offs.assign(sc.ncols, nullptr);
    for (int c = 0; c < sc.ncols; ++c) {
        const dq_column& col = sc.columns[c];
        if (!sc.use.col_used[c]) continue;
        if (col.flags & DQ_COL_DEVICE) {
            sc.val[c] = col.values;
            sc.valid[c] = col.validity;
            sc.offs[c] = col.offsets;
            continue;
        }
        const ScanLayout::Column& lc = sc.L.col[c];
        void* v = sc.at<void>(lc.values);
        void* vd = sc.at<void>(lc.validity);
        void* od = sc.at<void>(lc.offsets);
        if (lc.vbytes) DQ_HIP(ctx, hipMemcpyAsync(v, col.values, lc.vbytes, hipMemcpyHostToDevice, ctx->stream));
        if (vd && bitmap_bytes) DQ_HIP(ctx, hipMemcpyAsync(vd, col.validity, bitmap_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (od) DQ_HIP(ctx, hipMemcpyAsync(od, col.offsets, ((size_t)sc.nrows + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        sc.val[c] = v;
        sc.valid[c] = vd;
        sc.offs[c] = od;
    }
    return DQ_OK;
}

// The predicate passes (bitmaps of unmasked `where` filters and Compliance predicates), then the masked filters'
// descriptors and their standalone producers: all before the first scan launch.
int run_predicates(ScanCall& sc, Stager& up) {
    dq_ctx* ctx = sc.ctx;
    const ScanPlan& plan = sc.plan;
    int32_t* status = sc.at<int32_t>(sc.L.status);
    const PredColumn* pcols = sc.at<PredColumn>(sc.L.pcols);
    int npred_pass = 0;
    for (int p = 0; p < sc.npreds; ++p) npred_pass += plan.pred_pass[p];
    if (npred_pass || plan.nstandalone) {
        DQ_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int32_t) * std::max(sc.npreds, 1), ctx->stream));
        sc.pc.resize(std::max(sc.ncols, 1));
        memset(sc.pc.data(), 0, sizeof(PredColumn) * sc.pc.size());
        for (int c = 0; c < sc.ncols; ++c) sc.pc[c] = pred_column(sc.columns[c], sc.val[c], sc.valid[c], sc.offs[c]);
        int rc = up.upload((void*)pcols, sc.pc.data(), sizeof(PredColumn) * sc.pc.size());
        if (rc) return rc;
        for (int p = 0; p < sc.npreds; ++p) {
            if (!plan.pred_pass[p]) continue;
            const PredOffsets& po = sc.L.pred[p];
            const PredDevice d{sc.at<void>(po.prog), sc.at<void>(po.code), sc.at<void>(po.consts), sc.at<void>(po.strings)};
            bool may = false;
            rc = run_predicate(ctx, up, sc.preds[p], sc.columns, sc.ncols, sc.pc.data(), pcols, d, sc.nrows, sc.pwords(),
                               sc.pred_t(p), sc.pred_nn(p), status + p, sc.options.pred_vm, &may);
            if (rc) return rc;
            sc.any_status |= may;
        }
    }
    for (int p = 0; p < sc.npreds; ++p) {
        const WherePlan& wp = plan.where[p];
        if (!wp.masked) continue;
        const WhereOut wo = resolve_where_out(sc, p);
        WhereOut* wodev = sc.at<WhereOut>(sc.L.pred[p].wout);
        const int rc = up.upload(wodev, &wo, sizeof(wo));
        if (rc) return rc;
        if (wp.producer < 0) {
            launch_where_masks(wodev, wp.prog, pcols, sc.nrows, sc.pwords(), sc.at<SlotPartial>(sc.L.partials), wp.wslot,
                               sc.geo.gstride, sc.geo.slot_nblocks[wp.wslot], ctx->stream);
            DQ_HIP(ctx, hipGetLastError());
            ctx->kernel_launches[DQ_KERNEL_WHERE_MASKS]++;
        }
    }
    return DQ_OK;
}

// Slot descriptors, op maps, launch order and block counts of the value / bits / string launches.
int upload_descriptors(ScanCall& sc, Stager& up) {
    const ScanPlan& plan = sc.plan;
    const int nslots = (int)plan.slots.size();
    std::vector<SlotDesc> slots;
    slots.reserve(nslots);
    for (const PlanSlot& sl : plan.slots) slots.push_back(resolve_slot(sc, sl));
    int rc = up.upload(sc.at<void>(sc.L.slots), slots.data(), sizeof(SlotDesc) * nslots);
    if (rc) return rc;
    if ((rc = up.upload(sc.at<void>(sc.L.ops), plan.opmap.data(), sizeof(OpMap) * sc.nops))) return rc;
    if (nslots) {
        std::vector<int32_t> order;
        order.reserve(nslots);
        for (const PlanGroup& g : plan.groups) order.insert(order.end(), g.slots.begin(), g.slots.end());
        if ((rc = up.upload(sc.at<void>(sc.L.order), order.data(), sizeof(int32_t) * order.size()))) return rc;
        rc = up.upload(sc.at<void>(sc.L.slot_nblocks), sc.geo.slot_nblocks.data(), sizeof(int32_t) * sc.geo.slot_nblocks.size());
        if (rc) return rc;
    }
    std::vector<StrSlot> sslots;
    sslots.reserve(plan.sslots.size());
    for (const PlanStrSlot& ps : plan.sslots) sslots.push_back(resolve_str_slot(sc, ps));
    return up.upload(sc.at<void>(sc.L.sslots), sslots.data(), sizeof(StrSlot) * sslots.size());
}

// The scan launches: fused `where` producers first on the ctx stream (every other launch reads their masks), then the
// other groups and the string scan in order on the ctx stream, or one stream each (fork / join) when concurrent; the
// decimal128 launch after the join.
int launch_scans(ScanCall& sc, Stager& up) {
    dq_ctx* ctx = sc.ctx;
    const ScanPlan& plan = sc.plan;
    const ScanGeometry& geo = sc.geo;
    const int nsslots = (int)plan.sslots.size(), ndslots = (int)plan.dslots.size();
    const SlotDesc* dslots = sc.at<SlotDesc>(sc.L.slots);
    const int32_t* order = sc.at<int32_t>(sc.L.order);
    SlotPartial* partials = sc.at<SlotPartial>(sc.L.partials);
    uint8_t* hllp = sc.at<uint8_t>(sc.L.hll_partials);
    int used_side = 0;
    auto launch_stream = [&](int i) -> hipStream_t {
        if (!sc.concurrent || i == 0) return ctx->stream;
        const int j = (i - 1) % dq_ctx::kSide;
        used_side = std::max(used_side, j + 1);
        return ctx->side[j];
    };
    int li = 0;
    size_t goff = 0, gi = 0;
    auto launch_group = [&](size_t i, hipStream_t st) -> int {
        const PlanGroup& g = plan.groups[i];
        if (launch_scan_group(g.kind, g.P, g.nc, g.f0, g.f1, g.heavy, dslots, order + goff, (int)g.slots.size(), sc.nrows,
                              geo.ntiles, geo.gstride, geo.grid[i], partials, hllp, st) != 0)
            return fail(ctx, DQ_ERR_DEVICE, "scan launch failed for shape (%d,%d,%d)", g.kind, g.P, g.nc);
        DQ_HIP(ctx, hipGetLastError());
        ctx->kernel_launches[scan_kernel_family(g.kind, g.P, g.nc, g.heavy)]++;
        goff += g.slots.size();
        return DQ_OK;
    };
    int rc;
    for (; gi < plan.groups.size() && plan.groups[gi].heavy == 3; ++gi)
        if ((rc = launch_group(gi, ctx->stream))) return rc;
    if (sc.concurrent) {
        DQ_HIP(ctx, hipEventRecord(ctx->fork_ev, ctx->stream));
        for (int j = 0; j < std::min(plan.nlaunch() - 1, dq_ctx::kSide); ++j)
            DQ_HIP(ctx, hipStreamWaitEvent(ctx->side[j], ctx->fork_ev, 0));
    }
    for (; gi < plan.groups.size(); ++gi)
        if ((rc = launch_group(gi, launch_stream(li++)))) return rc;
    if (nsslots) {
        launch_string_scan(sc.at<StrSlot>(sc.L.sslots), nsslots, sc.nrows, geo.sgrid, geo.gstride, sc.at<StrPartial>(sc.L.spartials),
                           hllp, launch_stream(li++));
        DQ_HIP(ctx, hipGetLastError());
        ctx->kernel_launches[DQ_KERNEL_STRINGS]++;
    }
    for (int j = 0; j < used_side; ++j) {
        DQ_HIP(ctx, hipEventRecord(ctx->join_ev[j], ctx->side[j]));
        DQ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->join_ev[j], 0));
    }
    if (ndslots) {
        std::vector<D128Slot> ds;
        ds.reserve(ndslots);
        for (const PlanD128Slot& pd : plan.dslots) ds.push_back(resolve_d128_slot(sc, pd));
        if ((rc = up.upload(sc.at<void>(sc.L.dslots), ds.data(), sizeof(D128Slot) * ndslots))) return rc;
        launch_decimal128_scan(sc.at<D128Slot>(sc.L.dslots), ndslots, sc.nrows, geo.dgrid, geo.gstride,
                               sc.at<D128Partial>(sc.L.dpartials), hllp, ctx->stream);
        DQ_HIP(ctx, hipGetLastError());
        ctx->kernel_launches[DQ_KERNEL_DECIMAL128]++;
    }
    return DQ_OK;
}

// Per-block partials -> final slot partials and HLL registers -> one dq_state per op at `dout`.
int reduce_and_finalize(ScanCall& sc, Stager& up, dq_state* dout) {
    dq_ctx* ctx = sc.ctx;
    const ScanPlan& plan = sc.plan;
    const ScanGeometry& geo = sc.geo;
    const int nslots = (int)plan.slots.size(), nsslots = (int)plan.sslots.size(), ndslots = (int)plan.dslots.size();
    SlotPartial* finals = sc.at<SlotPartial>(sc.L.finals);
    uint8_t* hllf = sc.at<uint8_t>(sc.L.hll_final);
    int rc;
    if (nslots) {
        launch_reduce_partials(sc.at<SlotPartial>(sc.L.partials), sc.at<int32_t>(sc.L.slot_nblocks), nslots, geo.gstride, finals,
                               ctx->stream);
        DQ_HIP(ctx, hipGetLastError());
    }
    if (nslots || nsslots || ndslots) ctx->scan_launches++;
    if (plan.nhll) {
        int32_t* dhll_nb = sc.at<int32_t>(sc.L.hll_nblocks);
        if ((rc = up.upload(dhll_nb, geo.hll_nblocks.data(), sizeof(int32_t) * geo.hll_nblocks.size()))) return rc;
        launch_reduce_hll(sc.at<uint8_t>(sc.L.hll_partials), dhll_nb, plan.nhll, geo.gstride, hllf, ctx->stream);
        DQ_HIP(ctx, hipGetLastError());
    }
    launch_finalize(sc.at<OpMap>(sc.L.ops), sc.nops, finals, hllf, dout, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    if (!plan.sopmap.empty()) {
        StrOpMap* dsops = sc.at<StrOpMap>(sc.L.sops);
        if ((rc = up.upload(dsops, plan.sopmap.data(), sizeof(StrOpMap) * plan.sopmap.size()))) return rc;
        launch_finalize_strings(dsops, (int)plan.sopmap.size(), sc.at<StrPartial>(sc.L.spartials), geo.sgrid, geo.gstride, sc.nrows,
                                dout, ctx->stream);
        DQ_HIP(ctx, hipGetLastError());
    }
    if (!plan.dopmap.empty()) {
        D128OpMap* ddops = sc.at<D128OpMap>(sc.L.dops);
        if ((rc = up.upload(ddops, plan.dopmap.data(), sizeof(D128OpMap) * plan.dopmap.size()))) return rc;
        launch_finalize_decimal128(sc.at<D128Slot>(sc.L.dslots), ndslots, ddops, (int)plan.dopmap.size(),
                                   sc.at<D128Partial>(sc.L.dpartials), geo.dgrid, geo.gstride, sc.nrows, dout, ctx->stream);
        DQ_HIP(ctx, hipGetLastError());
    }
    return DQ_OK;
}

// The predicates' status words, read only when one may be set.
int check_pred_status(ScanCall& sc, Stager& up) {
    dq_ctx* ctx = sc.ctx;
    int rc;
    if (sc.any_status) {
        // a row that exhausted the backtracking budget, or whose string the device cannot convert to DOUBLE exactly,
        // fails the batch (never a silent count)
        void* h = nullptr;
        if ((rc = up.download(&h, sc.at<int32_t>(sc.L.status), sizeof(int32_t) * std::max(sc.npreds, 1)))) return rc;
        DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const int32_t* hs = (const int32_t*)h;
        for (int p = 0; p < sc.npreds; ++p)
            if (sc.plan.pred_pass[p] && (hs[p] & 1))
                return fail(ctx, DQ_ERR_UNSUPPORTED, "predicate %d: regex backtracking limit exceeded", p);
        for (int p = 0; p < sc.npreds; ++p)
            if (sc.plan.pred_pass[p] && hs[p])
                return fail(ctx, DQ_ERR_UNSUPPORTED,
                            "predicate %d: a string needs Double.parseDouble's arbitrary-precision path "
                            "(hexadecimal literal, or > 19 significant digits on a rounding boundary)", p);
    }
    return DQ_OK;
}

// The status words, then the states: to `out`, or left at `out` on the device (DQ_SCAN_OUT_DEVICE), where staged host
// columns must outlive the kernels.
int read_back(ScanCall& sc, Stager& up, const dq_state* dout, dq_state* out, uint32_t flags) {
    dq_ctx* ctx = sc.ctx;
    int rc;
    if ((rc = check_pred_status(sc, up))) return rc;
    if (!(flags & DQ_SCAN_OUT_DEVICE)) {
        void* h = nullptr;
        if ((rc = up.download(&h, dout, sizeof(dq_state) * sc.nops))) return rc;
        DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(out, h, sizeof(dq_state) * sc.nops);
    } else {
        bool staged = false;
        for (int c = 0; c < sc.ncols; ++c) staged |= sc.use.col_used[c] && !(sc.columns[c].flags & DQ_COL_DEVICE);
        if (staged) DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return DQ_OK;
}

// ---- the predicate-bitmap stage of dq_filter_validity and dq_row_outcomes ---------------------------------------------
// A validated call whose ops are one dummy Size(where = p) per predicate (size_where_ops) goes through dq_scan's own
// stages, planned for the bitmap pass (the caller's sc.options.where_masks = false): run_predicates leaves each
// predicate's TRUE / NOT-NULL bitmaps in the arena, once per predicate, and the scan launch itself is never issued.
// extra_pinned: staging of what the caller reads back after it. Without predicates nothing is planned or staged (the
// context's arena is not touched).
int predicate_bitmaps(ScanCall& sc, Stager& up, size_t extra_pinned) {
    dq_ctx* ctx = sc.ctx;
    int rc;
    if (sc.npreds > 0) {
        std::string msg;
        rc = plan_scan(sc.columns, sc.ncols, sc.nrows, sc.ops, sc.nops, sc.preds, sc.npreds, sc.use, sc.options, &sc.plan, &msg);
        if (rc) return fail(ctx, rc, "%s", msg.c_str());
        if ((rc = scan_geometry(sc))) return rc;
        sc.L = layout_scan(sc.plan, sc.geo, sc.use, sc.columns, sc.ncols, sc.nrows, sc.nops, sc.preds, sc.npreds, true);
        if ((rc = ensure_arena(ctx, sc.L.arena_bytes))) return rc;
    }
    if ((rc = ensure_pinned(ctx, sc.L.pinned_bytes + extra_pinned))) return rc;
    if ((rc = stage_columns(sc))) return rc;
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the pinned buffer may still be read by a previous call's copies
    return sc.npreds > 0 ? run_predicates(sc, up) : DQ_OK;
}

// Column c's validity on the device after the predicate stage, nullptr = all valid (validity_source). A host column no
// predicate reads: only its bitmap goes to the device, into per-call scratch, once per call.
int column_validity(ScanCall& sc, ScratchBuffers& buf, int c, const uint8_t** v) {
    dq_ctx* ctx = sc.ctx;
    const dq_column& col = sc.columns[c];
    const int src = validity_source(col, sc.use.col_used[c] != 0);
    if (src == RP_VALID_CALL && !sc.valid[c]) {
        const size_t bitmap_bytes = (size_t)(sc.nrows + 7) / 8;
        void* vd = nullptr;
        DQ_HIP(ctx, buf.alloc(&vd, align_up(bitmap_bytes, 8) + 8));
        DQ_HIP(ctx, hipMemcpyAsync(vd, col.validity, bitmap_bytes, hipMemcpyHostToDevice, ctx->stream));
        sc.valid[c] = vd;
    }
    *v = src == RP_ONES ? nullptr : src == RP_VALID_DEVICE ? col.validity : (const uint8_t*)sc.valid[c];
    return DQ_OK;
}

// The launch arguments of row_outcomes_kernel from the plan's indices and the addresses they name (every RP_VALID_CALL
// column staged by column_validity before).
RowOutcomeArgs resolve_row_args(const RowPlan& plan, const ScanCall& sc, const dq_row_term* terms, const dq_row_check* checks) {
    RowOutcomeArgs args;
    memset(&args, 0, sizeof(args));
    args.nterms = (int32_t)plan.term.size();
    args.nchecks = (int32_t)plan.term_begin.size();
    args.null_mode = plan.null_mode ? 1 : 0;
    args.ninline = (int32_t)plan.inl.size();
    for (int k = 0; k < args.ninline; ++k) {  // the column is one a predicate reads: staged, or read in place
        const PredTerm& q = plan.inl[k];
        RowInlineDev& d = args.inl[k];
        d.values = sc.val[q.col];
        d.validity = (const uint8_t*)sc.valid[q.col];
        d.spark_type = sc.columns[q.col].spark_type;
        d.op = q.op;
        d.dbl = q.dbl;
        d.ci = q.ci;
        d.cd = q.cd;
    }
    for (int c = 0; c < args.nchecks; ++c) {
        args.check[c].pass = (uint64_t*)checks[c].pass_bits;
        args.check[c].values = checks[c].values;
        args.check[c].validity = plan.null_mode ? (uint64_t*)checks[c].validity : nullptr;
        args.check[c].term_begin = plan.term_begin[c];
        args.check[c].term_end = plan.term_end[c];
    }
    for (int i = 0; i < args.nterms; ++i) {
        const RowPlanTerm& pt = plan.term[i];
        RowTermDev& td = args.term[i];
        td.src_inline = -1;
        td.w_inline = (int16_t)pt.w_inline;
        td.w = sc.pred_t(pt.where);
        switch (pt.src) {
            case RP_BITS:
                td.src = terms[pt.term].pass_bits;
                td.src_kind = RS_WORDS;
                td.w = (const uint64_t*)terms[pt.term].considered_bits;
                break;
            case RP_PRED:
                td.src = sc.pred_t(pt.index);
                td.src_kind = RS_WORDS;
                break;
            case RP_INLINE:
                td.src_kind = RS_INLINE;
                td.src_inline = (int16_t)pt.index;
                break;
            case RP_VALID_DEVICE:
                td.src = sc.columns[pt.index].validity;
                td.src_kind = RS_VALID_BYTES;
                break;
            case RP_VALID_SCAN:
            case RP_VALID_CALL:
                td.src = sc.valid[pt.index];
                td.src_kind = RS_VALID_BYTES;
                break;
            default:
                td.src_kind = RS_ONES;
                break;
        }
    }
    return args;
}

}  // namespace

namespace dq {
hipStream_t ctx_stream(dq_ctx* ctx) { return ctx->stream; }
int ctx_device(dq_ctx* ctx) { return ctx->device; }
int ctx_cus(dq_ctx* ctx) { return ctx->cus; }
int ctx_fail(dq_ctx* ctx, int code, const char* msg) { return fail(ctx, code, "%s", msg); }
int ctx_num_subs(dq_ctx* ctx) { return (int)ctx->subs.size(); }
// The context's side streams (created on first use) with its fork event and one join event per side stream; returns
// their number, 0 when they cannot be created.
int ctx_side_streams(dq_ctx* ctx, hipStream_t* side, hipEvent_t* fork, hipEvent_t* join) {
    if (ensure_side_streams(ctx) != DQ_OK) return 0;
    for (int i = 0; i < dq_ctx::kSide; ++i) {
        side[i] = ctx->side[i];
        join[i] = ctx->join_ev[i];
    }
    *fork = ctx->fork_ev;
    return dq_ctx::kSide;
}
dq_ctx* ctx_sub(dq_ctx* ctx, int i) { return ctx->subs[i]; }
// The context's device arena / pinned staging buffer, grown to `bytes` (NULL + error set on failure).
// Used by one call at a time (a ctx is not re-entrant); work queued on the ctx stream stays ordered.
void* ctx_scratch(dq_ctx* ctx, size_t bytes) { return ensure_arena(ctx, bytes) == DQ_OK ? ctx->arena : nullptr; }
void* ctx_pinned_buf(dq_ctx* ctx, size_t bytes) {
    if (ensure_pinned(ctx, bytes) != DQ_OK) return nullptr;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;  // earlier copies from it are done
    return ctx->pinned;
}

constexpr size_t kScratchCacheCap = size_t(48) << 30;  // idle bytes kept for re-use

// Every open single-device context, so an allocation that fails can release the idle scratch of the device's
// other contexts (helper contexts keep their caches between runs).
std::mutex g_ctx_mu;
std::vector<dq_ctx*> g_ctxs;

void register_ctx(dq_ctx* ctx) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    g_ctxs.push_back(ctx);
}

void unregister_ctx(dq_ctx* ctx) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), ctx), g_ctxs.end());
}

void free_blocks(int device, const std::vector<dq_ctx::CachedBlock>& blocks) {
    if (blocks.empty()) return;
    (void)hipSetDevice(device);
    for (const dq_ctx::CachedBlock& b : blocks) {
        (void)hipStreamSynchronize(b.stream);  // its last use was queued there
        (void)hipFree(b.ptr);
    }
}

// Take the cached blocks beyond keep_bytes (oldest first) out of the cache under its lock.
std::vector<dq_ctx::CachedBlock> take_blocks(dq_ctx* ctx, size_t keep_bytes) {
    std::vector<dq_ctx::CachedBlock> out;
    std::lock_guard<std::mutex> g(ctx->scratch_mu);
    size_t i = 0;
    while (ctx->scratch_cached > keep_bytes && i < ctx->scratch_free.size()) {
        out.push_back(ctx->scratch_free[i]);
        ctx->scratch_cached -= ctx->scratch_free[i].bytes;
        ++i;
    }
    ctx->scratch_free.erase(ctx->scratch_free.begin(), ctx->scratch_free.begin() + i);
    return out;
}

void scratch_trim(dq_ctx* ctx, size_t keep_bytes) { free_blocks(ctx->device, take_blocks(ctx, keep_bytes)); }

// Release the idle scratch of the device's other contexts (an allocation of `ctx` failed).
void trim_device_peers(dq_ctx* ctx) {
    std::vector<dq_ctx::CachedBlock> blocks;
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        for (dq_ctx* o : g_ctxs) {
            if (o == ctx || o->device != ctx->device) continue;
            std::vector<dq_ctx::CachedBlock> b = take_blocks(o, 0);
            blocks.insert(blocks.end(), b.begin(), b.end());
        }
    }
    free_blocks(ctx->device, blocks);
}

void* scratch_alloc(dq_ctx* ctx, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    {
        std::unique_lock<std::mutex> g(ctx->scratch_mu);
        int best = -1;
        for (int i = 0; i < (int)ctx->scratch_free.size(); ++i) {
            const size_t b = ctx->scratch_free[i].bytes;
            if (b >= bytes && b <= 2 * bytes && (best < 0 || b < ctx->scratch_free[best].bytes)) best = i;
        }
        if (best >= 0) {
            dq_ctx::CachedBlock blk = ctx->scratch_free[best];
            ctx->scratch_free.erase(ctx->scratch_free.begin() + best);
            ctx->scratch_cached -= blk.bytes;
            g.unlock();
            // last used on another stream (dq_set_stream since): that work must be done before this stream reuses it
            if (blk.stream != ctx->stream && hipStreamSynchronize(blk.stream) != hipSuccess) {
                (void)hipFree(blk.ptr);
                return nullptr;
            }
            return blk.ptr;
        }
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) == hipSuccess) return p;
    (void)hipGetLastError();
    scratch_trim(ctx);  // the cache may hold what this allocation needs
    if (hipMalloc(&p, bytes) == hipSuccess) return p;
    (void)hipGetLastError();
    trim_device_peers(ctx);  // then the idle caches of the device's other contexts
    if (hipMalloc(&p, bytes) == hipSuccess) return p;
    (void)hipGetLastError();
    return nullptr;
}

void scratch_release(dq_ctx* ctx, void* ptr, size_t bytes) {
    if (!ptr) return;
    bytes = std::max<size_t>(bytes, 256);
    {
        std::lock_guard<std::mutex> g(ctx->scratch_mu);
        ctx->scratch_free.push_back(dq_ctx::CachedBlock{ptr, bytes, ctx->stream});
        ctx->scratch_cached += bytes;
    }
    scratch_trim(ctx, kScratchCacheCap);  // beyond the cap: the oldest blocks (their stream's queued work first)
}
}  // namespace dq

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

int dq_abi_version(void) { return DQ_ABI_VERSION; }

dq_ctx* dq_open(int device, int* status) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        if (status) *status = DQ_ERR_NO_DEVICE;
        return nullptr;
    }
    if (device < 0 || device >= n) {
        if (status) *status = DQ_ERR_INVALID_ARGUMENT;
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        if (status) *status = DQ_ERR_DEVICE;
        return nullptr;
    }
    dq_ctx* ctx = new dq_ctx();
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        if (status) *status = DQ_ERR_DEVICE;
        return nullptr;
    }
    ctx->stream = ctx->own_stream;
    register_ctx(ctx);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->cus = prop.multiProcessorCount;
    if (status) *status = DQ_OK;
    return ctx;
}

void dq_close(dq_ctx* ctx) {
    if (!ctx) return;
    if (!ctx->subs.empty()) close_subs(ctx);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    unregister_ctx(ctx);
    scratch_trim(ctx);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    for (int i = 0; i < dq_ctx::kSide; ++i) {
        if (ctx->side[i]) (void)hipStreamDestroy(ctx->side[i]);
        if (ctx->join_ev[i]) (void)hipEventDestroy(ctx->join_ev[i]);
    }
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char* dq_last_error(const dq_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dq_set_stream(dq_ctx* ctx, void* stream) {
    if (!ctx) return DQ_ERR_INVALID_ARGUMENT;
    ctx->stream = stream ? (hipStream_t)stream : ctx->own_stream;
    return DQ_OK;
}

int dq_set_priority(dq_ctx* ctx, int priority) {
    if (!ctx || priority < -1 || priority > 1) return DQ_ERR_INVALID_ARGUMENT;
    for (dq_ctx* sub : ctx->subs) {
        const int rc = dq_set_priority(sub, priority);
        if (rc) return fail(ctx, rc, "device %d: %s", sub->device, sub->err.c_str());
    }
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    int least = 0, greatest = 0;
    DQ_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    const int want = priority > 0 ? greatest : priority < 0 ? least : std::min(std::max(0, greatest), least);
    if (want == ctx->hip_priority) return DQ_OK;
    // the old streams' queued work first: cached scratch blocks and events are re-tagged to the new streams
    DQ_HIP(ctx, hipStreamSynchronize(ctx->own_stream));
    for (int i = 0; i < dq_ctx::kSide; ++i)
        if (ctx->side[i]) DQ_HIP(ctx, hipStreamSynchronize(ctx->side[i]));
    hipStream_t fresh = nullptr;
    DQ_HIP(ctx, hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, want));
    const hipStream_t old = ctx->own_stream;
    {
        std::lock_guard<std::mutex> g(ctx->scratch_mu);
        for (dq_ctx::CachedBlock& b : ctx->scratch_free)
            if (b.stream == old) b.stream = fresh;
    }
    if (ctx->stream == old) ctx->stream = fresh;
    ctx->own_stream = fresh;
    (void)hipStreamDestroy(old);
    ctx->hip_priority = want;
    for (int i = 0; i < dq_ctx::kSide; ++i) {
        if (!ctx->side[i]) continue;
        (void)hipStreamDestroy(ctx->side[i]);
        DQ_HIP(ctx, hipStreamCreateWithPriority(&ctx->side[i], hipStreamNonBlocking, want));
    }
    return DQ_OK;
}

void dq_scratch_trim(dq_ctx* ctx, int64_t keep_bytes) {
    if (!ctx) return;
    for (dq_ctx* sub : ctx->subs) dq_scratch_trim(sub, keep_bytes);
    scratch_trim(ctx, (size_t)std::max<int64_t>(keep_bytes, 0));
}

int dq_synchronize(dq_ctx* ctx) {
    if (!ctx) return DQ_ERR_INVALID_ARGUMENT;
    for (dq_ctx* sub : ctx->subs) {
        const int rc = dq_synchronize(sub);
        if (rc) return fail(ctx, rc, "device %d: %s", sub->device, sub->err.c_str());
    }
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DQ_OK;
}

int64_t dq_scan_launch_count(const dq_ctx* ctx) { return ctx ? ctx->scan_launches : -1; }

int64_t dq_scan_kernel_launches(const dq_ctx* ctx, int32_t kernel) {
    if (!ctx || kernel < 0 || kernel >= DQ_KERNEL_COUNT) return -1;
    int64_t n = ctx->kernel_launches[kernel];
    for (const dq_ctx* sub : ctx->subs) n += sub->kernel_launches[kernel];
    return n;
}

int64_t dq_freq_path_count(const dq_ctx* ctx, int32_t path) {
    if (!ctx || path < 0 || path >= DQ_FREQ_PATH_COUNT) return -1;
    int64_t n = ctx->freq_paths[path];
    for (const dq_ctx* sub : ctx->subs) n += sub->freq_paths[path];
    return n;
}

int dq_scan(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops,
            const dq_predicate* preds, int npreds, dq_state* out, uint32_t flags) {
    if (!ctx) return DQ_ERR_INVALID_ARGUMENT;
    ctx->err.clear();
    if (nops < 0 || ncols < 0 || npreds < 0 || nrows < 0 || (nops > 0 && (!ops || !out)))
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "invalid arguments");
    if (nops == 0) return DQ_OK;
    if (!ctx->subs.empty()) return scan_multi_device(ctx, columns, ncols, nrows, ops, nops, preds, npreds, out, flags);
    DQ_HIP(ctx, hipSetDevice(ctx->device));

    // validate, plan, geometry, layout: pure host functions of the arguments (scan_plan.cpp)
    ScanCall sc{ctx, columns, ncols, nrows, ops, nops, preds, npreds};
    std::string msg;
    int rc = validate_scan(columns, ncols, nrows, ops, nops, preds, npreds, &sc.use, &msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    // DQ_WHERE_MASKS=0 / DQ_PRED_VM=1: the bitmap pass for every `where`; DQ_WHERE_FUSED=0: every masked filter from
    // where_masks_kernel, the filter column a consumer (A/B runs; read per call)
    const char* masks = getenv("DQ_WHERE_MASKS");
    const char* fused = getenv("DQ_WHERE_FUSED");
    sc.options.where_masks = !(masks && masks[0] == '0');
    sc.options.fused_producer = !(fused && fused[0] == '0');
    sc.options.pred_vm = pred_vm_forced();
    rc = plan_scan(columns, ncols, nrows, ops, nops, preds, npreds, sc.use, sc.options, &sc.plan, &msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    if ((rc = scan_geometry(sc))) return rc;
    sc.L = layout_scan(sc.plan, sc.geo, sc.use, columns, ncols, nrows, nops, preds, npreds, flags & DQ_SCAN_OUT_DEVICE);
    if ((rc = ensure_arena(ctx, sc.L.arena_bytes))) return rc;
    if ((rc = ensure_pinned(ctx, sc.L.pinned_bytes))) return rc;

    if ((rc = stage_columns(sc))) return rc;
    // The pinned buffer may still be read by a previous call's async copies: wait for them.
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    Stager up{ctx};
    if ((rc = run_predicates(sc, up))) return rc;
    if ((rc = upload_descriptors(sc, up))) return rc;
    if ((rc = launch_scans(sc, up))) return rc;
    dq_state* dout = (flags & DQ_SCAN_OUT_DEVICE) ? out : sc.at<dq_state>(sc.L.out);
    if ((rc = reduce_and_finalize(sc, up, dout))) return rc;
    return read_back(sc, up, dout, out, flags);
}

// Stages: argument checks and validate_scan, the predicate-bitmap stage (predicate_bitmaps: the filter's TRUE bitmap
// lands in the arena), every target's validity (column_validity), then one filter_validity_kernel launch (filter.hip)
// ANDs the bitmap into them, and the TRUE-row count is read back.
int dq_filter_validity(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_predicate* pred,
                       const int32_t* target_columns, int ntargets, uint8_t* const* out_validity_dev, int64_t* true_rows) {
    if (!ctx) return DQ_ERR_INVALID_ARGUMENT;
    ctx->err.clear();
    if (!columns || ncols <= 0 || nrows < 0 || !pred || ntargets < 0 || !true_rows ||
        (ntargets > 0 && (!target_columns || !out_validity_dev)))
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_filter_validity: invalid arguments");
    *true_rows = 0;
    if (!ctx->subs.empty()) return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_filter_validity: multi-device contexts are not supported");
    if (ntargets > kFilterTargets)
        return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_filter_validity: %d targets, at most %d per call", ntargets, kFilterTargets);
    for (int j = 0; j < ntargets; ++j) {
        const int c = target_columns[j];
        if (c < 0 || c >= ncols) return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_filter_validity: target %d names column %d", j, c);
        if (columns[c].length != nrows)
            return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "column %d has %lld rows, batch has %lld", c, (long long)columns[c].length,
                        (long long)nrows);
        if (!out_validity_dev[j]) return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_filter_validity: target %d has no output bitmap", j);
        if (((uintptr_t)out_validity_dev[j] & 7) || ((columns[c].flags & DQ_COL_DEVICE) && ((uintptr_t)columns[c].validity & 7)))
            return fail(ctx, DQ_ERR_ALIGNMENT, "dq_filter_validity: bitmaps must be 8-B aligned (target %d)", j);
    }
    DQ_HIP(ctx, hipSetDevice(ctx->device));

    const std::vector<dq_op> ops = size_where_ops(1);
    ScanCall sc{ctx, columns, ncols, nrows, ops.data(), 1, pred, 1};
    std::string msg;
    int rc = validate_scan(columns, ncols, nrows, ops.data(), 1, pred, 1, &sc.use, &msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    if (nrows == 0) return DQ_OK;
    sc.options.where_masks = false;  // the bitmap pass: TRUE / NOT-NULL bitmaps from a predicate launch
    sc.options.pred_vm = pred_vm_forced();
    Stager up{ctx};
    if ((rc = predicate_bitmaps(sc, up, 64))) return rc;  // + the TRUE-row count's read-back

    ScratchBuffers buf(ctx);
    FilterTargets ft;
    memset(&ft, 0, sizeof(ft));
    ft.ntargets = ntargets;
    for (int j = 0; j < ntargets; ++j) {
        ft.out[j] = (uint64_t*)out_validity_dev[j];
        if ((rc = column_validity(sc, buf, target_columns[j], &ft.valid[j]))) return rc;
    }
    unsigned long long* dcount = nullptr;
    DQ_HIP(ctx, buf.alloc((void**)&dcount, sizeof(*dcount)));
    DQ_HIP(ctx, hipMemsetAsync(dcount, 0, sizeof(*dcount), ctx->stream));
    if (launch_filter_validity(sc.pred_t(0), ft, nrows, dcount, ctx->stream) != 0)
        return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_filter_validity: more than 2^45 rows in one call (filter in chunks)");
    DQ_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_FILTER_VALIDITY]++;
    if ((rc = check_pred_status(sc, up))) {
        (void)hipStreamSynchronize(ctx->stream);  // staged host bitmaps must outlive the kernels
        return rc;
    }
    void* h = nullptr;
    if ((rc = up.download(&h, dcount, sizeof(*dcount)))) return rc;
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *true_rows = (int64_t) * (const unsigned long long*)h;
    return DQ_OK;
}

// Stages: the plan (plan_row_outcomes), the predicate-bitmap stage (predicate_bitmaps: each TRUE bitmap lands in the
// arena once per predicate, however many terms and filters name it), the host validity bitmaps no predicate reads, the
// launch arguments (resolve_row_args), then one row_outcomes_kernel launch (rowlevel.hip) folds the terms into every
// check's outputs and the counts, which are read back in the caller's term order. A predicate `column <op> constant` over
// a numeric column -- the form dq_scan fuses into a value scan -- gets no pass of its own: that launch evaluates it from
// the column (RowInlineDev, up to kRowInline per call), so the call costs no more predicate launches than the same
// predicates do as one scan's Compliance ops.
int dq_row_outcomes(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_predicate* preds, int npreds,
                    const dq_row_term* terms, int nterms, const dq_row_check* checks, int nchecks, uint32_t flags,
                    int64_t* term_counts, int64_t* check_counts) {
    if (!ctx) return DQ_ERR_INVALID_ARGUMENT;
    ctx->err.clear();
    if (ncols < 0 || nrows < 0 || npreds < 0 || nterms < 0 || nchecks <= 0 || !checks || !check_counts ||
        (ncols > 0 && !columns) || (npreds > 0 && !preds) || (nterms > 0 && (!terms || !term_counts)))
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: invalid arguments");
    if (!ctx->subs.empty()) return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_row_outcomes: multi-device contexts are not supported");
    // every other check, the term order, the inline predicates and every term's source: pure host (call_plans.cpp)
    RowPlan rp;
    std::string msg;
    int rc = plan_row_outcomes(columns, ncols, nrows, preds, npreds, terms, nterms, checks, nchecks, flags, pred_vm_forced(), &rp, &msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    for (int t = 0; t < 2 * nterms; ++t) term_counts[t] = 0;
    for (int c = 0; c < 2 * nchecks; ++c) check_counts[c] = 0;
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    if (nrows == 0) return DQ_OK;

    const std::vector<dq_op> ops = size_where_ops(npreds);
    ScanCall sc{ctx, columns, ncols, nrows, ops.data(), npreds, preds, npreds};
    sc.options = std::move(rp.options);
    sc.use = std::move(rp.use);
    const size_t count_bytes = sizeof(unsigned long long) * kRowCounters;
    Stager up{ctx};
    if ((rc = predicate_bitmaps(sc, up, count_bytes + 64))) return rc;  // + the counts' read-back

    ScratchBuffers buf(ctx);
    const uint8_t* v = nullptr;
    for (const RowPlanTerm& pt : rp.term)
        if (pt.src == RP_VALID_CALL && (rc = column_validity(sc, buf, pt.index, &v))) return rc;
    const RowOutcomeArgs args = resolve_row_args(rp, sc, terms, checks);
    unsigned long long* dcounts = nullptr;
    DQ_HIP(ctx, buf.alloc((void**)&dcounts, count_bytes));
    DQ_HIP(ctx, hipMemsetAsync(dcounts, 0, count_bytes, ctx->stream));
    if (launch_row_outcomes(args, nrows, dcounts, ctx->stream) != 0)
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_row_outcomes: nothing to launch");
    DQ_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_ROW_OUTCOMES]++;
    if ((rc = check_pred_status(sc, up))) {
        (void)hipStreamSynchronize(ctx->stream);  // staged host bitmaps must outlive the kernels
        return rc;
    }
    void* h = nullptr;
    if ((rc = up.download(&h, dcounts, count_bytes))) return rc;
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long* hc = (const unsigned long long*)h;
    for (int i = 0; i < nterms; ++i) {
        term_counts[2 * rp.term[i].term] = (int64_t)hc[2 * i];
        term_counts[2 * rp.term[i].term + 1] = (int64_t)hc[2 * i + 1];
    }
    for (int c = 0; c < 2 * nchecks; ++c) check_counts[c] = (int64_t)hc[2 * DQ_ROW_MAX_TERMS + c];
    return DQ_OK;
}

// Host columns streamed through HBM in row chunks (tables larger than HBM, or host-resident batches): the copy
// of chunk i + 1 (its own stream, double-buffered device chunks) overlaps the fused scan of chunk i; every chunk's
// states land in device memory and the chunks are folded in row order with the reference merges (the partition
// merge of R/AnalysisRunner.scala:313) — the same result as any other row partitioning.
int dq_scan_streamed(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_op* ops, int nops,
                     const dq_predicate* preds, int npreds, dq_state* out, int64_t chunk_rows) {
    if (!ctx || (nops > 0 && (!ops || !out)) || ncols < 0 || nrows < 0 || chunk_rows <= 0)
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_scan_streamed: invalid arguments");
    ctx->err.clear();
    if (!ctx->subs.empty()) return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_scan_streamed takes a single-device context");
    for (int c = 0; c < ncols; ++c) {
        if ((columns[c].flags & DQ_COL_DEVICE) || columns[c].length != nrows)
            return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_scan_streamed: column %d must be a host column of %lld rows", c,
                        (long long)nrows);
        if (columns[c].spark_type == DQ_TYPE_DECIMAL128)
            return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_scan_streamed: column %d: DECIMAL128 columns go through dq_scan", c);
    }
    if (nops == 0) return DQ_OK;
    chunk_rows = std::max<int64_t>(kTileRows, chunk_rows / kTileRows * kTileRows);
    if (nrows <= chunk_rows) return dq_scan(ctx, columns, ncols, nrows, ops, nops, preds, npreds, out, 0);
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t nchunks = (nrows + chunk_rows - 1) / chunk_rows;
    // device chunk buffers: 2 sets, each sized for the largest chunk of every column
    std::vector<size_t> vcap(ncols, 0), bcap(ncols, 0), ocap(ncols, 0);
    for (int c = 0; c < ncols; ++c) {
        const dq_column& col = columns[c];
        if (col.spark_type == DQ_TYPE_STRING) {
            size_t mx = 0;
            for (int64_t k = 0; k < nchunks; ++k) {
                const int64_t r0 = k * chunk_rows, r1 = std::min(nrows, r0 + chunk_rows);
                mx = std::max<size_t>(mx, (size_t)(col.offsets[r1] - col.offsets[r0]));
            }
            vcap[c] = mx + 16;
            ocap[c] = ((size_t)chunk_rows + 1) * 4;
        } else {
            vcap[c] = (size_t)chunk_rows * elem_size(elem_of(col.spark_type)) + 16;
        }
        if (col.validity) bcap[c] = (size_t)chunk_rows / 8 + 8;
    }
    struct Set { std::vector<void*> v, b, o; hipEvent_t copied, scanned; };
    Set sets[2];
    hipStream_t cstream = nullptr;
    std::vector<void*> allocs;
    dq_state* dstates = nullptr;
    std::vector<std::vector<int32_t>> rebased(2 * std::max(ncols, 1));
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        if (cstream) { (void)hipStreamSynchronize(cstream); (void)hipStreamDestroy(cstream); }
        for (Set& st : sets) {
            if (st.copied) (void)hipEventDestroy(st.copied);
            if (st.scanned) (void)hipEventDestroy(st.scanned);
        }
        for (void* p : allocs) (void)hipFree(p);
    };
    for (Set& st : sets) {
        st.copied = st.scanned = nullptr;
        st.v.assign(ncols, nullptr);
        st.b.assign(ncols, nullptr);
        st.o.assign(ncols, nullptr);
    }
    int rc = DQ_OK;
    auto dalloc = [&](size_t bytes) -> void* {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        allocs.push_back(p);
        return p;
    };
    for (Set& st : sets) {
        for (int c = 0; c < ncols && rc == DQ_OK; ++c) {
            if (!(st.v[c] = dalloc(vcap[c]))) rc = DQ_ERR_OUT_OF_MEMORY;
            if (bcap[c] && !(st.b[c] = dalloc(bcap[c]))) rc = DQ_ERR_OUT_OF_MEMORY;
            if (ocap[c] && !(st.o[c] = dalloc(ocap[c]))) rc = DQ_ERR_OUT_OF_MEMORY;
        }
        if (rc == DQ_OK && (hipEventCreateWithFlags(&st.copied, hipEventDisableTiming) != hipSuccess ||
                            hipEventCreateWithFlags(&st.scanned, hipEventDisableTiming) != hipSuccess))
            rc = DQ_ERR_DEVICE;
    }
    if (rc == DQ_OK && !(dstates = (dq_state*)dalloc(sizeof(dq_state) * (size_t)nops * nchunks))) rc = DQ_ERR_OUT_OF_MEMORY;
    if (rc == DQ_OK && hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking) != hipSuccess) rc = DQ_ERR_DEVICE;
    if (rc != DQ_OK) {
        cleanup();
        return fail(ctx, rc, "dq_scan_streamed: chunk buffers of %lld rows do not fit", (long long)chunk_rows);
    }
    auto issue_copy = [&](int64_t k) -> int {
        Set& st = sets[k & 1];
        const int64_t r0 = k * chunk_rows, n = std::min(nrows, r0 + chunk_rows) - r0;
        for (int c = 0; c < ncols; ++c) {
            const dq_column& col = columns[c];
            if (col.spark_type == DQ_TYPE_STRING) {
                std::vector<int32_t>& ro = rebased[(k & 1) * ncols + c];
                ro.resize((size_t)n + 1);
                const int32_t base = col.offsets[r0];
                for (int64_t i = 0; i <= n; ++i) ro[i] = col.offsets[r0 + i] - base;
                if (ro[n]) DQ_HIP(ctx, hipMemcpyAsync(st.v[c], (const uint8_t*)col.values + base, ro[n], hipMemcpyHostToDevice, cstream));
                DQ_HIP(ctx, hipMemcpyAsync(st.o[c], ro.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, cstream));
            } else {
                const size_t es = elem_size(elem_of(col.spark_type));
                DQ_HIP(ctx, hipMemcpyAsync(st.v[c], (const uint8_t*)col.values + r0 * es, (size_t)n * es,
                                           hipMemcpyHostToDevice, cstream));
            }
            if (col.validity)
                DQ_HIP(ctx, hipMemcpyAsync(st.b[c], col.validity + r0 / 8, (size_t)(n + 7) / 8, hipMemcpyHostToDevice, cstream));
        }
        DQ_HIP(ctx, hipEventRecord(st.copied, cstream));
        return DQ_OK;
    };
    rc = issue_copy(0);
    std::vector<dq_column> dcols(std::max(ncols, 1));
    for (int64_t k = 0; k < nchunks && rc == DQ_OK; ++k) {
        Set& st = sets[k & 1];
        if (k + 1 < nchunks) {
            // buffer set (k + 1) & 1 was read by chunk k - 1's scan: wait for it, then start the next copy
            if (k >= 1 && hipEventSynchronize(sets[(k + 1) & 1].scanned) != hipSuccess) { rc = DQ_ERR_DEVICE; break; }
            rc = issue_copy(k + 1);
            if (rc) break;
        }
        if (hipStreamWaitEvent(ctx->stream, st.copied, 0) != hipSuccess) { rc = DQ_ERR_DEVICE; break; }
        const int64_t r0 = k * chunk_rows, n = std::min(nrows, r0 + chunk_rows) - r0;
        for (int c = 0; c < ncols; ++c) {
            dcols[c] = columns[c];
            dcols[c].flags |= DQ_COL_DEVICE;
            dcols[c].length = n;
            dcols[c].values = st.v[c];
            dcols[c].validity = columns[c].validity ? (const uint8_t*)st.b[c] : nullptr;
            dcols[c].offsets = columns[c].spark_type == DQ_TYPE_STRING ? (const int32_t*)st.o[c] : nullptr;
        }
        rc = dq_scan(ctx, dcols.data(), ncols, n, ops, nops, preds, npreds, dstates + (size_t)k * nops, DQ_SCAN_OUT_DEVICE);
        if (rc) break;
        if (hipEventRecord(st.scanned, ctx->stream) != hipSuccess) { rc = DQ_ERR_DEVICE; break; }
    }
    std::vector<dq_state> hst;
    if (rc == DQ_OK) {
        hst.resize((size_t)nops * nchunks);
        if (hipMemcpyAsync(hst.data(), dstates, sizeof(dq_state) * hst.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = DQ_ERR_DEVICE;
    }
    const std::string err = ctx->err;
    cleanup();
    if (rc) return fail(ctx, rc, "%s", err.empty() ? "dq_scan_streamed failed" : err.c_str());
    rc = dq_state_fold(hst.data(), (int)nchunks, nops, out);  // chunks in row order
    if (rc) return fail(ctx, rc, "dq_scan_streamed: state fold failed");
    return DQ_OK;
}

int dq_synth_column(dq_ctx* ctx, int32_t kind, uint64_t seed, int64_t row0, int64_t nrows, void* values_dev) {
    if (!ctx || nrows < 0 || (!values_dev && nrows > 0) || kind < DQ_SYNTH_DYADIC || kind > DQ_SYNTH_GAUSS_CORR)
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_synth_column: invalid arguments");
    if (nrows == 0) return DQ_OK;
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    launch_synth_column(kind, seed, row0, nrows, values_dev, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    return DQ_OK;
}

int dq_synth_strings(dq_ctx* ctx, int32_t kind, uint64_t seed, int64_t row0, int64_t nrows, int32_t* offsets_dev,
                     void* bytes_dev, int64_t* total_bytes) {
    if (!ctx || nrows < 0 || !offsets_dev || !total_bytes || kind < DQ_SYNTH_STR_CAT50 || kind > DQ_SYNTH_STR_TEXT)
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_synth_strings: invalid arguments");
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    if (!bytes_dev) {
        // lengths into offsets[1..n], then an exclusive scan on the host (offsets are int32: < 2 GiB of text)
        DQ_HIP(ctx, hipMemsetAsync(offsets_dev, 0, 4, ctx->stream));
        if (nrows) launch_synth_string_lengths(kind, seed, row0, nrows, offsets_dev + 1, ctx->stream);
        DQ_HIP(ctx, hipGetLastError());
        std::vector<int32_t> h((size_t)nrows + 1);
        DQ_HIP(ctx, hipMemcpyAsync(h.data(), offsets_dev, ((size_t)nrows + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
        DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        int64_t acc = 0;
        for (int64_t i = 1; i <= nrows; ++i) {
            acc += h[(size_t)i];
            if (acc > INT32_MAX) return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_synth_strings: more than 2 GiB of text");
            h[(size_t)i] = (int32_t)acc;
        }
        DQ_HIP(ctx, hipMemcpyAsync(offsets_dev, h.data(), ((size_t)nrows + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *total_bytes = acc;
        return DQ_OK;
    }
    if (nrows) launch_synth_string_bytes(kind, seed, row0, nrows, offsets_dev, bytes_dev, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    return DQ_OK;
}

int dq_synth_freq_keys(dq_ctx* ctx, int64_t total_rows, int64_t distinct, int64_t row0, int64_t nrows, int64_t* keys_dev) {
    if (!ctx || total_rows <= 0 || distinct <= 0 || distinct > total_rows || nrows < 0 || row0 < 0 ||
        row0 + nrows > total_rows || (!keys_dev && nrows > 0))
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_synth_freq_keys: invalid arguments");
    if (nrows == 0) return DQ_OK;
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    launch_synth_freq_keys(total_rows, distinct, row0, nrows, keys_dev, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    return DQ_OK;
}

int dq_synth_validity(dq_ctx* ctx, uint64_t seed, int64_t row0, int64_t nrows, int32_t null_permille, uint8_t* validity_dev) {
    if (!ctx || nrows < 0 || (!validity_dev && nrows > 0) || null_permille < 0 || null_permille > 1000)
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_synth_validity: invalid arguments");
    if (nrows == 0) return DQ_OK;
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    launch_synth_validity(seed, row0, nrows, null_permille, validity_dev, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    return DQ_OK;
}

}  // extern "C"

// ---- dictionary-encoded STRING columns (dict.hip) ---------------------------------------------------------------------
namespace {

// DQ_DICT_LDS_ENTRIES=n: dictionaries of up to n entries count in LDS (at most kDictLdsWords); DQ_DICT_LDS_COPIES=1, 2
// or 4: fewer LDS counter copies (measurements). Read per call.
DictOptions dict_options() {
    DictOptions o;
    if (const char* e = getenv("DQ_DICT_LDS_ENTRIES")) o.lds_entries = (int)std::max<long>(0, std::min<long>(atol(e), kDictLdsWords));
    if (const char* e = getenv("DQ_DICT_LDS_COPIES")) o.lds_copies = atoi(e);
    return o;
}

// One validated predicate of dq_dict_scan: its program pieces in per-call scratch, then the stage dq_scan uses.
int dict_predicate(dq_ctx* ctx, Stager& up, ScratchBuffers& buf, const dq_predicate& pr, const dq_column* columns, int ncols,
                   const PredColumn* pc, const PredColumn* pcols_dev, int64_t nrows, uint64_t* pt, uint64_t* pn, int32_t* status) {
    PredDevice d{};
    DQ_HIP(ctx, buf.alloc(&d.code, sizeof(int32_t) * (size_t)pr.code_len));
    DQ_HIP(ctx, buf.alloc(&d.consts, sizeof(dq_const) * (size_t)std::max(pr.n_consts, 1)));
    DQ_HIP(ctx, buf.alloc(&d.strings, (size_t)std::max<int64_t>(pr.strings_len, 1) + 16));
    DQ_HIP(ctx, buf.alloc(&d.prog, sizeof(PredProgram)));
    bool may_set_status;  // every status word of the call is read back
    return run_predicate(ctx, up, pr, columns, ncols, pc, pcols_dev, d, nrows, padded_words_for(nrows), pt, pn, status,
                         pred_vm_forced(), &may_set_status);
}

void fill_dict_slot(DictSlot& s, const dq_dict_column& d) {
    memset(&s, 0, sizeof(s));
    s.indices = d.indices;
    s.validity = (const uint64_t*)d.validity;
    s.dict_data = (const uint8_t*)d.dictionary.values;
    s.dict_offsets = d.dictionary.offsets;
    s.n_dict = (int32_t)(d.dictionary.length - 1);
}

// A plan slot and the addresses its indices name: zero block, where bitmaps per predicate.
DictSlot resolve_dict_slot(const DictPlanSlot& ps, const dq_dict_column& d, int64_t* zero, uint64_t* const* wt, uint64_t* const* wn) {
    DictSlot s;
    fill_dict_slot(s, d);
    s.flags = ps.flags;
    s.stats = zero + ps.stats;
    s.fold = zero + ps.fold;
    s.counts = zero + ps.counts;
    s.hll = (uint32_t*)(zero + ps.hll);
    s.where_t = ps.where >= 0 ? wt[ps.where] : nullptr;
    s.where_nn = ps.where >= 0 ? wn[ps.where] : nullptr;
    s.lds_copies = ps.lds_copies;
    return s;
}

// One dq_dict_scan call: its arguments, its plan (call_plans.h) and the per-call scratch the plan's indices resolve to.
struct DictCall {
    dq_ctx* ctx;
    const dq_column* columns;
    int ncols;
    const dq_dict_column* dicts;
    int64_t nrows;
    const dq_op* ops;
    int nops;
    const dq_predicate* preds;
    int npreds;
    int grid;
    DictPlan plan;
    ScratchBuffers buf;
    int64_t* zero = nullptr;  // one zeroed block: per slot stats, fold, counts, HLL registers, then the predicate ops' sums
    DictSlot* dslots = nullptr;
    DictPredOp* dpops = nullptr;
    DictOpMap* dops = nullptr;
    dq_state* dout = nullptr;
    PredColumn* pcols = nullptr;     // the plain columns, then each predicate op's single column: its slot's dictionary
    int32_t* status = nullptr;       // one word per predicate, then one per predicate op
    std::vector<uint64_t*> wt, wn;   // per predicate in use as a where: TRUE / NOT-NULL bitmaps over the rows
    std::vector<uint64_t*> pt, pn;   // per predicate op: the same over its dictionary's n_dict + 1 entries
    std::vector<PredColumn> pc;      // host copy of pcols
    std::vector<DictSlot> slots;     // host copy of dslots
    int nslots() const { return (int)plan.slots.size(); }
    int npops() const { return (int)plan.pops.size(); }
    const dq_column& pop_dictionary(int q) const { return dicts[plan.slots[plan.pops[q].slot].dict].dictionary; }
};

int alloc_dict_buffers(DictCall& dc) {
    dq_ctx* ctx = dc.ctx;
    ScratchBuffers& buf = dc.buf;
    const int nslots = dc.nslots(), npops = dc.npops(), nops = dc.nops, ncols = dc.ncols, npreds = dc.npreds;
    DQ_HIP(ctx, buf.alloc((void**)&dc.zero, dc.plan.zwords * 8));
    DQ_HIP(ctx, buf.alloc((void**)&dc.dslots, sizeof(DictSlot) * nslots));
    DQ_HIP(ctx, buf.alloc((void**)&dc.dpops, sizeof(DictPredOp) * std::max(npops, 1)));
    DQ_HIP(ctx, buf.alloc((void**)&dc.dops, sizeof(DictOpMap) * nops));
    DQ_HIP(ctx, buf.alloc((void**)&dc.dout, sizeof(dq_state) * nops));
    DQ_HIP(ctx, buf.alloc((void**)&dc.pcols, sizeof(PredColumn) * (size_t)(std::max(ncols, 1) + std::max(npops, 1))));
    DQ_HIP(ctx, buf.alloc((void**)&dc.status, sizeof(int32_t) * dc.plan.nstatus));
    const int64_t pwords = padded_words_for(dc.nrows);
    dc.wt.assign(std::max(npreds, 1), nullptr);
    dc.wn.assign(std::max(npreds, 1), nullptr);
    for (int p = 0; p < npreds; ++p) {
        if (!dc.plan.where_used[p]) continue;
        DQ_HIP(ctx, buf.alloc((void**)&dc.wt[p], (size_t)pwords * 8));
        DQ_HIP(ctx, buf.alloc((void**)&dc.wn[p], (size_t)pwords * 8));
    }
    dc.pt.assign(std::max(npops, 1), nullptr);
    dc.pn.assign(std::max(npops, 1), nullptr);
    for (int q = 0; q < npops; ++q) {
        const int64_t ew = padded_words_for((int64_t)dc.plan.slots[dc.plan.pops[q].slot].n_dict + 1);
        DQ_HIP(ctx, buf.alloc((void**)&dc.pt[q], (size_t)ew * 8));
        DQ_HIP(ctx, buf.alloc((void**)&dc.pn[q], (size_t)ew * 8));
    }
    return DQ_OK;
}

// The zeroed block and status words, the PredColumn records, then the where bitmaps over the plain columns.
int dict_where_bitmaps(DictCall& dc, Stager& up) {
    dq_ctx* ctx = dc.ctx;
    const int ncols = dc.ncols, npops = dc.npops();
    DQ_HIP(ctx, hipMemsetAsync(dc.zero, 0, dc.plan.zwords * 8, ctx->stream));
    DQ_HIP(ctx, hipMemsetAsync(dc.status, 0, sizeof(int32_t) * dc.plan.nstatus, ctx->stream));
    std::vector<PredColumn>& pc = dc.pc;
    pc.resize(std::max(ncols, 1) + std::max(npops, 1));
    memset(pc.data(), 0, sizeof(PredColumn) * pc.size());
    for (int c = 0; c < ncols; ++c) {
        if (!(dc.columns[c].flags & DQ_COL_DEVICE)) continue;  // unread (checked by the plan)
        pc[c] = pred_column(dc.columns[c], dc.columns[c].values, dc.columns[c].validity, dc.columns[c].offsets);
    }
    for (int q = 0; q < npops; ++q) {
        const dq_column& e = dc.pop_dictionary(q);
        PredColumn& pq = pc[std::max(ncols, 1) + q];
        pq.values = e.values;
        pq.validity = (const uint64_t*)e.validity;
        pq.offsets = e.offsets;
        pq.spark_type = DQ_TYPE_STRING;
        pq.elem = ET_NONE;
    }
    int rc = up.upload(dc.pcols, pc.data(), sizeof(PredColumn) * pc.size());
    for (int p = 0; p < dc.npreds && !rc; ++p) {
        if (!dc.plan.where_used[p]) continue;
        rc = dict_predicate(ctx, up, dc.buf, dc.preds[p], dc.columns, ncols, pc.data(), dc.pcols, dc.nrows, dc.wt[p], dc.wn[p],
                            dc.status + p);
    }
    return rc;
}

// The per-row pass: every slot in one launch.
int launch_dict_rows(DictCall& dc, Stager& up) {
    dq_ctx* ctx = dc.ctx;
    dc.slots.reserve(dc.nslots());
    for (const DictPlanSlot& ps : dc.plan.slots)
        dc.slots.push_back(resolve_dict_slot(ps, dc.dicts[ps.dict], dc.zero, dc.wt.data(), dc.wn.data()));
    const int rc = up.upload(dc.dslots, dc.slots.data(), sizeof(DictSlot) * dc.nslots());
    if (rc) return rc;
    launch_dict_counts(dc.dslots, dc.nslots(), dc.nrows, dc.grid, dc.plan.lds_words, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_DICT_COUNTS]++;
    return DQ_OK;
}

// Per entry: the predicate ops over their dictionaries, then the fold and the states.
int launch_dict_entries(DictCall& dc, Stager& up) {
    dq_ctx* ctx = dc.ctx;
    const int npops = dc.npops(), pc0 = std::max(dc.ncols, 1);
    std::vector<DictPredOp> pops(std::max(npops, 1));
    int rc;
    for (int q = 0; q < npops; ++q) {
        const dq_column& e = dc.pop_dictionary(q);
        rc = dict_predicate(ctx, up, dc.buf, dict_pop_predicate(dc.plan, q, dc.preds), &e, 1, dc.pc.data() + pc0 + q,
                            dc.pcols + pc0 + q, e.length, dc.pt[q], dc.pn[q], dc.status + std::max(dc.npreds, 1) + q);
        if (rc) return rc;
        pops[q] = DictPredOp{dc.pt[q], dc.pn[q], (unsigned long long*)(dc.zero + dc.plan.sums_off + 2 * (size_t)q),
                             dc.plan.pops[q].slot, 0};
    }
    std::vector<DictOpMap> opmap = dc.plan.opmap;
    for (int i = 0; i < dc.nops; ++i)
        if (dc.plan.op_pop[i] >= 0) opmap[i].sums = pops[dc.plan.op_pop[i]].sums;
    if (npops && (rc = up.upload(dc.dpops, pops.data(), sizeof(DictPredOp) * npops))) return rc;
    if ((rc = up.upload(dc.dops, opmap.data(), sizeof(DictOpMap) * dc.nops))) return rc;
    launch_dict_fold(dc.dslots, dc.nslots(), dc.plan.max_entries, dc.dpops, npops, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_DICT_FOLD]++;
    launch_dict_finalize(dc.dslots, dc.dops, dc.nops, dc.nrows, dc.dout, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    return DQ_OK;
}

// The states, the status words and every slot's row statistics; the states go to `out` only when nothing failed.
int dict_read_back(DictCall& dc, Stager& up, dq_state* out) {
    dq_ctx* ctx = dc.ctx;
    const int nslots = dc.nslots(), nstatus = dc.plan.nstatus;
    void *hout = nullptr, *hstatus_ = nullptr;
    int rc;
    if ((rc = up.download(&hout, dc.dout, sizeof(dq_state) * dc.nops))) return rc;
    if ((rc = up.download(&hstatus_, dc.status, sizeof(int32_t) * nstatus))) return rc;
    const int32_t* hstatus = (const int32_t*)hstatus_;
    int64_t* hstats = (int64_t*)up.take(sizeof(int64_t) * DS_COUNT * nslots);
    if (!hstats) return fail(ctx, DQ_ERR_DEVICE, "dq_dict_scan: pinned staging exhausted");
    for (int s = 0; s < nslots; ++s)
        DQ_HIP(ctx, hipMemcpyAsync(hstats + DS_COUNT * s, dc.slots[s].stats, sizeof(int64_t) * DS_COUNT, hipMemcpyDeviceToHost, ctx->stream));
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < nslots; ++s)
        if (hstats[DS_COUNT * s + DS_BAD_INDEX])
            return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dictionary column %d: %lld non-NULL rows hold an index outside [0, %d)",
                        dc.plan.slots[s].dict, (long long)hstats[DS_COUNT * s + DS_BAD_INDEX], dc.slots[s].n_dict);
    for (int k = 0; k < nstatus; ++k)
        if (hstatus[k] & 1) return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_dict_scan: regex backtracking limit exceeded");
    for (int k = 0; k < nstatus; ++k)
        if (hstatus[k])
            return fail(ctx, DQ_ERR_UNSUPPORTED,
                        "dq_dict_scan: a string needs Double.parseDouble's arbitrary-precision path "
                        "(hexadecimal literal, or > 19 significant digits on a rounding boundary)");
    memcpy(out, hout, sizeof(dq_state) * dc.nops);
    return DQ_OK;
}

}  // namespace

extern "C" {

int dq_dict_counts(dq_ctx* ctx, const dq_dict_column* dict, int64_t* counts_dev, int64_t* rows) {
    if (!ctx || !dict || !rows) return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_dict_counts: invalid arguments");
    ctx->err.clear();
    if (!ctx->subs.empty()) return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_dict_counts takes a single-device context");
    const int64_t nrows = dict->length;
    std::string msg;
    const int rc = check_dict_column(*dict, nrows, 0, &msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    DictSlot s;
    fill_dict_slot(s, *dict);
    if ((s.n_dict > 0 && !counts_dev) || ((uintptr_t)counts_dev & 7))
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_dict_counts: counts_dev holds n_dict 8-byte aligned counts");
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    ScratchBuffers buf(ctx);
    int64_t* stats = nullptr;
    DictSlot* dslot = nullptr;
    DQ_HIP(ctx, buf.alloc((void**)&stats, sizeof(int64_t) * DS_COUNT));
    DQ_HIP(ctx, buf.alloc((void**)&dslot, sizeof(DictSlot)));
    const int grid = dict_counts_grid(ctx->cus, nrows);
    s.counts = counts_dev;
    s.stats = stats;
    s.lds_copies = dict_lds_copies(dict_options(), s.n_dict, nrows, grid);
    DQ_HIP(ctx, hipMemsetAsync(stats, 0, sizeof(int64_t) * DS_COUNT, ctx->stream));
    if (s.n_dict > 0) DQ_HIP(ctx, hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * (size_t)s.n_dict, ctx->stream));
    DQ_HIP(ctx, hipMemcpyAsync(dslot, &s, sizeof(s), hipMemcpyHostToDevice, ctx->stream));
    launch_dict_counts(dslot, 1, nrows, grid, s.lds_copies * s.n_dict, ctx->stream);
    DQ_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_DICT_COUNTS]++;
    int64_t h[DS_COUNT];
    DQ_HIP(ctx, hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h[DS_BAD_INDEX])
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_dict_counts: %lld non-NULL rows hold an index outside [0, %d)",
                    (long long)h[DS_BAD_INDEX], s.n_dict);
    rows[0] = nrows;
    rows[1] = h[DS_NONNULL];
    return DQ_OK;
}

int dq_dict_scan(dq_ctx* ctx, const dq_column* columns, int ncols, const dq_dict_column* dicts, int ndicts, int64_t nrows,
                 const dq_op* ops, int nops, const dq_predicate* preds, int npreds, dq_state* out) {
    if (!ctx) return DQ_ERR_INVALID_ARGUMENT;
    ctx->err.clear();
    if (nops < 0 || ncols < 0 || ndicts < 0 || npreds < 0 || nrows < 0 || (nops > 0 && (!ops || !out || !dicts)) ||
        (ncols > 0 && !columns) || (npreds > 0 && !preds))
        return fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_dict_scan: invalid arguments");
    if (nops == 0) return DQ_OK;
    if (!ctx->subs.empty()) return fail(ctx, DQ_ERR_UNSUPPORTED, "dq_dict_scan takes a single-device context");
    // checks, slots, predicate ops, zero-block layout and staging size: pure host (call_plans.cpp)
    DictCall dc{ctx, columns, ncols, dicts, nrows, ops, nops, preds, npreds, dict_counts_grid(ctx->cus, nrows), {}, ScratchBuffers(ctx)};
    std::string msg;
    int rc = plan_dict_scan(columns, ncols, dicts, ndicts, nrows, ops, nops, preds, npreds, dict_options(), dc.grid, &dc.plan, &msg);
    if (rc) return fail(ctx, rc, "%s", msg.c_str());
    DQ_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = alloc_dict_buffers(dc))) return rc;
    if ((rc = ensure_pinned(ctx, dc.plan.pinned_bytes))) return rc;
    DQ_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the pinned buffer may still feed a previous call's copies
    Stager up{ctx};
    if ((rc = dict_where_bitmaps(dc, up))) return rc;
    if ((rc = launch_dict_rows(dc, up))) return rc;
    if ((rc = launch_dict_entries(dc, up))) return rc;
    return dict_read_back(dc, up, out);
}

}  // extern "C"
