// schema.hip — RowLevelSchemaValidator on gfx950: one fused verdict pass over the text columns and a row compaction.
//
// Replaces schema/RowLevelSchemaValidator.scala:183-281 (the CNF column + persist, the cast of the valid rows, the
// filter of the invalid rows: three passes in Spark). schema_verdict_kernel evaluates every column definition for a
// row tile in one launch: one lane per row, each wave's 64 strings of a column staged in LDS by coalesced dword loads
// (as cast.hip does), the clauses folded with SQL's three-valued AND into one TRUE / FALSE / NULL verdict per row, the
// int / decimal / timestamp casts written in the same pass. A wave ballot gives one 64-bit word of each bitmap per 64
// rows; the row counts are popcounts, reduced per block and added with one atomic per counter per block.
// dq_gather_rows compacts one column under a selection bitmap: word popcounts -> exclusive scan (rocPRIM) -> source
// row index -> gathers (fixed width; strings: lengths, scan to offsets, wave-cooperative byte copy).
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "dq_common.h"
#include "dq_device.h"
#include "dq_internal.h"
#include "dq_schema_parse.h"
#include "rx_engine.h"

namespace dq {

constexpr int kSchemaBlock = 256;

struct SchemaDef {
    const uint8_t* bytes;
    const int32_t* offsets;
    const uint64_t* validity;    // nullptr = all valid
    const void* prog;            // regex image (int32 words) or compiled mask (bytes), device memory
    void* cast_values;           // INT: int32, DECIMAL / TIMESTAMP: int64 per row; nullptr = not wanted
    uint64_t* cast_validity;
    int64_t minv, maxv;          // STRING: character counts, INT: value bounds
    int32_t kind, nullable, has_min, has_max, precision, scale, prog_len, pad;
};

struct SchemaCounters {
    unsigned long long n[4];     // TRUE, FALSE, NULL verdicts, rows with an ambiguous cell
    int32_t first_ambiguous;     // lowest definition index with an ambiguous cell
    int32_t rx_status;           // a regex ran out of its backtracking budget
};

template <bool RX>
__global__ void __launch_bounds__(kSchemaBlock) __attribute__((amdgpu_waves_per_eu(7, 8)))
schema_verdict_kernel(const SchemaDef* __restrict__ defs, int ndefs, int64_t nrows, uint64_t* __restrict__ true_bits,
                      uint64_t* __restrict__ false_bits, uint64_t* __restrict__ amb_bits, SchemaCounters* counters) {
    __shared__ uint32_t stage[kSchemaBlock / 64][kStageWords];
    __shared__ unsigned long long wcnt[kSchemaBlock / 64][4];
    const int64_t stride = (int64_t)gridDim.x * kSchemaBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 4) wcnt[wave][lane] = 0;  // the wave's TRUE / FALSE / NULL / ambiguous rows, kept in LDS (lane 0 adds)
    for (int64_t base = (int64_t)blockIdx.x * kSchemaBlock; base < nrows; base += stride) {
        const int64_t w0 = base + 64 * wave;
        if (w0 >= nrows) continue;  // wave-uniform
        const int64_t wl = w0 + 64 < nrows ? w0 + 64 : nrows;
        const uint32_t r = (uint32_t)base + threadIdx.x;  // nrows < 2^31 (checked by the host)
        const bool rin = r < (uint32_t)nrows;
        bool f = false, u = false, amb = false;
        for (int d = 0; d < ndefs; ++d) {
            const SchemaDef D = defs[d];
            const bool rvalid = rin && row_valid(D.validity, r);
            int32_t ro = 0, rlen = 0;
            if (rin) {
                ro = D.offsets[r];
                rlen = D.offsets[r + 1] - ro;
            }
            int64_t a0;
            const uint8_t* sbase = stage_wave_bytes(stage[wave], D.bytes, D.offsets, w0, wl, lane, a0);
            const uint8_t* s = sbase ? sbase + (ro - a0) : D.bytes + ro;
            if (!D.nullable && rin && !rvalid) f = true;
            bool ok = false, a = false;
            int32_t v32 = 0;
            int64_t v64 = 0;
            switch (D.kind) {
                case DQ_SCHEMA_STRING:
                    if (rvalid) {
                        if (D.has_min || D.has_max) {
                            const int len = utf8_chars(s, rlen);
                            if (D.has_min && len < D.minv) f = true;
                            if (D.has_max && len > D.maxv) f = true;
                        }
                        if (RX && D.prog_len > 0 && !f) {  // only lanes not already FALSE run the matcher
                            const rx::RxProg p = rx::rx_program(static_cast<const int32_t*>(D.prog));
                            uint64_t stk[rx::kRxStack];
                            int start;
                            const int end = rx::rx_find(p, s, rlen, stk, start);
                            if (end == -2) atomicOr(&counters->rx_status, 1);
                            if (end <= start) f = true;  // the first match must be non-empty
                        }
                    }
                    break;
                case DQ_SCHEMA_INT:
                    if (rvalid) {
                        ok = spark_string_to_int(s, rlen, v32);
                        if (!ok) f = true;
                        else if ((D.has_max && v32 > D.maxv) || (D.has_min && v32 < D.minv)) f = true;
                    } else if (rin && D.has_min) {
                        u = true;  // `colIsNull.isNull or cast >= min` is FALSE OR NULL for a NULL cell (:246)
                    }
                    break;
                case DQ_SCHEMA_DECIMAL:
                    if (rvalid) {
                        ok = spark_string_to_decimal(s, rlen, D.precision, D.scale, v64, a);
                        if (!ok) f = true;
                    }
                    break;
                default:  // DQ_SCHEMA_TIMESTAMP
                    if (rvalid) {
                        ok = parse_timestamp_mask(static_cast<const uint8_t*>(D.prog), D.prog_len, s, rlen, v64, a);
                        if (!ok) f = true;
                    }
                    break;
            }
            if (D.kind != DQ_SCHEMA_STRING) {
                if (D.cast_values && rin) {
                    if (D.kind == DQ_SCHEMA_INT) static_cast<int32_t*>(D.cast_values)[r] = ok ? v32 : 0;
                    else static_cast<int64_t*>(D.cast_values)[r] = ok ? v64 : 0;
                }
                const unsigned long long okb = __ballot(ok);
                if (lane == 0 && D.cast_validity) D.cast_validity[w0 >> 6] = okb;
                const unsigned long long ab = __ballot(a);
                if (ab != 0ull && lane == 0) atomicMin(&counters->first_ambiguous, d);
                amb |= a;
            }
            __builtin_amdgcn_wave_barrier();  // every lane done with the stage before the next column's bytes
        }
        const unsigned long long bt = __ballot(rin && !f && !u);
        const unsigned long long bf = __ballot(rin && f);
        const unsigned long long bu = __ballot(rin && !f && u);
        const unsigned long long ba = __ballot(rin && amb);
        if (lane == 0) {
            if (true_bits) true_bits[w0 >> 6] = bt;
            if (false_bits) false_bits[w0 >> 6] = bf;
            if (amb_bits) amb_bits[w0 >> 6] = ba;
            wcnt[wave][0] += __popcll(bt);
            wcnt[wave][1] += __popcll(bf);
            wcnt[wave][2] += __popcll(bu);
            wcnt[wave][3] += __popcll(ba);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0;
        for (int w = 0; w < kSchemaBlock / 64; ++w) t += wcnt[w][threadIdx.x];
        if (t) atomicAdd(&counters->n[threadIdx.x], t);
    }
}

// ---- compaction -------------------------------------------------------------------------------------------------------
// pc[w] = selected rows of word w (bits past nrows ignored), pc[nwords] = 0 so that the exclusive scan's last entry
// is the total.
__global__ void __launch_bounds__(256)
select_popc_kernel(const uint64_t* __restrict__ sel, int64_t nrows, int64_t nwords, uint32_t* __restrict__ pc) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > nwords) return;
    uint64_t x = 0;
    if (w < nwords) {
        x = sel[w];
        const int64_t rem = nrows - w * 64;
        if (rem < 64) x &= (1ull << rem) - 1ull;
    }
    pc[w] = (uint32_t)__popcll(x);
}

// idx[k] = the k-th selected row.
__global__ void __launch_bounds__(256)
select_index_kernel(const uint64_t* __restrict__ sel, int64_t nrows, const uint32_t* __restrict__ wbase,
                    int32_t* __restrict__ idx) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint64_t x = sel[r >> 6];
    const int b = (int)(r & 63);
    if ((x >> b) & 1ull) idx[wbase[r >> 6] + (uint32_t)__popcll(x & ((1ull << b) - 1ull))] = (int32_t)r;
}

// One thread per output row: the value and (ballot) the compacted validity word.
template <typename T>
__global__ void __launch_bounds__(256)
gather_fixed_kernel(const T* __restrict__ in, const uint64_t* __restrict__ in_valid, const int32_t* __restrict__ idx,
                    int64_t nsel, T* __restrict__ out, uint64_t* __restrict__ out_valid) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool v = false;
    if (k < nsel) {
        const int64_t r = idx[k];
        out[k] = in[r];
        v = row_valid(in_valid, r);
    }
    const unsigned long long b = __ballot(v);
    if ((threadIdx.x & 63) == 0 && out_valid && (k & ~(int64_t)63) < nsel) out_valid[k >> 6] = b;
}

// Strings, step 1: lens[k] = byte length of the k-th selected row (lens[nsel] = 0), and the compacted validity.
__global__ void __launch_bounds__(256)
gather_lengths_kernel(const int32_t* __restrict__ offsets, const uint64_t* __restrict__ in_valid,
                      const int32_t* __restrict__ idx, int64_t nsel, int32_t* __restrict__ lens,
                      uint64_t* __restrict__ out_valid) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool v = false;
    if (k < nsel) {
        const int64_t r = idx[k];
        lens[k] = offsets[r + 1] - offsets[r];
        v = row_valid(in_valid, r);
    } else if (k == nsel) {
        lens[k] = 0;
    }
    const unsigned long long b = __ballot(v);
    if ((threadIdx.x & 63) == 0 && out_valid && (k & ~(int64_t)63) < nsel) out_valid[k >> 6] = b;
}

// Strings, step 3: each wave copies the bytes of 64 consecutive output rows, a contiguous destination range: the lanes
// walk the destination bytes (coalesced stores) and find each byte's row by a search of the group's 65 offsets in LDS.
__global__ void __launch_bounds__(256)
gather_bytes_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ in_offsets,
                    const int32_t* __restrict__ idx, const int32_t* __restrict__ out_offsets, int64_t nsel,
                    uint8_t* __restrict__ out) {
    __shared__ int32_t s_dst[4][65];
    __shared__ int32_t s_src[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
    const int cnt = g0 < nsel ? (nsel - g0 < 64 ? (int)(nsel - g0) : 64) : 0;
    if (lane < cnt) {
        s_dst[wave][lane] = out_offsets[g0 + lane];
        s_src[wave][lane] = in_offsets[idx[g0 + lane]];
    }
    if (lane == 0 && cnt > 0) s_dst[wave][cnt] = out_offsets[g0 + cnt];
    __syncthreads();
    if (cnt == 0) return;
    const int32_t d0 = s_dst[wave][0], d1 = s_dst[wave][cnt];
    for (int32_t b = d0 + lane; b < d1; b += 64) {
        int lo = 0, hi = cnt - 1;  // the last row j with s_dst[j] <= b (its successor starts past b: it holds b)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_dst[wave][mid] <= b) lo = mid; else hi = mid - 1;
        }
        out[b] = in[s_src[wave][lo] + (b - s_dst[wave][lo])];
    }
    if (g0 + cnt == nsel && lane < 16) out[d1 + lane] = 0;  // the read-past padding of the dword loads
}

// Decode of a dictionary-encoded column, step 1: the source entry of every row (0 for a NULL row or an index outside
// the dictionary, which is counted in *bad) and its byte length (0 for those rows; lens[nrows] = 0). Steps 2 and 3 are
// the string gather's: an exclusive scan into offsets and gather_bytes_kernel with the entries as the source rows.
__global__ void __launch_bounds__(256)
dict_lengths_kernel(const int32_t* __restrict__ indices, const uint64_t* __restrict__ valid, const int32_t* __restrict__ dict_offsets,
                    int32_t n_dict, int64_t nrows, int32_t* __restrict__ src, int64_t* __restrict__ lens,
                    unsigned long long* __restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nrows) return;
    int64_t len = 0;
    if (k < nrows) {
        const bool on = row_valid(valid, k);
        const int32_t e = indices[k];
        const bool ok = on && (uint32_t)e < (uint32_t)n_dict;
        if (on && !ok) atomicAdd(bad, 1ull);
        src[k] = ok ? e : 0;
        len = ok ? dict_offsets[e + 1] - dict_offsets[e] : 0;
    }
    lens[k] = len;
}

__global__ void __launch_bounds__(256)
narrow_offsets_kernel(const int64_t* __restrict__ wide, int64_t n, int32_t* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = (int32_t)wide[k];
}

}  // namespace dq

namespace {

int blocks_of(int64_t n) { return (int)std::max<int64_t>(1, (n + 255) / 256); }
}  // namespace

extern "C" {

int dq_schema_validate(dq_ctx* ctx, const dq_column* columns, int ncols, int64_t nrows, const dq_schema_column* defs,
                       int ndefs, uint32_t flags, uint8_t* true_bits, uint8_t* false_bits, uint8_t* ambiguous_bits,
                       dq_schema_result* result) {
    if (!ctx || !result || nrows < 0 || ncols < 0 || ndefs < 0 || (ncols > 0 && !columns) || (ndefs > 0 && !defs))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: invalid arguments");
    memset(result, 0, sizeof(*result));
    result->first_ambiguous_column = -1;
    if (dq::ctx_num_subs(ctx) != 0)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_schema_validate: multi-device contexts are not supported");
    if (nrows > INT32_MAX)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_schema_validate: more than 2^31 - 1 rows (validate in chunks)");
    if (((uintptr_t)true_bits | (uintptr_t)false_bits | (uintptr_t)ambiguous_bits) & 7)
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_schema_validate: bitmaps must be 8-B aligned");
    std::vector<dq::SchemaDef> hd((size_t)ndefs);
    std::vector<uint8_t> progs;
    std::vector<size_t> prog_at((size_t)ndefs, 0);
    bool any_rx = false;
    for (int d = 0; d < ndefs; ++d) {
        const dq_schema_column& sc = defs[d];
        if (sc.column < 0 || sc.column >= ncols)
            return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: column index out of range");
        const dq_column& c = columns[sc.column];
        if (c.spark_type != DQ_TYPE_STRING || !c.offsets || c.length != nrows)
            return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: a schema column must be a STRING column of nrows rows");
        if (!(c.flags & DQ_COL_DEVICE) || (c.flags & DQ_COL_OFFSETS64))
            return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_schema_validate: columns must be device-resident with int32 offsets");
        if (((uintptr_t)c.values & 3) || ((uintptr_t)c.validity & 7) || ((uintptr_t)sc.cast_values & 7) ||
            ((uintptr_t)sc.cast_validity & 7))
            return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_schema_validate: misaligned column or cast buffer");
        if (sc.program_len < 0 || (sc.program_len > 0 && !sc.program))
            return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: bad program");
        dq::SchemaDef& D = hd[d];
        memset(&D, 0, sizeof(D));
        D.bytes = (const uint8_t*)c.values;
        D.offsets = c.offsets;
        D.validity = (const uint64_t*)c.validity;
        D.cast_values = sc.cast_values;
        D.cast_validity = (uint64_t*)sc.cast_validity;
        D.kind = sc.kind;
        D.nullable = sc.nullable ? 1 : 0;
        D.has_min = sc.has_min ? 1 : 0;
        D.has_max = sc.has_max ? 1 : 0;
        D.minv = sc.min_value;
        D.maxv = sc.max_value;
        D.precision = sc.precision;
        D.scale = sc.scale;
        D.prog_len = sc.program_len;
        switch (sc.kind) {
            case DQ_SCHEMA_STRING:
                if (sc.program_len > 0) {
                    if (!dq::rx::rx_image_ok(sc.program, sc.program_len))
                        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: malformed regex program");
                    any_rx = true;
                }
                break;
            case DQ_SCHEMA_INT:
                if ((sc.has_min && (sc.min_value < INT32_MIN || sc.min_value > INT32_MAX)) ||
                    (sc.has_max && (sc.max_value < INT32_MIN || sc.max_value > INT32_MAX)))
                    return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: int bounds must fit int32");
                D.prog_len = 0;
                break;
            case DQ_SCHEMA_DECIMAL:
                if (sc.scale < 0 || sc.scale > sc.precision || sc.precision > 18)
                    return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_schema_validate: decimal needs 0 <= scale <= precision <= 18");
                D.prog_len = 0;
                break;
            case DQ_SCHEMA_TIMESTAMP:
                if (!dq::mask_program_ok((const uint8_t*)sc.program, sc.program_len))
                    return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: malformed timestamp mask program");
                break;
            default:
                return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_schema_validate: unknown definition kind");
        }
        if (D.prog_len > 0) {
            prog_at[d] = (progs.size() + 7) & ~(size_t)7;
            progs.resize(prog_at[d] + (size_t)D.prog_len);
            memcpy(progs.data() + prog_at[d], sc.program, (size_t)D.prog_len);
        }
    }
    if (nrows == 0 || ndefs == 0) {
        // no definition: every row is TRUE (the fold starts from `true`)
        if (ndefs == 0 && nrows > 0) {
            DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
            hipStream_t s0 = dq::ctx_stream(ctx);
            const size_t bb = (size_t)(nrows + 63) / 64 * 8;
            if (true_bits) DQ_CTX_HIP(ctx, hipMemsetAsync(true_bits, 0xFF, bb, s0));
            if (false_bits) DQ_CTX_HIP(ctx, hipMemsetAsync(false_bits, 0, bb, s0));
            if (ambiguous_bits) DQ_CTX_HIP(ctx, hipMemsetAsync(ambiguous_bits, 0, bb, s0));
            DQ_CTX_HIP(ctx, hipStreamSynchronize(s0));
            result->num_valid = nrows;
        }
        return DQ_OK;
    }
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    uint8_t* dprogs = nullptr;
    if (!progs.empty()) {
        DQ_CTX_HIP(ctx, buf.alloc((void**)&dprogs, progs.size()));
        DQ_CTX_HIP(ctx, hipMemcpyAsync(dprogs, progs.data(), progs.size(), hipMemcpyHostToDevice, s));
        for (int d = 0; d < ndefs; ++d)
            if (hd[d].prog_len > 0) hd[d].prog = dprogs + prog_at[d];
    }
    dq::SchemaDef* ddefs = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&ddefs, sizeof(dq::SchemaDef) * (size_t)ndefs));
    DQ_CTX_HIP(ctx, hipMemcpyAsync(ddefs, hd.data(), sizeof(dq::SchemaDef) * (size_t)ndefs, hipMemcpyHostToDevice, s));
    dq::SchemaCounters hc;
    memset(&hc, 0, sizeof(hc));
    hc.first_ambiguous = INT_MAX;
    dq::SchemaCounters* dc = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&dc, sizeof(hc)));
    DQ_CTX_HIP(ctx, hipMemcpyAsync(dc, &hc, sizeof(hc), hipMemcpyHostToDevice, s));
    // persistent workgroups, exactly as many as are resident at once: the rows of a tile cost very different amounts
    // (a regex against a NULL cell), so a partial second round of workgroups would leave CUs idle at the end
    const int64_t blocks = (nrows + dq::kSchemaBlock - 1) / dq::kSchemaBlock;
    auto kernel = any_rx ? dq::schema_verdict_kernel<true> : dq::schema_verdict_kernel<false>;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, dq::kSchemaBlock, 0) != hipSuccess || per_cu < 1)
        per_cu = 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)dq::ctx_cus(ctx) * per_cu));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(dq::kSchemaBlock), 0, s, ddefs, ndefs, nrows, (uint64_t*)true_bits,
                       (uint64_t*)false_bits, (uint64_t*)ambiguous_bits, dc);
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->schema_launches++;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&hc, dc, sizeof(hc), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    result->num_valid = (int64_t)hc.n[0];
    result->num_invalid = (int64_t)hc.n[1];
    result->num_unknown = (int64_t)hc.n[2];
    result->num_ambiguous = (int64_t)hc.n[3];
    result->first_ambiguous_column = hc.n[3] ? defs[hc.first_ambiguous].column : -1;
    if (hc.rx_status)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_schema_validate: a value exceeded the regex backtracking budget");
    if (hc.n[3] && !(flags & DQ_SCHEMA_AMBIGUOUS_NULL)) {
        char msg[256];
        snprintf(msg, sizeof(msg),
                 "dq_schema_validate: %lld rows hold a cell whose JVM parse is ambiguous (first in column %d); "
                 "pass DQ_SCHEMA_AMBIGUOUS_NULL to cast such cells to NULL",
                 (long long)hc.n[3], (int)result->first_ambiguous_column);
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, msg);
    }
    return DQ_OK;
}

int64_t dq_schema_launch_count(const dq_ctx* ctx) { return ctx ? ctx->schema_launches : -1; }

int dq_gather_rows(dq_ctx* ctx, const dq_column* column, int64_t nrows, const uint8_t* select_bits, int64_t nselected,
                   void* out_values, uint8_t* out_validity, int32_t* out_offsets, int64_t* out_bytes) {
    if (!ctx || !column || nrows < 0 || nselected < 0 || nselected > nrows || column->length != nrows ||
        (nrows > 0 && !select_bits))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_gather_rows: invalid arguments");
    if (dq::ctx_num_subs(ctx) != 0)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_gather_rows: multi-device contexts are not supported");
    if (nrows > INT32_MAX) return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_gather_rows: more than 2^31 - 1 rows");
    const bool is_string = column->spark_type == DQ_TYPE_STRING;
    if (!(column->flags & DQ_COL_DEVICE) || (column->flags & DQ_COL_OFFSETS64))
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_gather_rows: the column must be device-resident with int32 offsets");
    const int esize = is_string ? 1 : dq::elem_size(dq::elem_of(column->spark_type));
    if (esize == 0) return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_gather_rows: unknown column type");
    if (is_string && (!column->offsets || !out_offsets || !out_bytes))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_gather_rows: a string gather needs offsets and out_bytes");
    if (!is_string && nselected > 0 && !out_values)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_gather_rows: no output buffer");
    if (((uintptr_t)select_bits & 7) || ((uintptr_t)out_validity & 7) || ((uintptr_t)column->validity & 7) ||
        (!is_string && (((uintptr_t)out_values | (uintptr_t)column->values) & (uintptr_t)(esize - 1))))
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_gather_rows: misaligned buffer");
    if (out_bytes) *out_bytes = 0;
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    const int64_t nwords = (nrows + 63) / 64;
    uint32_t *pc = nullptr, *wbase = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&pc, sizeof(uint32_t) * (size_t)(nwords + 1)));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&wbase, sizeof(uint32_t) * (size_t)(nwords + 1)));
    hipLaunchKernelGGL(dq::select_popc_kernel, dim3(blocks_of(nwords + 1)), dim3(256), 0, s, (const uint64_t*)select_bits,
                       nrows, nwords, pc);
    DQ_CTX_HIP(ctx, hipGetLastError());
    size_t tb = 0;
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, pc, wbase, 0u, (size_t)(nwords + 1), rocprim::plus<uint32_t>(), s));
    void* tmp = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc(&tmp, tb));
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(tmp, tb, pc, wbase, 0u, (size_t)(nwords + 1), rocprim::plus<uint32_t>(), s));
    uint32_t total = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&total, wbase + nwords, sizeof(total), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    if ((int64_t)total != nselected)  // the output buffers were sized for nselected rows
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_gather_rows: nselected differs from the bitmap's set bits");
    if (nselected == 0) {
        if (is_string) {
            DQ_CTX_HIP(ctx, hipMemsetAsync(out_offsets, 0, sizeof(int32_t), s));
            if (out_values) DQ_CTX_HIP(ctx, hipMemsetAsync(out_values, 0, 16, s));
            DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        }
        return DQ_OK;
    }
    int32_t* idx = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&idx, sizeof(int32_t) * (size_t)nselected));
    hipLaunchKernelGGL(dq::select_index_kernel, dim3(blocks_of(nrows)), dim3(256), 0, s, (const uint64_t*)select_bits, nrows,
                       wbase, idx);
    DQ_CTX_HIP(ctx, hipGetLastError());
    const uint64_t* iv = (const uint64_t*)column->validity;
    uint64_t* ov = (uint64_t*)out_validity;
    if (!is_string) {
        const dim3 g(blocks_of(nselected)), b(256);
        switch (esize) {
            case 1: hipLaunchKernelGGL(dq::gather_fixed_kernel<uint8_t>, g, b, 0, s, (const uint8_t*)column->values, iv, idx, nselected, (uint8_t*)out_values, ov); break;
            case 2: hipLaunchKernelGGL(dq::gather_fixed_kernel<uint16_t>, g, b, 0, s, (const uint16_t*)column->values, iv, idx, nselected, (uint16_t*)out_values, ov); break;
            case 4: hipLaunchKernelGGL(dq::gather_fixed_kernel<uint32_t>, g, b, 0, s, (const uint32_t*)column->values, iv, idx, nselected, (uint32_t*)out_values, ov); break;
            default: hipLaunchKernelGGL(dq::gather_fixed_kernel<uint64_t>, g, b, 0, s, (const uint64_t*)column->values, iv, idx, nselected, (uint64_t*)out_values, ov); break;
        }
        DQ_CTX_HIP(ctx, hipGetLastError());
        DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        return DQ_OK;
    }
    if (!out_values) {  // sizing call: offsets, validity, total bytes
        int32_t* lens = nullptr;
        DQ_CTX_HIP(ctx, buf.alloc((void**)&lens, sizeof(int32_t) * (size_t)(nselected + 1)));
        hipLaunchKernelGGL(dq::gather_lengths_kernel, dim3(blocks_of(nselected + 1)), dim3(256), 0, s, column->offsets, iv, idx,
                           nselected, lens, ov);
        DQ_CTX_HIP(ctx, hipGetLastError());
        size_t tb2 = 0;
        DQ_CTX_HIP(ctx, rocprim::exclusive_scan(nullptr, tb2, lens, out_offsets, 0, (size_t)(nselected + 1), rocprim::plus<int32_t>(), s));
        void* tmp2 = nullptr;
        DQ_CTX_HIP(ctx, buf.alloc(&tmp2, tb2));
        DQ_CTX_HIP(ctx, rocprim::exclusive_scan(tmp2, tb2, lens, out_offsets, 0, (size_t)(nselected + 1), rocprim::plus<int32_t>(), s));
        int32_t bytes = 0;
        DQ_CTX_HIP(ctx, hipMemcpyAsync(&bytes, out_offsets + nselected, sizeof(bytes), hipMemcpyDeviceToHost, s));
        DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        *out_bytes = bytes;
        return DQ_OK;
    }
    // copy call: out_offsets holds the sizing call's offsets; out_values has their total + 16 bytes
    hipLaunchKernelGGL(dq::gather_bytes_kernel, dim3((unsigned)((nselected + 255) / 256)), dim3(256), 0, s,
                       (const uint8_t*)column->values, column->offsets, idx, out_offsets, nselected, (uint8_t*)out_values);
    DQ_CTX_HIP(ctx, hipGetLastError());
    int32_t bytes = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&bytes, out_offsets + nselected, sizeof(bytes), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    *out_bytes = bytes;
    return DQ_OK;
}

int dq_dict_decode(dq_ctx* ctx, const dq_dict_column* dict, int32_t* out_offsets, void* out_values, int64_t* out_bytes) {
    if (!ctx || !dict || !out_offsets || !out_bytes || dict->length < 0)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: invalid arguments");
    if (dq::ctx_num_subs(ctx) != 0)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_dict_decode: multi-device contexts are not supported");
    const dq_column& e = dict->dictionary;
    const int64_t nrows = dict->length;
    if (!(dict->flags & DQ_COL_DEVICE) || !(e.flags & DQ_COL_DEVICE) || (e.flags & DQ_COL_OFFSETS64))
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_dict_decode: device buffers with int32 offsets only");
    if (e.spark_type != DQ_TYPE_STRING || e.length < 1 || e.length > INT32_MAX - 1 || !e.offsets || !e.values ||
        (nrows > 0 && !dict->indices))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: the dictionary is a STRING column of n_dict + 1 entries");
    if (nrows > INT32_MAX) return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_dict_decode: more than 2^31 - 1 rows");
    if (((uintptr_t)dict->indices & 3) || ((uintptr_t)dict->validity & 7) || ((uintptr_t)out_offsets & 3))
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_dict_decode: misaligned buffer");
    const int32_t n_dict = (int32_t)(e.length - 1);
    *out_bytes = 0;
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    int32_t* src = nullptr;
    int64_t *lens = nullptr, *wide = nullptr;
    unsigned long long* bad = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&src, sizeof(int32_t) * (size_t)std::max<int64_t>(nrows, 1)));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&lens, sizeof(int64_t) * (size_t)(nrows + 1)));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&wide, sizeof(int64_t) * (size_t)(nrows + 1)));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&bad, sizeof(unsigned long long)));
    DQ_CTX_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(dq::dict_lengths_kernel, dim3(blocks_of(nrows + 1)), dim3(256), 0, s, dict->indices,
                       (const uint64_t*)dict->validity, e.offsets, n_dict, nrows, src, lens, bad);
    DQ_CTX_HIP(ctx, hipGetLastError());
    size_t tb = 0;
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, lens, wide, (int64_t)0, (size_t)(nrows + 1), rocprim::plus<int64_t>(), s));
    void* tmp = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc(&tmp, tb));
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(tmp, tb, lens, wide, (int64_t)0, (size_t)(nrows + 1), rocprim::plus<int64_t>(), s));
    int64_t total = 0;
    unsigned long long nbad = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&total, wide + nrows, sizeof(total), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&nbad, bad, sizeof(nbad), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    if (nbad) {
        char msg[160];
        snprintf(msg, sizeof(msg), "dq_dict_decode: %llu non-NULL rows hold an index outside [0, %d)", nbad, n_dict);
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, msg);
    }
    if (total >= ((int64_t)1 << 31)) {
        char msg[200];
        snprintf(msg, sizeof(msg), "dq_dict_decode: the decoded strings hold %lld bytes, past the int32 offsets of one "
                 "column (2^31): keep the column encoded or split the rows", (long long)total);
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, msg);
    }
    *out_bytes = total;
    if (!out_values) {  // sizing call: the offsets
        hipLaunchKernelGGL(dq::narrow_offsets_kernel, dim3(blocks_of(nrows + 1)), dim3(256), 0, s, wide, nrows + 1, out_offsets);
        DQ_CTX_HIP(ctx, hipGetLastError());
        DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        return DQ_OK;
    }
    // copy call: out_offsets holds the sizing call's offsets; out_values has their total + 16 bytes
    if (nrows == 0) {
        DQ_CTX_HIP(ctx, hipMemsetAsync(out_values, 0, 16, s));
    } else {
        hipLaunchKernelGGL(dq::gather_bytes_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s,
                           (const uint8_t*)e.values, e.offsets, src, out_offsets, nrows, (uint8_t*)out_values);
        DQ_CTX_HIP(ctx, hipGetLastError());
    }
    ctx->kernel_launches[DQ_KERNEL_DICT_DECODE]++;
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    return DQ_OK;
}

// Host-only entries (no context, no device): the header's parsers for one cell. Return 1 = value, 0 = NULL,
// 2 = ambiguous.
int dq_parse_int32(const uint8_t* s, int32_t n, int32_t* out) {
    int32_t v = 0;
    if (n < 0 || (n > 0 && !s) || !dq::spark_string_to_int(s, n, v)) return 0;
    if (out) *out = v;
    return 1;
}

int dq_parse_decimal(const uint8_t* s, int32_t n, int32_t precision, int32_t scale, int64_t* out) {
    if (n < 0 || (n > 0 && !s) || scale < 0 || scale > precision || precision > 18) return 0;
    int64_t v = 0;
    bool amb = false;
    if (!dq::spark_string_to_decimal(s, n, precision, scale, v, amb)) return amb ? 2 : 0;
    if (out) *out = v;
    return 1;
}

int dq_parse_timestamp(const uint8_t* program, int32_t program_len, const uint8_t* s, int32_t n, int64_t* out) {
    if (n < 0 || (n > 0 && !s) || !dq::mask_program_ok(program, program_len)) return 0;
    int64_t v = 0;
    bool amb = false;
    if (!dq::parse_timestamp_mask(program, program_len, s, n, v, amb)) return amb ? 2 : 0;
    if (out) *out = v;
    return 1;
}

}  // extern "C"
