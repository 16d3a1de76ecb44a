// csv_write.hip — device-resident columns into the bytes of a CSV body on gfx950 (Table.to_csv of a device table;
// DESIGN.md §3k). The mirror image of csv.hip: the same dialect (',' delimiter, '"' quote, doubled-quote escape, LF
// after every record), the cell text of dq_csv_cell.h.
//
//   1. csvw_mark_kernel    per STRING column: its bytes streamed once, 64 bytes a lane (16-byte loads), into two bits a
//                          byte: "forces quotes" (',' '"' LF CR) and "is a quote". A cell's quoting decision and its
//                          extra length are then an OR and a popcount over its bit range: a lane walks words, not bytes.
//   2. csvw_sizes_kernel   one lane per row: the bytes of its record (typed cells are formatted for their length), then
//                          a rocPRIM exclusive scan of the int64 sizes into row_start[nrows + 1].
//   3. csvw_write_kernel   one workgroup per tile of kWBlock consecutive rows, whose output is the contiguous span
//                          [row_start[r0], row_start[r1]). STAGE route (the span fits kWStage bytes of LDS): every lane
//                          writes its record into LDS, the workgroup flushes the span with aligned 16-byte stores (head
//                          and tail bytewise). DIRECT route (it does not): the lanes write to global memory. On both
//                          routes a STRING cell longer than kWLongCell bytes is copied by the whole wave, 64 bytes a
//                          step, so no lane walks a long cell byte by byte while its wave waits.
//
// Launch counts depend on the number and the types of the columns, never on the rows or the bytes. Both calls run the
// mark pass: the C-ABI keeps no state between them.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "dq_common.h"
#include "dq_csv_cell.h"
#include "dq_internal.h"

namespace dq {

constexpr int kWBlock = 256;           // lanes of a workgroup = rows of a write tile
constexpr int kWStage = 31 * 1024;     // LDS stage of the write kernel: 5 workgroups (20 waves) fit a CU's 160 KiB
constexpr int kWLongCell = 64;         // a STRING cell longer than this is copied by its wave
static_assert(kWStage == DQ_CSV_WRITE_STAGE_BYTES, "dq.h and the kernels disagree on the stage");

struct CsvWCol {
    const void* values;
    const uint64_t* validity;
    const void* offsets;
    const uint64_t* special;  // STRING: bit i = byte i forces quotes
    const uint64_t* quote;    // STRING: bit i = byte i is '"'
    int32_t type, scale, off64, pad;
};

__global__ void __launch_bounds__(kWBlock)
csvw_mark_kernel(const uint8_t* __restrict__ data, int64_t n, int64_t nwords, uint64_t* __restrict__ special,
                 uint64_t* __restrict__ quote) {
    const int64_t word = (int64_t)blockIdx.x * kWBlock + threadIdx.x;
    if (word >= nwords) return;
    const int64_t base = word * 64;
    uint64_t sp = 0, qt = 0;
    if (base + 64 <= n && ((uintptr_t)data & 15) == 0) {
        const uint4* p = reinterpret_cast<const uint4*>(data + base);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint4 q = p[v];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t c = (w[k] >> (8 * b)) & 0xFFu;
                    const int bit = v * 16 + k * 4 + b;
                    sp |= (uint64_t)csv_special_byte(c) << bit;
                    qt |= (uint64_t)(c == '"') << bit;
                }
            }
        }
    } else {
        for (int i = 0; i < 64 && base + i < n; ++i) {
            const uint32_t c = data[base + i];
            sp |= (uint64_t)csv_special_byte(c) << i;
            qt |= (uint64_t)(c == '"') << i;
        }
    }
    special[word] = sp;
    quote[word] = qt;
}

__device__ __forceinline__ int64_t csvw_offset(const CsvWCol& c, int64_t r) {
    return c.off64 ? static_cast<const int64_t*>(c.offsets)[r] : (int64_t) static_cast<const int32_t*>(c.offsets)[r];
}

__device__ __forceinline__ bool csvw_valid(const CsvWCol& c, int64_t r) {
    return !c.validity || ((c.validity[r >> 6] >> (r & 63)) & 1ull);
}

struct CsvWCell {
    int64_t start, len, quotes;
    bool quoted;
};

// A STRING cell from the column's bitmaps: one OR and one popcount per 64 bytes.
__device__ __forceinline__ CsvWCell csvw_string_cell(const CsvWCol& c, int64_t r) {
    const int64_t a = csvw_offset(c, r), b = csvw_offset(c, r + 1);
    CsvWCell cell = {a, b > a ? b - a : 0, 0, b <= a};
    if (b > a) {
        const int64_t w0 = a >> 6, w1 = (b - 1) >> 6;
        uint64_t any = 0;
        for (int64_t w = w0; w <= w1; ++w) {
            uint64_t m = ~0ull;
            if (w == w0) m &= ~0ull << (a & 63);
            if (w == w1 && (b & 63)) m &= (1ull << (b & 63)) - 1ull;
            any |= c.special[w] & m;
            cell.quotes += __popcll(c.quote[w] & m);
        }
        cell.quoted = any != 0;
    }
    return cell;
}

__global__ void __launch_bounds__(kWBlock)
csvw_sizes_kernel(const CsvWCol* __restrict__ cols, int ncols, int64_t nrows, int64_t* __restrict__ sizes) {
    const int64_t r = (int64_t)blockIdx.x * kWBlock + threadIdx.x;
    if (r > nrows) return;
    int64_t total = 0;
    if (r < nrows) {
        total = ncols;  // ncols - 1 commas and the LF
        for (int c = 0; c < ncols; ++c) {
            const CsvWCol col = cols[c];
            if (!csvw_valid(col, r)) continue;
            if (col.type == DQ_TYPE_STRING) {
                const CsvWCell cell = csvw_string_cell(col, r);
                total += csv_quoted_length(cell.len, cell.quoted, cell.quotes);
            } else {
                uint8_t buf[kCsvCellText];
                total += csv_typed_text(col.type, col.values, r, col.scale, buf);
            }
        }
    }
    sizes[r] = total;
}

__device__ __forceinline__ int64_t csvw_shfl64(int64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The whole wave copies one cell (every lane calls this with the same arguments), quoted or as it is.
__device__ __forceinline__ void csvw_wave_copy(uint8_t* dst, const uint8_t* __restrict__ src, int64_t len, bool quoted,
                                               int lane) {
    if (!quoted) {
        for (int64_t i = lane; i < len; i += 64) dst[i] = src[i];
        return;
    }
    int64_t at = 1, quotes = 0;  // the output position of the step's first byte; the quotes so far
    for (int64_t i0 = 0; i0 < len; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool in = i < len;
        const uint8_t b = in ? src[i] : (uint8_t)0;
        const bool isq = in && b == '"';
        const unsigned long long qm = __ballot(isq);
        if (in) {
            const int64_t p = at + lane + __popcll(qm & ((1ull << lane) - 1ull));
            dst[p] = b;
            if (isq) dst[p + 1] = '"';
        }
        const int nq = __popcll(qm);
        at += 64 + nq;
        quotes += nq;
    }
    if (lane == 0) {
        dst[0] = '"';
        dst[1 + len + quotes] = '"';
    }
}

// Row r's record at base + pos (LDS or global memory). Every lane of the wave runs this, live or not: the long cells of
// a column are copied by the wave between the lanes' own cells.
__device__ __forceinline__ void csvw_row(const CsvWCol* __restrict__ cols, int ncols, int64_t r, bool live, uint8_t* base,
                                         int64_t pos) {
    const int lane = threadIdx.x & 63;
    for (int c = 0; c < ncols; ++c) {
        const CsvWCol col = cols[c];
        int64_t lsrc = 0, ldst = 0, llen = 0;
        int lquoted = 0;
        bool is_long = false;
        if (live) {
            if (c) base[pos++] = ',';
            if (csvw_valid(col, r)) {
                if (col.type == DQ_TYPE_STRING) {
                    const CsvWCell cell = csvw_string_cell(col, r);
                    const uint8_t* s = static_cast<const uint8_t*>(col.values) + cell.start;
                    if (cell.len > kWLongCell) {
                        is_long = true;
                        lsrc = (int64_t)(uintptr_t)s;
                        ldst = pos;
                        llen = cell.len;
                        lquoted = cell.quoted;
                    } else if (cell.quoted) {
                        csv_quoted_copy(base + pos, s, cell.len);
                    } else {
                        for (int k = 0; k < (int)cell.len; ++k) base[pos + k] = s[k];
                    }
                    pos += csv_quoted_length(cell.len, cell.quoted, cell.quotes);
                } else {
                    uint8_t buf[kCsvCellText];
                    const int n = csv_typed_text(col.type, col.values, r, col.scale, buf);
                    for (int k = 0; k < n; ++k) base[pos + k] = buf[k];
                    pos += n;
                }
            }
        }
        unsigned long long m = __ballot(is_long);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint8_t* src = reinterpret_cast<const uint8_t*>((uintptr_t)csvw_shfl64(lsrc, l));
            const int64_t dst = csvw_shfl64(ldst, l), len = csvw_shfl64(llen, l);
            const bool quoted = __shfl(lquoted, l, 64) != 0;
            csvw_wave_copy(base + dst, src, len, quoted, lane);
        }
    }
    if (live) base[pos] = '\n';
}

// routes[0] += 1 for a tile that took the STAGE route, routes[1] for one that took the DIRECT route.
__global__ void __launch_bounds__(kWBlock)
csvw_write_kernel(const CsvWCol* __restrict__ cols, int ncols, int64_t nrows, const int64_t* __restrict__ row_start,
                  uint8_t* __restrict__ out, unsigned long long* __restrict__ routes) {
    __shared__ __align__(16) uint8_t stage[kWStage];
    const int64_t r0 = (int64_t)blockIdx.x * kWBlock;
    const int64_t r1 = r0 + kWBlock < nrows ? r0 + kWBlock : nrows;
    const int64_t r = r0 + threadIdx.x;
    const bool live = r < r1;
    const int64_t s0 = row_start[r0], span = row_start[r1] - s0;
    uint8_t* g0 = out + s0;
    // the span lies in LDS at the alignment it has in global memory, so 16-byte units of the two coincide
    const int shift = (int)((uintptr_t)g0 & 15);
    const bool staged = span + shift <= kWStage;
    if (threadIdx.x == 0) atomicAdd(&routes[staged ? 0 : 1], 1ull);
    const int64_t pos = live ? row_start[r] - s0 : 0;
    if (!staged) {
        csvw_row(cols, ncols, r, live, g0, pos);
        return;
    }
    csvw_row(cols, ncols, r, live, stage + shift, pos);
    __syncthreads();
    const int n = (int)span;
    const int head = min(n, (16 - shift) & 15);
    const int body = (n - head) & ~15;
    for (int i = threadIdx.x; i < head; i += kWBlock) g0[i] = stage[shift + i];
    const uint4* ls = reinterpret_cast<const uint4*>(stage + shift + head);
    uint4* gd = reinterpret_cast<uint4*>(g0 + head);
    for (int i = threadIdx.x; i < body / 16; i += kWBlock) gd[i] = ls[i];
    for (int i = head + body + threadIdx.x; i < n; i += kWBlock) g0[i] = stage[shift + i];
}

static unsigned csvw_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kWBlock - 1) / kWBlock); }

// Validates the columns, runs the mark pass of the STRING columns and uploads the column records: *dcols.
static int csvw_prepare(dq_ctx* ctx, const char* what, const dq_column* columns, int32_t ncols, int64_t nrows,
                        ScratchBuffers& buf, CsvWCol** dcols) {
    char msg[256];
    if (ctx_num_subs(ctx) != 0) {
        snprintf(msg, sizeof(msg), "%s: multi-device contexts are not supported", what);
        return ctx_fail(ctx, DQ_ERR_UNSUPPORTED, msg);
    }
    std::vector<CsvWCol> h((size_t)ncols);
    for (int c = 0; c < ncols; ++c) {
        const dq_column& col = columns[c];
        int width = 0;
        switch (col.spark_type) {
            case DQ_TYPE_BOOLEAN: case DQ_TYPE_BYTE: case DQ_TYPE_STRING: width = 1; break;
            case DQ_TYPE_SHORT: width = 2; break;
            case DQ_TYPE_INT: case DQ_TYPE_FLOAT: case DQ_TYPE_DATE: width = 4; break;
            case DQ_TYPE_LONG: case DQ_TYPE_DOUBLE: case DQ_TYPE_TIMESTAMP: case DQ_TYPE_DECIMAL: width = 8; break;
            default:
                snprintf(msg, sizeof(msg), "%s: column %d: type %d has no CSV text on the device (DECIMAL128 is not "
                         "written)", what, c, (int)col.spark_type);
                return ctx_fail(ctx, DQ_ERR_UNSUPPORTED, msg);
        }
        const bool is_string = col.spark_type == DQ_TYPE_STRING;
        if (!(col.flags & DQ_COL_DEVICE) || col.length != nrows || (nrows > 0 && !col.values) || (is_string && !col.offsets)) {
            snprintf(msg, sizeof(msg), "%s: column %d must be a device column of %lld rows with its buffers", what, c,
                     (long long)nrows);
            return ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, msg);
        }
        const int owidth = (col.flags & DQ_COL_OFFSETS64) ? 8 : 4;
        if (((uintptr_t)col.validity & 7) || ((uintptr_t)col.values & (uintptr_t)(width - 1)) ||
            (is_string && ((uintptr_t)col.offsets & (uintptr_t)(owidth - 1)))) {
            snprintf(msg, sizeof(msg), "%s: column %d: misaligned buffer", what, c);
            return ctx_fail(ctx, DQ_ERR_ALIGNMENT, msg);
        }
        h[c] = CsvWCol{col.values, reinterpret_cast<const uint64_t*>(col.validity), col.offsets, nullptr, nullptr,
                       (int32_t)col.spark_type, (int32_t)col.decimal_scale, owidth == 8 ? 1 : 0, 0};
    }
    hipStream_t s = ctx_stream(ctx);
    // the end of every STRING column's bytes (its last offset) sizes its bitmaps
    std::vector<int64_t> ends((size_t)ncols, 0);
    std::vector<int32_t> ends32((size_t)ncols, 0);
    for (int c = 0; c < ncols; ++c) {
        if (h[c].type != DQ_TYPE_STRING) continue;
        if (h[c].off64) DQ_CTX_HIP(ctx, hipMemcpyAsync(&ends[c], static_cast<const int64_t*>(h[c].offsets) + nrows, 8, hipMemcpyDeviceToHost, s));
        else DQ_CTX_HIP(ctx, hipMemcpyAsync(&ends32[c], static_cast<const int32_t*>(h[c].offsets) + nrows, 4, hipMemcpyDeviceToHost, s));
    }
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    for (int c = 0; c < ncols; ++c) {
        if (h[c].type != DQ_TYPE_STRING) continue;
        const int64_t end = h[c].off64 ? ends[c] : (int64_t)ends32[c];
        if (end < 0) {
            snprintf(msg, sizeof(msg), "%s: column %d: a negative last offset", what, c);
            return ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, msg);
        }
        const int64_t nwords = std::max<int64_t>(1, (end + 63) / 64);
        uint64_t *sp = nullptr, *qt = nullptr;
        DQ_CTX_HIP(ctx, buf.alloc((void**)&sp, sizeof(uint64_t) * (size_t)nwords));
        DQ_CTX_HIP(ctx, buf.alloc((void**)&qt, sizeof(uint64_t) * (size_t)nwords));
        hipLaunchKernelGGL(csvw_mark_kernel, dim3(csvw_blocks(nwords)), dim3(kWBlock), 0, s,
                           static_cast<const uint8_t*>(h[c].values), end, nwords, sp, qt);
        DQ_CTX_HIP(ctx, hipGetLastError());
        ctx->csv_write_launches[DQ_CSV_WRITE_KERNEL_MARK]++;
        h[c].special = sp;
        h[c].quote = qt;
    }
    DQ_CTX_HIP(ctx, buf.alloc((void**)dcols, sizeof(CsvWCol) * (size_t)ncols));
    DQ_CTX_HIP(ctx, hipMemcpyAsync(*dcols, h.data(), sizeof(CsvWCol) * (size_t)ncols, hipMemcpyHostToDevice, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));  // `h` leaves scope with the caller's next statement
    return DQ_OK;
}

}  // namespace dq

extern "C" {

int dq_csv_write_size(dq_ctx* ctx, const dq_column* columns, int32_t ncols, int64_t nrows, int64_t* row_start,
                      int64_t* out_bytes) {
    if (!ctx || !columns || ncols < 1 || nrows < 0 || !row_start || !out_bytes)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_write_size: invalid arguments");
    *out_bytes = 0;
    if ((uintptr_t)row_start & 7) return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_csv_write_size: row_start must be 8-B aligned");
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    dq::CsvWCol* dcols = nullptr;
    const int rc = dq::csvw_prepare(ctx, "dq_csv_write_size", columns, ncols, nrows, buf, &dcols);
    if (rc != DQ_OK) return rc;
    int64_t* sizes = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&sizes, sizeof(int64_t) * (size_t)(nrows + 1)));
    hipLaunchKernelGGL(dq::csvw_sizes_kernel, dim3(dq::csvw_blocks(nrows + 1)), dim3(dq::kWBlock), 0, s, dcols, (int)ncols,
                       nrows, sizes);
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->csv_write_launches[DQ_CSV_WRITE_KERNEL_SIZES]++;
    size_t tb = 0;
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, sizes, row_start, (int64_t)0, (size_t)(nrows + 1),
                                            rocprim::plus<int64_t>(), s));
    void* tmp = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc(&tmp, tb));
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(tmp, tb, sizes, row_start, (int64_t)0, (size_t)(nrows + 1),
                                            rocprim::plus<int64_t>(), s));
    int64_t total = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&total, row_start + nrows, sizeof(total), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    *out_bytes = total;
    return DQ_OK;
}

int dq_csv_write(dq_ctx* ctx, const dq_column* columns, int32_t ncols, int64_t nrows, const int64_t* row_start,
                 uint8_t* out, int64_t out_bytes) {
    if (!ctx || !columns || ncols < 1 || nrows < 0 || !row_start || out_bytes < 0 || (!out && out_bytes > 0))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_write: invalid arguments");
    if ((uintptr_t)row_start & 7) return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_csv_write: row_start must be 8-B aligned");
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    dq::CsvWCol* dcols = nullptr;
    const int rc = dq::csvw_prepare(ctx, "dq_csv_write", columns, ncols, nrows, buf, &dcols);
    if (rc != DQ_OK) return rc;
    // the buffer must be the one the sizing call measured: nothing is written past it
    int64_t total = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&total, row_start + nrows, sizeof(total), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    if (total != out_bytes)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_write: out_bytes is not the total of dq_csv_write_size");
    if (nrows == 0) return DQ_OK;
    unsigned long long* droutes = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&droutes, 2 * sizeof(unsigned long long)));
    DQ_CTX_HIP(ctx, hipMemsetAsync(droutes, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(dq::csvw_write_kernel, dim3(dq::csvw_blocks(nrows)), dim3(dq::kWBlock), 0, s, dcols, (int)ncols, nrows,
                       row_start, out, droutes);
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->csv_write_launches[DQ_CSV_WRITE_KERNEL_WRITE]++;
    unsigned long long hroutes[2] = {0, 0};
    DQ_CTX_HIP(ctx, hipMemcpyAsync(hroutes, droutes, sizeof(hroutes), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    ctx->csv_write_routes[DQ_CSV_WRITE_ROUTE_STAGE] += (int64_t)hroutes[0];
    ctx->csv_write_routes[DQ_CSV_WRITE_ROUTE_DIRECT] += (int64_t)hroutes[1];
    return DQ_OK;
}

int64_t dq_csv_write_launch_count(const dq_ctx* ctx, int32_t kernel) {
    if (!ctx || kernel < 0 || kernel >= DQ_CSV_WRITE_KERNEL_COUNT) return -1;
    return ctx->csv_write_launches[kernel];
}

int64_t dq_csv_write_route_count(const dq_ctx* ctx, int32_t route) {
    if (!ctx || route < 0 || route >= DQ_CSV_WRITE_ROUTE_COUNT) return -1;
    return ctx->csv_write_routes[route];
}

}  // extern "C"
