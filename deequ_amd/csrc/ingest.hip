// ingest.hip — Arrow buffers, uploaded as they are, into the engine's column layout on gfx950
// (Table.from_arrow(t, device=...)).
//
// Arrow's buffers are almost the layout of dq_column: the int / float / date cells, microsecond timestamps and string
// bytes are uploaded straight into their final place and no kernel sees them. What remains per row is here:
//
//   1. ingest_validity_kernel  the validity bitmaps of a column's pieces (slices of Arrow chunks, each starting at its
//                              own bit offset) concatenated bitwise. A lane owns whole 64-bit OUTPUT words: it finds
//                              the pieces covering its 64 rows in the piece table (one binary search for the wave's
//                              first row, then a walk), takes each piece's bits with a funnel shift of two source words
//                              and ORs them in. A piece without a bitmap gives ones; bits at and past nrows are 0.
//   2. ingest_bool_kernel      the same addressing over value bits, 8 rows per lane: one source byte's worth of bits
//                              spread into eight 0/1 bytes, stored as one 8-byte word.
//   3. ingest_offsets_kernel   out[i] = src[i] - src[0] + base (int32 or int64 source), range-checked into a flag.
//   4. ingest_convert_kernel   one template per kind: decimal128 cell -> low 8 bytes or the cell itself, zero under a
//                              clear validity bit; timestamp * or / a constant.
//   5. ingest_indices_kernel   dictionary indices of 1 / 2 / 4 / 8 bytes -> int32, range-checked on valid rows (the
//                              smallest offending row by atomicMin on the report), NULL entries folded into the
//                              piece's validity words (wave ballot), NULL rows' index 0.
//
// Kernels 3-5 are streaming: a workgroup takes a tile of kIngestBlock * kIngestPerLane cells, every lane issues its
// kIngestPerLane loads (one cell each, the lanes of a wave adjacent) before the first use, and stores whole cells.
// No kernel uses an atomic on an output word (the only atomics are on the report of kernel 5: a min and a sum, both
// independent of the order), so no result depends on the grid. A source is read inside its uploaded bytes only.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "dq_common.h"
#include "dq_internal.h"

namespace dq {

constexpr int kIngestBlock = 256;
constexpr int kIngestPerLane = 4;
constexpr int kIngestTile = kIngestBlock * kIngestPerLane;

struct IngestReport {  // device side of dq_ingest_index_report
    unsigned long long bad_row;  // ~0: none
    unsigned long long null_rows;
};

// Word k of an 8-B aligned bitmap of nbytes bytes; bytes at and past nbytes read as 0 and are not loaded.
__device__ __forceinline__ uint64_t ingest_word(const uint8_t* __restrict__ p, int64_t nbytes, int64_t k) {
    const int64_t b = k * 8;
    if (b + 8 <= nbytes) return *reinterpret_cast<const uint64_t*>(p + b);
    uint64_t w = 0;
    for (int64_t i = b; i < nbytes; ++i) w |= (uint64_t)p[i] << (8 * (int)(i - b));
    return w;
}

// The 64 bits from bit `bit` on (bit i of the result = bit + i).
__device__ __forceinline__ uint64_t ingest_bits64(const uint8_t* __restrict__ p, int64_t nbytes, int64_t bit) {
    const int64_t k = bit >> 6;
    const int sh = (int)(bit & 63);
    const uint64_t lo = ingest_word(p, nbytes, k);
    if (sh == 0) return lo;
    const uint64_t hi = ingest_word(p, nbytes, k + 1);
    return (lo >> sh) | (hi << (64 - sh));
}

__device__ __forceinline__ bool ingest_bit(const uint8_t* __restrict__ p, int64_t nbytes, int64_t bit) {
    const int64_t b = bit >> 3;
    return b < nbytes && ((p[b] >> (bit & 7)) & 1);
}

// The first piece that ends after `row` (npieces when there is none).
__device__ __forceinline__ int ingest_find_piece(const dq_ingest_piece* __restrict__ pc, int npieces, int64_t row) {
    int lo = 0, hi = npieces;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pc[mid].out_row0 + pc[mid].rows <= row) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Bits of the output rows [row, min(row + ROWS, nrows)) at bit 0 on, the rest 0. `k`: a piece at or before the one
// that holds `row`.
template <int ROWS>
__device__ __forceinline__ uint64_t ingest_gather_bits(const dq_ingest_piece* __restrict__ pc, int npieces, int k,
                                                       int64_t row, int64_t nrows) {
    const int64_t end = row + ROWS < nrows ? row + ROWS : nrows;
    while (k < npieces && pc[k].out_row0 + pc[k].rows <= row) ++k;
    uint64_t w = 0;
    int64_t r = row;
    while (r < end && k < npieces) {
        const dq_ingest_piece p = pc[k];
        const int64_t stop = end < p.out_row0 + p.rows ? end : p.out_row0 + p.rows;
        const int cnt = (int)(stop - r);  // 1..64
        uint64_t bits = p.src ? ingest_bits64(p.src, p.src_bytes, p.src_bit0 + (r - p.out_row0)) : ~0ull;
        if (cnt < 64) bits &= (1ull << cnt) - 1;
        w |= bits << (int)(r - row);
        r = stop;
        ++k;
    }
    return w;
}

__global__ void __launch_bounds__(kIngestBlock)
ingest_validity_kernel(const dq_ingest_piece* __restrict__ pc, int npieces, int64_t nrows, uint64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * kIngestBlock + threadIdx.x;
    const int64_t nwords = (nrows + 63) >> 6;
    if (word - lane >= nwords) return;  // the whole wave is past the end
    const int k = ingest_find_piece(pc, npieces, (word - lane) << 6);  // wave-uniform
    if (word < nwords) out[word] = ingest_gather_bits<64>(pc, npieces, k, word << 6, nrows);
}

__global__ void __launch_bounds__(kIngestBlock)
ingest_bool_kernel(const dq_ingest_piece* __restrict__ pc, int npieces, int64_t nrows, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t group = (int64_t)blockIdx.x * kIngestBlock + threadIdx.x;  // 8 rows
    const int64_t ngroups = (nrows + 7) >> 3;
    if (group - lane >= ngroups) return;
    const int k = ingest_find_piece(pc, npieces, (group - lane) << 3);  // wave-uniform
    if (group >= ngroups) return;
    const int64_t row = group << 3;
    const uint64_t b = ingest_gather_bits<8>(pc, npieces, k, row, nrows);
    // bit i -> byte i: the multiply copies the 8 bits into every byte, the mask keeps bit i of byte i
    const uint64_t x = (b * 0x0101010101010101ull) & 0x8040201008040201ull;
    const uint64_t bytes = ((x + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;
    if (row + 8 <= nrows) {
        *reinterpret_cast<uint64_t*>(out + row) = bytes;
    } else {
        for (int i = 0; row + i < nrows; ++i) out[row + i] = (uint8_t)(bytes >> (8 * i));
    }
}

template <typename T>
__global__ void __launch_bounds__(kIngestBlock)
ingest_offsets_kernel(const T* __restrict__ src, int64_t count, int64_t base, int32_t* __restrict__ out,
                      int32_t* __restrict__ flag) {
    const int64_t tile = (int64_t)blockIdx.x * kIngestTile + threadIdx.x;
    const int64_t first = (int64_t)src[0];
    T v[kIngestPerLane];
#pragma unroll
    for (int j = 0; j < kIngestPerLane; ++j) {
        const int64_t i = tile + (int64_t)j * kIngestBlock;
        v[j] = i < count ? src[i] : T(0);
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kIngestPerLane; ++j) {
        const int64_t i = tile + (int64_t)j * kIngestBlock;
        if (i < count) {
            const int64_t o = (int64_t)v[j] - first + base;
            bad |= o < 0 || o > (int64_t)INT32_MAX;
            out[i] = (int32_t)o;
        }
    }
    if (bad) *flag = 1;  // every writer stores the same value
}

// KIND: dq_ingest_kind. In / Out cells per kind.
template <int KIND>
struct IngestCells {
    using In = int64_t;
    using Out = int64_t;
};
template <>
struct IngestCells<DQ_INGEST_DECIMAL_LOW> {
    using In = ulonglong2;
    using Out = uint64_t;
};
template <>
struct IngestCells<DQ_INGEST_DECIMAL_WIDE> {
    using In = ulonglong2;
    using Out = ulonglong2;
};

template <int KIND>
__global__ void __launch_bounds__(kIngestBlock)
ingest_convert_kernel(const typename IngestCells<KIND>::In* __restrict__ src, const uint8_t* __restrict__ validity,
                      int64_t validity_bytes, int64_t validity_bit0, int64_t rows, int64_t param,
                      typename IngestCells<KIND>::Out* __restrict__ out) {
    using In = typename IngestCells<KIND>::In;
    const int64_t tile = (int64_t)blockIdx.x * kIngestTile + threadIdx.x;
    In v[kIngestPerLane];
    bool ok[kIngestPerLane];
#pragma unroll
    for (int j = 0; j < kIngestPerLane; ++j) {
        const int64_t i = tile + (int64_t)j * kIngestBlock;
        if (i < rows) v[j] = src[i];
        ok[j] = true;
        if constexpr (KIND == DQ_INGEST_DECIMAL_LOW || KIND == DQ_INGEST_DECIMAL_WIDE)
            if (validity && i < rows) ok[j] = ingest_bit(validity, validity_bytes, validity_bit0 + i);
    }
#pragma unroll
    for (int j = 0; j < kIngestPerLane; ++j) {
        const int64_t i = tile + (int64_t)j * kIngestBlock;
        if (i >= rows) continue;
        if constexpr (KIND == DQ_INGEST_DECIMAL_LOW) {
            out[i] = ok[j] ? v[j].x : 0ull;
        } else if constexpr (KIND == DQ_INGEST_DECIMAL_WIDE) {
            out[i] = ok[j] ? v[j] : make_ulonglong2(0ull, 0ull);
        } else if constexpr (KIND == DQ_INGEST_TIME_MUL) {
            out[i] = (int64_t)((uint64_t)v[j] * (uint64_t)param);  // wraps modulo 2^64
        } else {
            out[i] = v[j] / param;  // truncates toward zero; param > 0, so no overflow
        }
    }
}

// T: the Arrow index type. One row per lane and step, so a wave's ballot is one validity word of the piece.
template <typename T>
__global__ void __launch_bounds__(kIngestBlock)
ingest_indices_kernel(const T* __restrict__ src, const uint8_t* __restrict__ validity, int64_t validity_bytes,
                      int64_t validity_bit0, int64_t rows, int64_t n_dict, const uint8_t* __restrict__ dict_validity,
                      int32_t* __restrict__ out, uint64_t* __restrict__ out_validity, IngestReport* __restrict__ report) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * kIngestTile + threadIdx.x;
    T v[kIngestPerLane];
    bool ok[kIngestPerLane];
#pragma unroll
    for (int j = 0; j < kIngestPerLane; ++j) {
        const int64_t i = tile + (int64_t)j * kIngestBlock;
        v[j] = i < rows ? src[i] : T(0);
        ok[j] = i < rows && (!validity || ingest_bit(validity, validity_bytes, validity_bit0 + i));
    }
    unsigned long long nulls = 0;
#pragma unroll
    for (int j = 0; j < kIngestPerLane; ++j) {
        const int64_t i = tile + (int64_t)j * kIngestBlock;
        const int64_t idx = (int64_t)v[j];  // a uint64 index past 2^63 reads as negative, as the host's astype does
        bool valid = ok[j];
        if (valid && (idx < 0 || idx >= n_dict)) {
            atomicMin(&report->bad_row, (unsigned long long)i);
            valid = false;
        }
        if (valid && dict_validity) valid = (dict_validity[idx >> 3] >> (idx & 7)) & 1;
        if (i < rows) out[i] = valid ? (int32_t)idx : 0;
        const unsigned long long vb = __ballot(valid);
        if (lane == 0 && i < rows) {  // i is the wave's first row: a multiple of 64
            if (out_validity) out_validity[i >> 6] = vb;
            const int64_t in_word = rows - i < 64 ? rows - i : 64;
            nulls += (unsigned long long)(in_word - __popcll(vb));
        }
    }
    if (lane == 0 && nulls) atomicAdd(&report->null_rows, nulls);
}

static unsigned ingest_tiles(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kIngestTile - 1) / kIngestTile); }
static unsigned ingest_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kIngestBlock - 1) / kIngestBlock); }

// The checks every entry point shares; 0 = go on.
static int ingest_enter(dq_ctx* ctx, const char* what) {
    char msg[128];
    if (dq::ctx_num_subs(ctx) != 0) {
        snprintf(msg, sizeof(msg), "%s: multi-device contexts are not supported", what);
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, msg);
    }
    return DQ_OK;
}

}  // namespace dq

extern "C" {

int dq_ingest_bits(dq_ctx* ctx, const dq_ingest_piece* pieces, int32_t npieces, int64_t nrows, int32_t to_bytes,
                   void* out) {
    if (!ctx || nrows < 0 || npieces < 0 || (nrows > 0 && (!pieces || !out || npieces < 1)))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_ingest_bits: invalid arguments");
    if (int rc = dq::ingest_enter(ctx, "dq_ingest_bits")) return rc;
    if (nrows == 0) return DQ_OK;
    int64_t at = 0;
    for (int k = 0; k < npieces; ++k) {
        const dq_ingest_piece& p = pieces[k];
        if (p.rows < 1 || p.out_row0 != at || p.src_bit0 < 0 || p.src_bytes < 0 || (to_bytes && !p.src) ||
            (p.src && (p.src_bit0 + p.rows + 7) / 8 > p.src_bytes))
            return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT,
                                "dq_ingest_bits: the pieces must be non-empty, in row order, and their sources must "
                                "hold their bits");
        if ((uintptr_t)p.src & 7) return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_ingest_bits: a source must be 8-B aligned");
        at += p.rows;
    }
    if (at != nrows) return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_ingest_bits: the pieces do not cover the rows");
    if ((uintptr_t)out & 7) return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_ingest_bits: the output must be 8-B aligned");
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    dq_ingest_piece* dpc = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&dpc, sizeof(dq_ingest_piece) * (size_t)npieces));
    DQ_CTX_HIP(ctx, hipMemcpyAsync(dpc, pieces, sizeof(dq_ingest_piece) * (size_t)npieces, hipMemcpyHostToDevice, s));
    if (to_bytes) {
        hipLaunchKernelGGL(dq::ingest_bool_kernel, dim3(dq::ingest_blocks((nrows + 7) / 8)), dim3(dq::kIngestBlock), 0, s,
                           dpc, (int)npieces, nrows, (uint8_t*)out);
        ctx->kernel_launches[DQ_KERNEL_INGEST_BOOL]++;
    } else {
        hipLaunchKernelGGL(dq::ingest_validity_kernel, dim3(dq::ingest_blocks((nrows + 63) / 64)), dim3(dq::kIngestBlock),
                           0, s, dpc, (int)npieces, nrows, (uint64_t*)out);
        ctx->kernel_launches[DQ_KERNEL_INGEST_VALIDITY]++;
    }
    DQ_CTX_HIP(ctx, hipGetLastError());
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    return DQ_OK;
}

int dq_ingest_offsets(dq_ctx* ctx, const void* src, int64_t src_bytes, int32_t src_width, int64_t rows, int64_t base,
                      int32_t write_last, int32_t* out, int32_t* out_of_range) {
    if (!ctx || !src || !out || !out_of_range || rows < 0 || (src_width != 4 && src_width != 8) ||
        src_bytes < (rows + 1) * src_width)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_ingest_offsets: invalid arguments");
    *out_of_range = 0;
    if (int rc = dq::ingest_enter(ctx, "dq_ingest_offsets")) return rc;
    if (((uintptr_t)src & (uintptr_t)(src_width - 1)) || ((uintptr_t)out & 3))
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_ingest_offsets: misaligned buffer");
    const int64_t count = rows + (write_last ? 1 : 0);
    if (count == 0) return DQ_OK;
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    int32_t* dflag = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&dflag, sizeof(int32_t)));
    DQ_CTX_HIP(ctx, hipMemsetAsync(dflag, 0, sizeof(int32_t), s));
    const dim3 g(dq::ingest_tiles(count)), b(dq::kIngestBlock);
    if (src_width == 4) hipLaunchKernelGGL(dq::ingest_offsets_kernel<int32_t>, g, b, 0, s, (const int32_t*)src, count, base, out, dflag);
    else hipLaunchKernelGGL(dq::ingest_offsets_kernel<int64_t>, g, b, 0, s, (const int64_t*)src, count, base, out, dflag);
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_INGEST_OFFSETS]++;
    int32_t hflag = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&hflag, dflag, sizeof(hflag), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    *out_of_range = hflag;
    return DQ_OK;
}

int dq_ingest_convert(dq_ctx* ctx, int32_t kind, const void* src, int64_t src_bytes, const uint8_t* validity,
                      int64_t validity_bytes, int64_t validity_bit0, int64_t rows, int64_t param, void* out) {
    if (!ctx || rows < 0 || (rows > 0 && (!src || !out)) || kind < DQ_INGEST_DECIMAL_LOW || kind > DQ_INGEST_TIME_DIV)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_ingest_convert: invalid arguments");
    const bool decimal = kind == DQ_INGEST_DECIMAL_LOW || kind == DQ_INGEST_DECIMAL_WIDE;
    const int in_size = decimal ? 16 : 8, out_size = kind == DQ_INGEST_DECIMAL_WIDE ? 16 : 8;
    if (src_bytes < rows * in_size || (kind == DQ_INGEST_TIME_DIV && param <= 0) ||
        (decimal && validity && (validity_bit0 < 0 || (validity_bit0 + rows + 7) / 8 > validity_bytes)))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_ingest_convert: a source is shorter than its rows");
    if (int rc = dq::ingest_enter(ctx, "dq_ingest_convert")) return rc;
    if (((uintptr_t)src & (uintptr_t)(in_size - 1)) || ((uintptr_t)out & (uintptr_t)(out_size - 1)) ||
        ((uintptr_t)validity & 7))
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_ingest_convert: misaligned buffer");
    if (rows == 0) return DQ_OK;
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    const dim3 g(dq::ingest_tiles(rows)), b(dq::kIngestBlock);
    switch (kind) {
        case DQ_INGEST_DECIMAL_LOW:
            hipLaunchKernelGGL(dq::ingest_convert_kernel<DQ_INGEST_DECIMAL_LOW>, g, b, 0, s, (const ulonglong2*)src, validity,
                               validity_bytes, validity_bit0, rows, param, (uint64_t*)out);
            break;
        case DQ_INGEST_DECIMAL_WIDE:
            hipLaunchKernelGGL(dq::ingest_convert_kernel<DQ_INGEST_DECIMAL_WIDE>, g, b, 0, s, (const ulonglong2*)src, validity,
                               validity_bytes, validity_bit0, rows, param, (ulonglong2*)out);
            break;
        case DQ_INGEST_TIME_MUL:
            hipLaunchKernelGGL(dq::ingest_convert_kernel<DQ_INGEST_TIME_MUL>, g, b, 0, s, (const int64_t*)src, validity,
                               validity_bytes, validity_bit0, rows, param, (int64_t*)out);
            break;
        default:
            hipLaunchKernelGGL(dq::ingest_convert_kernel<DQ_INGEST_TIME_DIV>, g, b, 0, s, (const int64_t*)src, validity,
                               validity_bytes, validity_bit0, rows, param, (int64_t*)out);
            break;
    }
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_INGEST_CONVERT]++;
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    return DQ_OK;
}

int dq_ingest_indices(dq_ctx* ctx, const void* src, int64_t src_bytes, int32_t index_width, int32_t index_signed,
                      const uint8_t* validity, int64_t validity_bytes, int64_t validity_bit0, int64_t rows, int64_t n_dict,
                      const uint8_t* dict_validity, int32_t* out, uint8_t* out_validity, dq_ingest_index_report* report) {
    if (!ctx || !report || rows < 0 || n_dict < 0 || n_dict > (int64_t)INT32_MAX || (rows > 0 && (!src || !out)) ||
        (index_width != 1 && index_width != 2 && index_width != 4 && index_width != 8) || src_bytes < rows * index_width ||
        (validity && (validity_bit0 < 0 || (validity_bit0 + rows + 7) / 8 > validity_bytes)))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_ingest_indices: invalid arguments");
    report->bad_row = -1;
    report->bad_index = 0;
    report->null_rows = 0;
    if (int rc = dq::ingest_enter(ctx, "dq_ingest_indices")) return rc;
    if (((uintptr_t)src & 7) || ((uintptr_t)validity & 7) || ((uintptr_t)out & 3) || ((uintptr_t)out_validity & 7))
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_ingest_indices: misaligned buffer");
    if (rows == 0) return DQ_OK;
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    dq::IngestReport* drep = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&drep, sizeof(dq::IngestReport)));
    dq::IngestReport hrep = {~0ull, 0ull};
    DQ_CTX_HIP(ctx, hipMemcpyAsync(drep, &hrep, sizeof(hrep), hipMemcpyHostToDevice, s));
    const dim3 g(dq::ingest_tiles(rows)), b(dq::kIngestBlock);
    uint64_t* ov = (uint64_t*)out_validity;
#define DQ_INGEST_INDICES(T)                                                                                          \
    hipLaunchKernelGGL(dq::ingest_indices_kernel<T>, g, b, 0, s, (const T*)src, validity, validity_bytes, validity_bit0, \
                       rows, n_dict, dict_validity, out, ov, drep)
    switch (index_width * 2 + (index_signed ? 1 : 0)) {
        case 2: DQ_INGEST_INDICES(uint8_t); break;
        case 3: DQ_INGEST_INDICES(int8_t); break;
        case 4: DQ_INGEST_INDICES(uint16_t); break;
        case 5: DQ_INGEST_INDICES(int16_t); break;
        case 8: DQ_INGEST_INDICES(uint32_t); break;
        case 9: DQ_INGEST_INDICES(int32_t); break;
        default: DQ_INGEST_INDICES(int64_t); break;  // uint64 too: by its bit pattern
    }
#undef DQ_INGEST_INDICES
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_INGEST_INDICES]++;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&hrep, drep, sizeof(hrep), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    report->null_rows = (int64_t)hrep.null_rows;
    if (hrep.bad_row != ~0ull) {
        report->bad_row = (int64_t)hrep.bad_row;
        uint64_t cell = 0;  // little-endian: the low index_width bytes
        DQ_CTX_HIP(ctx, hipMemcpyAsync(&cell, (const uint8_t*)src + (int64_t)hrep.bad_row * index_width, (size_t)index_width,
                                       hipMemcpyDeviceToHost, s));
        DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        switch (index_width * 2 + (index_signed ? 1 : 0)) {
            case 3: report->bad_index = (int8_t)cell; break;
            case 5: report->bad_index = (int16_t)cell; break;
            case 9: report->bad_index = (int32_t)cell; break;
            default: report->bad_index = (int64_t)cell; break;  // unsigned narrower cells are already zero-extended
        }
    }
    return DQ_OK;
}

}  // extern "C"
