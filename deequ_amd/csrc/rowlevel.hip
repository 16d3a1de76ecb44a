// rowlevel.hip — the one launch of dq_row_outcomes on gfx950.
//
// A check's outcome on a row is the AND of its terms; a term passes a row it considers when its source bit is set.
// Sources and filters are bitmaps by the time this kernel runs (a column's validity, a predicate's TRUE bitmap from the
// scan's own predicate launches, the ballots of dq_freq_row_bits), so the logic is one lane per 64-row word, as in
// filter_validity_kernel: per term pass = src & w & in and fail = ~src & w & in, per check FAIL |= fail and
// NUL |= ~w & in. The one source that is not a bitmap yet is an inline predicate (RowInlineDev, `column <op> constant`):
// the wave evaluates it over its tile in 64 coalesced passes of 64 rows, pass j's __ballot being word j, which lane j
// keeps in its LDS slot -- the bitmap never goes through HBM and the predicate costs no launch of its own.
// A wave owns a tile of 64 words = 4096 rows. Its lanes store the pass (and validity) words with 8-byte
// stores, 512 contiguous bytes per wave; the BOOLEAN byte column is not written 64 strided bytes per lane: the words are
// exchanged with __shfl so that in store k of 4, lane l expands the 16 bits of rows k * 1024 + 16 l .. + 15 into 16 bytes
// and issues one 16-byte store, 1024 contiguous bytes per wave store instruction. Counts are integer popcounts reduced
// per wave with __shfl_down, kept per wave in LDS over the grid stride, folded per block and added with one integer
// atomic per counter per block: the result does not depend on scheduling.
#include <hip/hip_runtime.h>

#include "dq_common.h"
#include "dq_internal.h"

namespace dq {

constexpr int kRowBlock = 256;
constexpr int kRowWaves = kRowBlock / 64;
constexpr int kRowTileWords = 64;                     // one word per lane
constexpr int kRowTileRows = kRowTileWords * 64;      // 4096 rows per wave tile
constexpr int kRowMaxBlocks = 512;                    // grid cap: 2048 waves; larger inputs stride over the tiles

// Bits 0..7 of b -> 8 bytes of 0 / 1, byte i = bit i.
__device__ __forceinline__ unsigned long long expand8(unsigned int b) {
    unsigned long long x = b & 0xFFull;
    x = (x | (x << 28)) & 0x0000000F0000000Full;
    x = (x | (x << 14)) & 0x0003000300030003ull;
    x = (x | (x << 7)) & 0x0101010101010101ull;
    return x;
}

// Two counts of at most 64 per lane, packed 16 bits each (a wave's sums are at most 4096), reduced to lane 0.
__device__ __forceinline__ unsigned int wave_sum2(unsigned int lo, unsigned int hi) {
    unsigned int v = lo | (hi << 16);
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Spark's NaN-aware double ordering (NaN = NaN, NaN greatest), as the predicate kernels compare.
__device__ __forceinline__ int row_cmp_double(double a, double b) {
    const bool an = a != a, bn = b != b;
    if (an && bn) return 0;
    if (an) return 1;
    if (bn) return -1;
    return a < b ? -1 : (a > b ? 1 : 0);
}

// Is inline predicate Q TRUE on `row` (< nrows)? A NULL cell is not TRUE. The type switches are wave-uniform.
__device__ __forceinline__ bool inline_true(const RowInlineDev& Q, int64_t row) {
    if (Q.validity && !((Q.validity[row >> 3] >> (row & 7)) & 1)) return false;
    int c3;
    if (Q.dbl) {
        double x;
        switch (Q.spark_type) {
            case DQ_TYPE_BOOLEAN: x = static_cast<const uint8_t*>(Q.values)[row] != 0 ? 1.0 : 0.0; break;
            case DQ_TYPE_BYTE: x = (double)static_cast<const int8_t*>(Q.values)[row]; break;
            case DQ_TYPE_SHORT: x = (double)static_cast<const int16_t*>(Q.values)[row]; break;
            case DQ_TYPE_INT: case DQ_TYPE_DATE: x = (double)static_cast<const int32_t*>(Q.values)[row]; break;
            case DQ_TYPE_FLOAT: x = (double)static_cast<const float*>(Q.values)[row]; break;
            case DQ_TYPE_DOUBLE: x = static_cast<const double*>(Q.values)[row]; break;
            default: x = (double)static_cast<const int64_t*>(Q.values)[row]; break;  // LONG / TIMESTAMP
        }
        c3 = row_cmp_double(x, Q.cd);
    } else {
        int64_t x;
        switch (Q.spark_type) {
            case DQ_TYPE_BOOLEAN: x = static_cast<const uint8_t*>(Q.values)[row] != 0 ? 1 : 0; break;
            case DQ_TYPE_BYTE: x = static_cast<const int8_t*>(Q.values)[row]; break;
            case DQ_TYPE_SHORT: x = static_cast<const int16_t*>(Q.values)[row]; break;
            case DQ_TYPE_INT: case DQ_TYPE_DATE: x = static_cast<const int32_t*>(Q.values)[row]; break;
            default: x = static_cast<const int64_t*>(Q.values)[row]; break;  // LONG / TIMESTAMP
        }
        c3 = x < Q.ci ? -1 : (x > Q.ci ? 1 : 0);
    }
    switch (Q.op) {
        case DQ_P_EQ: return c3 == 0;
        case DQ_P_NE: return c3 != 0;
        case DQ_P_LT: return c3 < 0;
        case DQ_P_LE: return c3 <= 0;
        case DQ_P_GT: return c3 > 0;
        default: return c3 >= 0;
    }
}

__global__ void __launch_bounds__(kRowBlock)
row_outcomes_kernel(const RowOutcomeArgs A, int64_t nrows, int64_t nwords, int64_t ntiles,
                    unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long acc[kRowWaves][kRowCounters];
    // the tile's TRUE word of every inline predicate, one slot per lane: a lane reads back only what it wrote
    __shared__ unsigned long long inl[kRowInline][kRowBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < kRowWaves * kRowCounters; i += kRowBlock) (&acc[0][0])[i] = 0;
    __syncthreads();
    const int64_t vbytes = (nrows + 7) >> 3;
    // wave-uniform loop: every lane of a wave runs the same tiles, so the shuffles below see all 64 lanes
    for (int64_t tile = (int64_t)blockIdx.x * kRowWaves + wave; tile < ntiles; tile += (int64_t)gridDim.x * kRowWaves) {
        const int64_t w = tile * kRowTileWords + lane;
        const bool have = w < nwords;
        const int64_t rem = nrows - w * 64;  // >= 1 when have
        const unsigned long long in = !have ? 0ull : rem < 64 ? (1ull << rem) - 1ull : ~0ull;
        // inline predicates: pass j reads rows tile_row0 + 64 j + lane (coalesced), its ballot is word j of the tile
        const int64_t tile_row0 = tile * kRowTileRows;
        for (int p = 0; p < A.ninline; ++p) {
            const RowInlineDev& Q = A.inl[p];
            unsigned long long mine = 0;
            for (int j0 = 0; j0 < kRowTileWords && tile_row0 + 64 * j0 < nrows; j0 += 8) {  // wave-uniform
                bool r[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int64_t row = tile_row0 + 64 * (j0 + j) + lane;
                    r[j] = row < nrows && inline_true(Q, row);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned long long b = __ballot(r[j]);
                    mine = lane == j0 + j ? b : mine;
                }
            }
            inl[p][threadIdx.x] = mine;
        }
        for (int c = 0; c < A.nchecks; ++c) {
            const RowCheckDev& C = A.check[c];
            unsigned long long FAIL = 0, NUL = 0;
            for (int t = C.term_begin; t < C.term_end; ++t) {
                const RowTermDev& T = A.term[t];
                unsigned long long src = ~0ull, wm = in;
                if (have) {
                    if (T.src_kind == RS_WORDS) src = ((const unsigned long long*)T.src)[w];
                    else if (T.src_kind == RS_VALID_BYTES) src = filter_valid_word((const uint8_t*)T.src, w, vbytes);
                    else if (T.src_kind == RS_INLINE) src = inl[T.src_inline][threadIdx.x];
                    if (T.w_inline >= 0) wm = inl[T.w_inline][threadIdx.x] & in;
                    else if (T.w) wm = T.w[w] & in;
                }
                const unsigned long long pass = src & wm, fail = ~src & wm;
                FAIL |= fail;
                NUL |= ~wm & in;
                const unsigned int s = wave_sum2((unsigned int)__popcll(pass), (unsigned int)__popcll(wm));
                if (lane == 0) {
                    acc[wave][2 * t] += s & 0xFFFFu;
                    acc[wave][2 * t + 1] += s >> 16;
                }
            }
            const unsigned long long V = A.null_mode ? ~FAIL & ~NUL & in : ~FAIL & in;
            const unsigned long long nul = A.null_mode ? NUL & ~FAIL & in : 0ull;
            if (have) {
                C.pass[w] = V;
                if (A.null_mode) C.validity[w] = (FAIL | ~NUL) & in;
            }
            const unsigned int s = wave_sum2((unsigned int)__popcll(V), (unsigned int)__popcll(nul));
            if (lane == 0) {
                acc[wave][2 * DQ_ROW_MAX_TERMS + 2 * c] += s & 0xFFFFu;
                acc[wave][2 * DQ_ROW_MAX_TERMS + 2 * c + 1] += s >> 16;
            }
            // the byte column: store k covers rows [k * 1024, (k + 1) * 1024) of the tile, 16 rows per lane
            const int64_t row0 = tile * kRowTileRows + lane * 16;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long word = __shfl(V, k * 16 + (lane >> 2), 64);
                const unsigned int bits = (unsigned int)(word >> ((lane & 3) * 16)) & 0xFFFFu;
                const int64_t r = row0 + k * 1024;
                // r is a multiple of 16: r < nrows keeps the store inside nrows rounded up to 16 bytes, and V is clear
                // at and past nrows, so the padding bytes are 0
                if (r < nrows) *(ulonglong2*)(C.values + r) = make_ulonglong2(expand8(bits), expand8(bits >> 8));
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kRowCounters; i += kRowBlock) {
        unsigned long long n = 0;
        for (int k = 0; k < kRowWaves; ++k) n += acc[k][i];
        if (n) atomicAdd(counts + i, n);
    }
}

int launch_row_outcomes(const RowOutcomeArgs& args, int64_t nrows, unsigned long long* counts, hipStream_t s) {
    const int64_t nwords = (nrows + 63) >> 6;
    const int64_t ntiles = (nwords + kRowTileWords - 1) / kRowTileWords;
    if (ntiles <= 0) return -1;
    const int64_t blocks = std::min<int64_t>((ntiles + kRowWaves - 1) / kRowWaves, kRowMaxBlocks);
    hipLaunchKernelGGL(row_outcomes_kernel, dim3((unsigned)blocks), dim3(kRowBlock), 0, s, args, nrows, nwords, ntiles,
                       counts);
    return 0;
}

}  // namespace dq
