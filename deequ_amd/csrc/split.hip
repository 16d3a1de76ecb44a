// split.hip — the train / test row split of ConstraintSuggestionRunner on gfx950.
//
// Replaces data.randomSplit(Array(1 - r, r), seed) (suggestions/ConstraintSuggestionRunner.scala:138-159) by a
// membership that is a function of (seed, global row index, ratio) alone (dq_split.h), so a table splits the same way
// however it is cut into calls. split_rows_kernel reads nothing: one lane per row hashes the row index, a wave ballot
// gives the 64-bit TEST word, its complement within nrows is the TRAIN word. Every workgroup covers exactly
// kSplitTile rows (each wave kSplitWordsPerWave consecutive words, stored by its first lanes as one contiguous run),
// so there is no grid-stride loop; the TEST rows are popcounts, reduced per block and added with one integer atomic.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "dq_common.h"
#include "dq_internal.h"
#include "dq_split.h"

namespace dq {

constexpr int kSplitBlock = 256;
constexpr int kSplitWaves = kSplitBlock / 64;
constexpr int kSplitWordsPerWave = 16;
constexpr int kSplitTile = kSplitBlock * kSplitWordsPerWave;  // rows per workgroup: 64 bitmap words

__global__ void __launch_bounds__(kSplitBlock)
split_rows_kernel(int64_t nrows, int64_t row0, uint64_t seed, uint64_t threshold, uint64_t* __restrict__ train_bits,
                  uint64_t* __restrict__ test_bits, unsigned long long* __restrict__ num_test) {
    __shared__ unsigned int wcnt[kSplitWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwords = (nrows + 63) >> 6;
    const int64_t word0 = ((int64_t)blockIdx.x * kSplitWaves + wave) * kSplitWordsPerWave;
    unsigned long long mine = 0;  // lane i keeps the wave's i-th TEST word
    unsigned int cnt = 0;
#pragma unroll
    for (int i = 0; i < kSplitWordsPerWave; ++i) {
        const int64_t r = (word0 + i) * 64 + lane;
        const bool t = r < nrows && split_row_is_test(row0 + r, seed, threshold);
        const unsigned long long b = __ballot(t);
        if (lane == i) mine = b;
        cnt += (unsigned int)__popcll(b);
    }
    const int64_t w = word0 + lane;
    if (lane < kSplitWordsPerWave && w < nwords) {
        const int64_t rem = nrows - w * 64;  // >= 1
        const unsigned long long in = rem < 64 ? (1ull << rem) - 1ull : ~0ull;
        if (test_bits) test_bits[w] = mine;
        if (train_bits) train_bits[w] = ~mine & in;
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < kSplitWaves; ++k) t += wcnt[k];
        if (t) atomicAdd(num_test, t);
    }
}

}  // namespace dq

extern "C" {

int dq_split_rows(dq_ctx* ctx, int64_t nrows, int64_t row0, uint64_t seed, double test_ratio, uint8_t* train_bits,
                  uint8_t* test_bits, int64_t* num_train, int64_t* num_test) {
    if (!ctx || !num_train || !num_test || !(test_ratio > 0.0 && test_ratio < 1.0) || nrows < 0 || row0 < 0 ||
        row0 > INT64_MAX - nrows)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_split_rows: invalid arguments");
    *num_train = *num_test = 0;
    if (dq::ctx_num_subs(ctx) != 0)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_split_rows: multi-device contexts are not supported");
    if (((uintptr_t)train_bits | (uintptr_t)test_bits) & 7)
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_split_rows: bitmaps must be 8-B aligned");
    if (nrows == 0) return DQ_OK;
    const int64_t blocks = (nrows + dq::kSplitTile - 1) / dq::kSplitTile;
    if (blocks > INT32_MAX)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_split_rows: more than 2^42 rows in one call (split in chunks)");
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    unsigned long long* dcount = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&dcount, sizeof(*dcount)));
    DQ_CTX_HIP(ctx, hipMemsetAsync(dcount, 0, sizeof(*dcount), s));
    hipLaunchKernelGGL(dq::split_rows_kernel, dim3((unsigned)blocks), dim3(dq::kSplitBlock), 0, s, nrows, row0, seed,
                       dq::split_threshold(test_ratio), (uint64_t*)train_bits, (uint64_t*)test_bits, dcount);
    DQ_CTX_HIP(ctx, hipGetLastError());
    unsigned long long hcount = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&hcount, dcount, sizeof(hcount), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    *num_test = (int64_t)hcount;
    *num_train = nrows - (int64_t)hcount;
    return DQ_OK;
}

int dq_split_row_is_test(int64_t global_row, uint64_t seed, double test_ratio) {
    if (global_row < 0 || !(test_ratio > 0.0 && test_ratio < 1.0)) return DQ_ERR_INVALID_ARGUMENT;
    return dq::split_row_is_test(global_row, seed, dq::split_threshold(test_ratio)) ? 1 : 0;
}

}  // extern "C"
