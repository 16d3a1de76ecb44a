// filter.hip — the mask launch of dq_filter_validity on gfx950.
//
// A `where` on a grouping analyzer or ApproxQuantile keeps the rows on which the filter is TRUE. Those analyzers
// already skip NULL cells (a grouping drops the rows whose key columns are all NULL), so a dropped row is a row whose
// key cells are NULL: the filter becomes validity bitmaps, out[j] = TRUE & validity(target j), and no frequency-table
// or quantile kernel takes a filter argument. dq_api.cpp evaluates the predicate into its TRUE bitmap with the scan's
// own predicate launches; filter_validity_kernel below ANDs it into every target in one launch: one lane per 64-row
// word, so a wave reads and writes 512 contiguous bytes per bitmap with 8-byte accesses. Bits at and past nrows are
// cleared whatever the inputs hold there; the TRUE rows are popcounts reduced per wave and block, one integer atomic
// per block.
#include <hip/hip_runtime.h>

#include "dq_common.h"
#include "dq_internal.h"

namespace dq {

constexpr int kFilterBlock = 256;
constexpr int kFilterWaves = kFilterBlock / 64;

__global__ void __launch_bounds__(kFilterBlock)
filter_validity_kernel(const uint64_t* __restrict__ true_bits, const FilterTargets T, int64_t nrows, int64_t nwords,
                       unsigned long long* __restrict__ true_rows) {
    __shared__ unsigned int wcnt[kFilterWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * kFilterBlock + threadIdx.x;
    unsigned int cnt = 0;
    if (w < nwords) {
        const int64_t rem = nrows - w * 64;  // >= 1
        const unsigned long long in = rem < 64 ? (1ull << rem) - 1ull : ~0ull;
        const unsigned long long t = true_bits[w] & in;
        const int64_t vbytes = (nrows + 7) >> 3;
        for (int j = 0; j < T.ntargets; ++j) {
            const uint8_t* v = T.valid[j];
            T.out[j][w] = v ? t & filter_valid_word(v, w, vbytes) : t;
        }
        cnt = (unsigned int)__popcll(t);
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long n = 0;
        for (int k = 0; k < kFilterWaves; ++k) n += wcnt[k];
        if (n) atomicAdd(true_rows, n);
    }
}

int launch_filter_validity(const uint64_t* true_bits, const FilterTargets& targets, int64_t nrows,
                           unsigned long long* true_rows, hipStream_t s) {
    const int64_t nwords = (nrows + 63) >> 6;
    const int64_t blocks = (nwords + kFilterBlock - 1) / kFilterBlock;
    if (blocks <= 0 || blocks > INT32_MAX) return -1;
    hipLaunchKernelGGL(filter_validity_kernel, dim3((unsigned)blocks), dim3(kFilterBlock), 0, s, true_bits, targets, nrows,
                       nwords, true_rows);
    return 0;
}

}  // namespace dq
