// decimal128.hip — the scan of DQ_TYPE_DECIMAL128 columns (Spark decimals of precision 19..38, 16-byte cells).
//
// One launch per dq_scan call covers every (wide column, where) slot of the call. One lane reads one 16-byte cell
// per step (a global_load_dwordx4), so a wave step covers 64 rows = one validity word and one `where` word; a wave
// issues the loads of kD128WordsPerWave such steps before it uses the first, to keep 4 KB per wave in flight. Per
// slot, only what its ops ask for is computed (D128Flags): the non-NULL count from word popcounts, the exact 192-bit
// sum, the signed 128-bit extremes, the (n, avg, m2) moments over dec128_to_double of each row (what CentralMomentAgg
// sees after its per-row cast) and the HLL++ registers of dec128_spark_hash (LDS atomicMax, then a grid max in
// reduce_hll_kernel).
// Reduction: lanes -> wave (shuffles) -> LDS -> one partial per workgroup -> finalize_decimal128_kernel, which folds
// the workgroup partials in a fixed order. No floating-point atomics. Counts, sums, extremes and registers are
// integers, exact in any order; the moments merge with StandardDeviationState.sum in a fixed tree.
// Traffic: 16 B per row + 1 validity bit (+ 2 `where` bits).
#include "dq_internal.h"
#include "dq_dec128.h"
#include "dq_device.h"

namespace dq {

namespace {

constexpr int kMomCopies = 16;  // LDS copies of the exact-moment counters (4 KB a workgroup)

struct D128Acc {
    Acc192 sum;
    uint64_t minlo, minhi, maxlo, maxhi;
    int64_t cnt;  // rows behind (mean, m2)
    double mean, m2;
};

__device__ __forceinline__ void d128_init(D128Acc& a) {
    acc192_zero(a.sum);
    a.minlo = ~0ull;
    a.minhi = 0x7fffffffffffffffull;  // INT128_MAX
    a.maxlo = 0;
    a.maxhi = 0x8000000000000000ull;  // INT128_MIN
    a.cnt = 0;
    a.mean = 0.0;
    a.m2 = 0.0;
}

// StandardDeviationState.sum (A/StandardDeviation.scala:37-44) with an explicit empty side: the formulas of
// reduce_partials_kernel (scan.hip moments_merge).
__device__ __forceinline__ void d128_moments_merge(int64_t na, double& mean, double& m2, int64_t nb, double meanb,
                                                   double m2b) {
    if (nb == 0) return;
    if (na == 0) {
        mean = meanb;
        m2 = m2b;
        return;
    }
    const double n1 = (double)na, n2 = (double)nb;
    const double newN = n1 + n2;
    const double delta = meanb - mean;
    const double deltaN = delta / newN;
    mean = mean + deltaN * n2;
    m2 = m2 + m2b + delta * deltaN * n1 * n2;
}

__device__ __forceinline__ void d128_merge(D128Acc& a, const D128Acc& b) {
    acc192_add(a.sum, b.sum);
    if (dec128_less(b.minlo, b.minhi, a.minlo, a.minhi)) { a.minlo = b.minlo; a.minhi = b.minhi; }
    if (dec128_less(a.maxlo, a.maxhi, b.maxlo, b.maxhi)) { a.maxlo = b.maxlo; a.maxhi = b.maxhi; }
    d128_moments_merge(a.cnt, a.mean, a.m2, b.cnt, b.mean, b.m2);
    a.cnt += b.cnt;
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int off) {
    return (uint64_t)__shfl_down((unsigned long long)v, off, 64);
}

__device__ __forceinline__ D128Acc d128_shfl_down(const D128Acc& a, int off) {
    D128Acc o;
    o.sum.w[0] = shfl_down_u64(a.sum.w[0], off);
    o.sum.w[1] = shfl_down_u64(a.sum.w[1], off);
    o.sum.w[2] = shfl_down_u64(a.sum.w[2], off);
    o.minlo = shfl_down_u64(a.minlo, off);
    o.minhi = shfl_down_u64(a.minhi, off);
    o.maxlo = shfl_down_u64(a.maxlo, off);
    o.maxhi = shfl_down_u64(a.maxhi, off);
    o.cnt = (int64_t)shfl_down_u64((uint64_t)a.cnt, off);
    o.mean = __shfl_down(a.mean, off, 64);
    o.m2 = __shfl_down(a.m2, off, 64);
    return o;
}

// wave64 tree in a fixed order: lane 0 ends with the wave's fold
__device__ __forceinline__ void d128_wave_reduce(D128Acc& a, int lane) {
#pragma unroll 1
    for (int off = 32; off > 0; off >>= 1) {
        const D128Acc o = d128_shfl_down(a, off);
        if (lane < off) d128_merge(a, o);
    }
}

__device__ __forceinline__ void d128_to_partial(const D128Acc& a, int64_t n, int64_t wt, int64_t wnn, D128Partial& p) {
    p.n = n;
    p.wt = wt;
    p.wnn = wnn;
    p.mcount = a.cnt;
    p.sum[0] = a.sum.w[0];
    p.sum[1] = a.sum.w[1];
    p.sum[2] = a.sum.w[2];
    p.minlo = a.minlo;
    p.minhi = a.minhi;
    p.maxlo = a.maxlo;
    p.maxhi = a.maxhi;
    p.mean = a.mean;
    p.m2 = a.m2;
}

__device__ __forceinline__ void d128_from_partial(const D128Partial& p, D128Acc& a) {
    a.sum.w[0] = p.sum[0];
    a.sum.w[1] = p.sum[1];
    a.sum.w[2] = p.sum[2];
    a.minlo = p.minlo;
    a.minhi = p.minhi;
    a.maxlo = p.maxlo;
    a.maxhi = p.maxhi;
    a.cnt = p.mcount;
    a.mean = p.mean;
    a.m2 = p.m2;
}

// Validity word w of a bitmap of exactly ceil(nrows / 8) bytes: the last word is assembled from its bytes.
__device__ __forceinline__ uint64_t d128_valid_word(const uint64_t* validity, int64_t w, int64_t nrows) {
    const int64_t nin = nrows - (w << 6);
    if (nin >= 64) return validity[w];
    const uint8_t* vb = reinterpret_cast<const uint8_t*>(validity) + (w << 3);
    uint64_t v = 0;
    for (int64_t b = 0; b < (nin + 7) / 8; ++b) v |= (uint64_t)vb[b] << (8 * b);
    return v;
}

}  // namespace

// One row into a lane's accumulators (and the workgroup's HLL registers). A row that is off carries a zero cell.
// HEAVY: the slot has moments or HLL registers (a count / sum / compare slot runs the instantiation without them).
template <bool HEAVY>
__device__ __forceinline__ void d128_row(D128Acc& acc, uint32_t flags, const Dec128Scale& sc, uint32_t* regs,
                                         unsigned long long* mom, uint4 cell, bool on) {
    const uint64_t lo = on ? (((uint64_t)cell.y << 32) | cell.x) : 0ull;
    const uint64_t hi = on ? (((uint64_t)cell.w << 32) | cell.z) : 0ull;
    if (flags & DF_SUM) acc192_add128(acc.sum, lo, hi);
    if ((flags & DF_MINMAX) && on) {
        if (dec128_less(lo, hi, acc.minlo, acc.minhi)) { acc.minlo = lo; acc.minhi = hi; }
        if (dec128_less(acc.maxlo, acc.maxhi, lo, hi)) { acc.maxlo = lo; acc.maxhi = hi; }
    }
    if (HEAVY && (flags & DF_MOMENTS) && on) {
        // CentralMomentAgg's per-row update (Welford) over the row's double
        const double x = dec128_to_double_scaled(lo, hi, sc);
        acc.cnt += 1;
        const double delta = x - acc.mean;
        acc.mean += delta / (double)acc.cnt;
        acc.m2 += delta * (x - acc.mean);
        // and the exact sums of x and x^2 (order-free): signed digits into the workgroup's LDS counters
        // (kMomCopies copies of the counters, by lane: rows of one column share exponents, so the lanes of a wave
        // would otherwise queue on a handful of addresses)
        unsigned long long* mine = mom + (threadIdx.x & (kMomCopies - 1)) * kMomLimbs;
        moment_digits(x, [mine](int limb, int64_t d) {
            if (d) atomicAdd(&mine[limb], (unsigned long long)d);
        });
    }
    if (HEAVY && (flags & DF_HLL) && on) {
        const uint64_t x = dec128_spark_hash(lo, hi, SPARK_HLL_SEED);
        atomicMax(&regs[hll_index(x)], hll_rank(x));
    }
}

// The rows of one slot for this wave: whole 64-row words in steps of kD128WordsPerWave, tiles interleaved over the
// grid; the ragged last word is taken by the first wave of the grid.
template <bool HEAVY>
__device__ __forceinline__ void d128_scan_rows(const D128Slot& s, uint32_t flags, const Dec128Scale& sc, int64_t nrows,
                                               int lane, int wave, uint32_t* regs, unsigned long long* mom,
                                               D128Acc& acc, int64_t& n, int64_t& wt, int64_t& wnn) {
    const int64_t nfull = nrows >> 6;
    const uint4* __restrict__ cells = reinterpret_cast<const uint4*>(s.values);
    const int64_t step = (int64_t)gridDim.x * (kBlock / 64) * kD128WordsPerWave;
    for (int64_t w0 = ((int64_t)blockIdx.x * (kBlock / 64) + wave) * kD128WordsPerWave; w0 < nfull; w0 += step) {
        // every load of the step is issued before the first use: the cells unconditionally (a word past the
        // last whole one re-reads that one and counts nothing), the bitmap words from wave-uniform addresses
        uint4 v[kD128WordsPerWave];
        uint64_t m[kD128WordsPerWave];
#pragma unroll
        for (int k = 0; k < kD128WordsPerWave; ++k) {
            const bool live = w0 + k < nfull;
            const int64_t w = live ? w0 + k : nfull - 1;  // < nfull: rows (w << 6) + lane < nrows
            v[k] = cells[(w << 6) + lane];
            const uint64_t wtb = s.where_t ? s.where_t[w] : ~0ull;
            const uint64_t wnb = s.where_t ? s.where_nn[w] : ~0ull;
            const uint64_t vw = s.validity ? s.validity[w] : ~0ull;
            m[k] = live ? (vw & wtb) : 0ull;
            wt += live ? __popcll(wtb) : 0;
            wnn += live ? __popcll(wnb) : 0;
            n += __popcll(m[k]);
        }
#pragma unroll
        for (int k = 0; k < kD128WordsPerWave; ++k)
            d128_row<HEAVY>(acc, flags, sc, regs, mom, v[k], (m[k] >> lane) & 1ull);
    }
    if ((nrows & 63) && blockIdx.x == 0 && wave == 0) {  // the ragged last word: rows past nrows never count
        const int64_t nin = nrows & 63;
        const uint64_t range = (1ull << nin) - 1ull;
        const uint64_t wtb = s.where_t ? (s.where_t[nfull] & range) : range;
        const uint64_t wnb = s.where_t ? (s.where_nn[nfull] & range) : range;
        const uint64_t mask = s.validity ? (d128_valid_word(s.validity, nfull, nrows) & wtb) : wtb;
        wt += __popcll(wtb);
        wnn += __popcll(wnb);
        n += __popcll(mask);
        const bool on = (mask >> lane) & 1ull;  // only rows whose bit is set are read: every such row is < nrows
        const uint4 cell = on ? cells[(nfull << 6) + lane] : make_uint4(0u, 0u, 0u, 0u);
        d128_row<HEAVY>(acc, flags, sc, regs, mom, cell, on);
    }
}

__global__ void __launch_bounds__(kBlock)
scan_decimal128_kernel(const D128Slot* __restrict__ slots, int nslots, int64_t nrows, int gstride,
                       D128Partial* __restrict__ partials, uint8_t* __restrict__ hll_partials) {
    __shared__ uint32_t regs[kHllRegs];
    __shared__ unsigned long long mom[kMomCopies * kMomLimbs];
    __shared__ D128Partial red[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int si = 0; si < nslots; ++si) {
        const D128Slot s = slots[si];
        uint32_t flags = s.flags;
        if (s.hll_slot < 0) flags &= ~(uint32_t)DF_HLL;
        const bool want_hll = flags & DF_HLL;
        if (want_hll) {
            for (int i = tid; i < kHllRegs; i += kBlock) regs[i] = 0;
        }
        const bool want_mom = flags & DF_MOMENTS;
        if (want_mom) {
            for (int i = tid; i < kMomCopies * kMomLimbs; i += kBlock) mom[i] = 0;
        }
        __syncthreads();
        const Dec128Scale sc = dec128_scale(s.scale);
        D128Acc acc;
        d128_init(acc);
        int64_t n = 0, wt = 0, wnn = 0;  // the same in every lane of the wave
        if (flags & (DF_MOMENTS | DF_HLL)) d128_scan_rows<true>(s, flags, sc, nrows, lane, wave, regs, mom, acc, n, wt, wnn);
        else d128_scan_rows<false>(s, flags, sc, nrows, lane, wave, regs, mom, acc, n, wt, wnn);
        d128_wave_reduce(acc, lane);
        if (lane == 0) d128_to_partial(acc, n, wt, wnn, red[wave]);
        __syncthreads();
        if (tid == 0) {  // the 4 waves in a fixed order
            D128Acc a;
            d128_from_partial(red[0], a);
            int64_t bn = red[0].n, bwt = red[0].wt, bwnn = red[0].wnn;
            for (int w = 1; w < kBlock / 64; ++w) {
                D128Acc b;
                d128_from_partial(red[w], b);
                d128_merge(a, b);
                bn += red[w].n;
                bwt += red[w].wt;
                bwnn += red[w].wnn;
            }
            d128_to_partial(a, bn, bwt, bwnn, partials[(int64_t)si * gstride + blockIdx.x]);  // every field but mom
        }
        if (tid < kMomLimbs) {  // the workgroup's exact moment counters (every lane's LDS adds precede the barrier)
            unsigned long long t = 0;
            if (want_mom) {
                for (int c = 0; c < kMomCopies; ++c) t += mom[c * kMomLimbs + tid];
            }
            partials[(int64_t)si * gstride + blockIdx.x].mom[tid] = (int64_t)t;
        }
        if (want_hll) {
            uint8_t* dst = hll_partials + ((int64_t)s.hll_slot * gstride + blockIdx.x) * kHllRegs;
            for (int i = tid; i < kHllRegs; i += kBlock) dst[i] = (uint8_t)regs[i];
        }
        __syncthreads();
    }
}

// One wave per slot: folds the slot's workgroup partials (lane l takes blocks l, l + 64, ... in order, then the
// wave tree) and writes the dq_state of every op answered from the slot. Finalisation follows A/Sum.scala:40,
// A/Mean.scala:40, A/Minimum.scala:40, A/Maximum.scala:40: aggregate in decimal, then one cast to double.
__global__ void __launch_bounds__(64)
finalize_decimal128_kernel(const D128Slot* __restrict__ slots, const D128OpMap* __restrict__ ops, int nops,
                           const D128Partial* __restrict__ partials, int nblocks, int gstride, int64_t nrows,
                           dq_state* __restrict__ out) {
    const int si = blockIdx.x, lane = threadIdx.x;
    // the exact moment sums: lane l adds counter l of every workgroup (128-bit: 2048 counters of up to 2^62), then
    // lane 0 propagates the carries over the 32-bit digits into two's-complement 64-bit limbs
    __shared__ __int128 momsum[kMomLimbs];
    if (lane < kMomLimbs && (slots[si].flags & DF_MOMENTS)) {
        __int128 t = 0;
        for (int b = 0; b < nblocks; ++b) t += (__int128)partials[(int64_t)si * gstride + b].mom[lane];
        momsum[lane] = t;
    }
    __syncthreads();
    D128Acc acc;
    d128_init(acc);
    int64_t n = 0, wt = 0, wnn = 0;
    for (int b = lane; b < nblocks; b += 64) {
        const D128Partial p = partials[(int64_t)si * gstride + b];
        D128Acc o;
        d128_from_partial(p, o);
        d128_merge(acc, o);
        n += p.n;
        wt += p.wt;
        wnn += p.wnn;
    }
    d128_wave_reduce(acc, lane);
#pragma unroll 1
    for (int off = 32; off > 0; off >>= 1) {
        n += (int64_t)shfl_down_u64((uint64_t)n, off);
        wt += (int64_t)shfl_down_u64((uint64_t)wt, off);
        wnn += (int64_t)shfl_down_u64((uint64_t)wnn, off);
    }
    if (lane != 0) return;
    const int scale = slots[si].scale;
    const bool overflow = acc192_overflows_38(acc.sum);
    const double total = overflow ? NAN : dec128_to_double(acc.sum.w[0], acc.sum.w[1], scale);
    for (int i = 0; i < nops; ++i) {
        const D128OpMap om = ops[i];
        if (om.slot != si) continue;
        dq_state* st = out + om.op;
        for (int w = 0; w < DQ_HLL_NUM_WORDS; ++w) st->u.hll.words[w] = 0;
        st->kind = om.kind;
        // conditionalCount(where) (A/Analyzer.scala:426-432): NULL when no row has a non-null `where` value
        const int64_t cond_count = om.has_where ? wt : nrows;
        const bool cond_present = om.has_where ? wnn > 0 : true;
        int present = n > 0;
        switch (om.kind) {
            case DQ_OP_COMPLETENESS:
                st->u.num_matches_and_count.num_matches = n;
                st->u.num_matches_and_count.count = cond_count;
                present = nrows > 0 && cond_present;
                break;
            case DQ_OP_MEAN:
                st->u.mean.sum = total;
                st->u.mean.count = n;
                st->u.mean.exact = 2;
                for (int k = 0; k < 3; ++k) st->u.mean.wsum[k] = acc.sum.w[k];
                st->u.mean.wscale = scale;
                st->u.mean.woverflow = overflow ? 1 : 0;
                break;
            case DQ_OP_SUM:
                st->u.dbl.value = total;
                st->u.dbl.exact = 2;
                for (int k = 0; k < 3; ++k) st->u.dbl.wsum[k] = acc.sum.w[k];
                st->u.dbl.wscale = scale;
                st->u.dbl.woverflow = overflow ? 1 : 0;
                break;
            case DQ_OP_MINIMUM:
                st->u.dbl.value = n > 0 ? dec128_to_double(acc.minlo, acc.minhi, scale) : 0.0;
                break;
            case DQ_OP_MAXIMUM:
                st->u.dbl.value = n > 0 ? dec128_to_double(acc.maxlo, acc.maxhi, scale) : 0.0;
                break;
            case DQ_OP_STANDARD_DEVIATION:
                st->u.stddev.n = (double)acc.cnt;
                st->u.stddev.avg = acc.mean;
                st->u.stddev.m2 = acc.m2;
                {
                    __int128 carry = 0;
                    for (int k = 0; k < 12; ++k) {  // S1: 12 digits = 6 limbs
                        const __int128 t = (k < kMomS1Limbs ? momsum[k] : (__int128)0) + carry;
                        const uint64_t d = (uint64_t)t & 0xffffffffull;
                        carry = t >> 32;
                        if (k & 1) st->u.stddev.xs1[k >> 1] |= d << 32;
                        else st->u.stddev.xs1[k >> 1] = d;
                    }
                    carry = 0;
                    for (int k = 0; k < 22; ++k) {  // S2: 20 digits and the sign extension = 11 limbs
                        const __int128 t = (k < kMomS2Limbs ? momsum[kMomS1Limbs + k] : (__int128)0) + carry;
                        const uint64_t d = (uint64_t)t & 0xffffffffull;
                        carry = t >> 32;
                        if (k & 1) st->u.stddev.xs2[k >> 1] |= d << 32;
                        else st->u.stddev.xs2[k >> 1] = d;
                    }
                    st->u.stddev.exact = 1;
                }
                break;
            default:
                present = 0;
                break;
        }
        st->present = present;
    }
}

// Memory-bound slots want every CU streaming: 8 workgroups per CU, fewer when the column is short.
int decimal128_scan_grid(int cus, int64_t nrows) {
    const int64_t want = (nrows + kD128TileRows - 1) / kD128TileRows;
    const int64_t cap = (int64_t)cus * 8;
    return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

void launch_decimal128_scan(const D128Slot* slots, int nslots, int64_t nrows, int grid, int gstride,
                            D128Partial* partials, uint8_t* hll_partials, hipStream_t s) {
    if (nslots == 0) return;
    hipLaunchKernelGGL(scan_decimal128_kernel, dim3(grid), dim3(kBlock), 0, s, slots, nslots, nrows, gstride, partials,
                       hll_partials);
}

void launch_finalize_decimal128(const D128Slot* slots, int nslots, const D128OpMap* ops, int nops,
                                const D128Partial* partials, int nblocks, int gstride, int64_t nrows, dq_state* out,
                                hipStream_t s) {
    if (nslots == 0 || nops == 0) return;
    hipLaunchKernelGGL(finalize_decimal128_kernel, dim3(nslots), dim3(64), 0, s, slots, ops, nops, partials, nblocks,
                       gstride, nrows, out);
}

}  // namespace dq
