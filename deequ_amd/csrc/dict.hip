// dict.hip — dictionary-encoded STRING columns (dq_dict_column): int32 indices into a small dictionary of strings.
//
// Every answer deequ asks of such a column is a function of the dictionary entries and of how many rows under the
// `where` point at each entry, so the per-row work is an index histogram and everything string-shaped runs once per
// entry:
//   dict_counts_kernel   per row: counts[e] for every entry, the rows under the `where`, the non-NULL rows under it.
//                        One launch per call covers every (dictionary column, where) slot. One lane reads four
//                        consecutive indices (16 bytes), so a wave load covers 256 rows = four validity words and
//                        four `where` words; a wave issues the loads of kDictVecPerWave such groups before it uses the
//                        first (unconditionally: a load under the validity bit makes the compiler wait for each one,
//                        DESIGN.md §3d); the rows after the last whole group go in 64-row steps. Dictionaries of up to
//                        DQ_DICT_LDS_ENTRIES entries count in workgroup-private 32-bit LDS counters (several copies,
//                        chosen by lane, while they fit 32 KiB), flushed once per workgroup with 64-bit global adds;
//                        larger ones count with 64-bit global atomics. Steps whose live lanes all hold one index (a
//                        dominant value) are summed in registers and added once per run, so a single hot value does
//                        not queue the lanes, or the chip's waves, on one address. Integer atomics only: exact and
//                        independent of grid and order.
//                        An index outside [0, n_dict) on a live row is never an address: it bumps an error counter.
//   dict_fold_kernel     per entry: UTF-8 lengths, DataType classes, XXH64 -> HLL registers of the entries with
//                        count > 0, and the counts summed under predicate bitmaps evaluated over the entries.
//   dict_finalize_kernel per op: the dq_state dq_scan writes over the decoded column.
// Traffic per row: 4 B + 1 validity bit (+ 2 `where` bits).
#include "dq_common.h"
#include "dq_device.h"
#include "dq_dict.h"
#include "dq_internal.h"
#include "dq_strfn.h"

namespace dq {

namespace {

__device__ __forceinline__ uint64_t dict_valid_word(const uint64_t* validity, int64_t w, int64_t nrows) {
    const int64_t nin = nrows - (w << 6);
    if (nin >= 64) return validity[w];
    const uint8_t* vb = reinterpret_cast<const uint8_t*>(validity) + (w << 3);
    uint64_t v = 0;
    for (int64_t b = 0; b < (nin + 7) / 8; ++b) v |= (uint64_t)vb[b] << (8 * b);
    return v;
}

// A wave's run of steps whose live lanes all hold one index (a dominant value): kept in registers, added once.
struct DictRun {
    int32_t index;
    int64_t count;  // below 2^31 on the LDS path: a workgroup's share of rows is (host check)
};

template <bool LDS>
__device__ __forceinline__ void dict_flush(const DictSlot& s, uint32_t* cnt, int lane, DictRun& run) {
    if (run.count && lane == 0) {
        if (LDS) atomicAdd(&cnt[run.index], (uint32_t)run.count);
        else atomicAdd(reinterpret_cast<unsigned long long*>(s.counts) + run.index, (unsigned long long)run.count);
    }
    run.count = 0;
}

// One 64-row step into the counters: `on` = the row is non-NULL under the `where`. LDS: 32-bit counters, copy by lane.
template <bool LDS>
__device__ __forceinline__ void dict_add(const DictSlot& s, uint32_t* cnt, int copies, int lane, int32_t i, bool on,
                                         int64_t& bad, DictRun& run) {
    const bool ok = on && (uint32_t)i < (uint32_t)s.n_dict;
    bad += __popcll(__ballot(on && !ok));
    const unsigned long long okm = __ballot(ok);
    if (!okm) return;
    const int first = __ffsll(okm) - 1;
    const int32_t i0 = __shfl(i, first, 64);
    const bool uniform = __ballot(ok && i != i0) == 0ull;  // wave-uniform, as is everything the run holds
    if (uniform) {
        if (i0 != run.index) {
            dict_flush<LDS>(s, cnt, lane, run);
            run.index = i0;
        }
        run.count += __popcll(okm);
    } else if (ok) {
        if (LDS) atomicAdd(&cnt[(lane & (copies - 1)) * s.n_dict + i], 1u);
        else atomicAdd(reinterpret_cast<unsigned long long*>(s.counts) + i, 1ull);
    }
}

template <bool LDS>
__device__ __forceinline__ void dict_count_rows(const DictSlot& s, uint32_t* cnt, int copies, int64_t nrows, int lane,
                                                int wave, int64_t& n, int64_t& wt, int64_t& wnn, int64_t& bad) {
    const int64_t nfull = nrows >> 6;
    const int32_t* __restrict__ idx = s.indices;
    const int64_t step = (int64_t)gridDim.x * (kBlock / 64) * kDictWordsPerWave;
    DictRun run = {0, 0};
    // The bulk: 16-byte loads, one lane reads four consecutive rows, so a wave load covers 256 rows = four bitmap
    // words (lane l holds rows 4 * (l & 15) .. + 3 of word l >> 4). The loads of kDictVecPerWave such groups are issued
    // before the first is used. Needs 16-byte aligned indices; otherwise every word takes the 4-byte loop below.
    const int64_t nvec = (reinterpret_cast<uintptr_t>(idx) & 15) ? 0 : nrows >> 8;
    {
        const int4* __restrict__ idx4 = reinterpret_cast<const int4*>(idx);
        const int sub = lane >> 4, sh = (lane & 15) * 4;
        long long ln = 0, lwt = 0, lwnn = 0;  // this lane's rows: summed over the wave after the loop
        const int64_t vstep = (int64_t)gridDim.x * (kBlock / 64) * kDictVecPerWave;
        for (int64_t g0 = ((int64_t)blockIdx.x * (kBlock / 64) + wave) * kDictVecPerWave; g0 < nvec; g0 += vstep) {
            int4 v[kDictVecPerWave];
            uint32_t m[kDictVecPerWave];
#pragma unroll
            for (int k = 0; k < kDictVecPerWave; ++k) {
                const bool live = g0 + k < nvec;
                const int64_t g = live ? g0 + k : nvec - 1;  // < nvec: rows (g << 8) + 4 * lane + 3 < nrows
                v[k] = idx4[(g << 6) + lane];
                const int64_t w = (g << 2) + sub;             // < nrows >> 6: a whole word
                const uint32_t wtb = s.where_t ? (uint32_t)(s.where_t[w] >> sh) & 15u : 15u;
                const uint32_t wnb = s.where_t ? (uint32_t)(s.where_nn[w] >> sh) & 15u : 15u;
                const uint32_t vb = s.validity ? (uint32_t)(s.validity[w] >> sh) & 15u : 15u;
                m[k] = live ? (vb & wtb) : 0u;
                lwt += live ? __popc(wtb) : 0;
                lwnn += live ? __popc(wnb) : 0;
                ln += __popc(m[k]);
            }
#pragma unroll
            for (int k = 0; k < kDictVecPerWave; ++k) {
                dict_add<LDS>(s, cnt, copies, lane, v[k].x, m[k] & 1u, bad, run);
                dict_add<LDS>(s, cnt, copies, lane, v[k].y, m[k] & 2u, bad, run);
                dict_add<LDS>(s, cnt, copies, lane, v[k].z, m[k] & 4u, bad, run);
                dict_add<LDS>(s, cnt, copies, lane, v[k].w, m[k] & 8u, bad, run);
            }
        }
#pragma unroll 1
        for (int off = 32; off > 0; off >>= 1) {
            ln += __shfl_xor(ln, off, 64);
            lwt += __shfl_xor(lwt, off, 64);
            lwnn += __shfl_xor(lwnn, off, 64);
        }
        n += ln;
        wt += lwt;
        wnn += lwnn;
    }
    // the words after the last whole 256-row group (or every word), 4-byte loads: one lane reads one row
    for (int64_t w0 = (nvec << 2) + ((int64_t)blockIdx.x * (kBlock / 64) + wave) * kDictWordsPerWave; w0 < nfull; w0 += step) {
        int32_t v[kDictWordsPerWave];
        uint64_t m[kDictWordsPerWave];
#pragma unroll
        for (int k = 0; k < kDictWordsPerWave; ++k) {
            const bool live = w0 + k < nfull;
            const int64_t w = live ? w0 + k : nfull - 1;  // < nfull: rows (w << 6) + lane < nrows
            v[k] = idx[(w << 6) + lane];
            const uint64_t wtb = s.where_t ? s.where_t[w] : ~0ull;
            const uint64_t wnb = s.where_t ? s.where_nn[w] : ~0ull;
            const uint64_t vw = s.validity ? s.validity[w] : ~0ull;
            m[k] = live ? (vw & wtb) : 0ull;
            wt += live ? __popcll(wtb) : 0;
            wnn += live ? __popcll(wnb) : 0;
            n += __popcll(m[k]);
        }
#pragma unroll
        for (int k = 0; k < kDictWordsPerWave; ++k) dict_add<LDS>(s, cnt, copies, lane, v[k], (m[k] >> lane) & 1ull, bad, run);
    }
    if ((nrows & 63) && blockIdx.x == 0 && wave == 0) {  // the ragged last word: rows past nrows never count
        const int64_t nin = nrows & 63;
        const uint64_t range = (1ull << nin) - 1ull;
        const uint64_t wtb = s.where_t ? (s.where_t[nfull] & range) : range;
        const uint64_t wnb = s.where_t ? (s.where_nn[nfull] & range) : range;
        const uint64_t mask = s.validity ? (dict_valid_word(s.validity, nfull, nrows) & wtb) : wtb;
        wt += __popcll(wtb);
        wnn += __popcll(wnb);
        n += __popcll(mask);
        const bool on = (mask >> lane) & 1ull;  // only rows whose bit is set are read: every such row is < nrows
        const int32_t i = on ? idx[(nfull << 6) + lane] : 0;
        dict_add<LDS>(s, cnt, copies, lane, i, on, bad, run);
    }
    dict_flush<LDS>(s, cnt, lane, run);
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
dict_counts_kernel(const DictSlot* __restrict__ slots, int nslots, int64_t nrows) {
    extern __shared__ uint32_t cnt[];  // the launch's largest copies * n_dict words (at most kDictLdsWords)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int si = 0; si < nslots; ++si) {
        const DictSlot s = slots[si];
        const int copies = s.lds_copies;  // 0: global atomics; else a power of two with copies * n_dict <= kDictLdsWords
        if (copies) {
            for (int i = tid; i < copies * s.n_dict; i += kBlock) cnt[i] = 0;
            __syncthreads();
        }
        int64_t n = 0, wt = 0, wnn = 0, bad = 0;  // the same in every lane of the wave
        if (copies) dict_count_rows<true>(s, cnt, copies, nrows, lane, wave, n, wt, wnn, bad);
        else dict_count_rows<false>(s, cnt, copies, nrows, lane, wave, n, wt, wnn, bad);
        if (lane == 0) {
            unsigned long long* st = reinterpret_cast<unsigned long long*>(s.stats);
            if (n) atomicAdd(&st[DS_NONNULL], (unsigned long long)n);
            if (wt) atomicAdd(&st[DS_WHERE_TRUE], (unsigned long long)wt);
            if (wnn) atomicAdd(&st[DS_WHERE_NOTNULL], (unsigned long long)wnn);
            if (bad) atomicAdd(&st[DS_BAD_INDEX], (unsigned long long)bad);
        }
        if (copies) {
            __syncthreads();  // every wave's LDS adds
            for (int e = tid; e < s.n_dict; e += kBlock) {
                unsigned long long t = 0;
                for (int c = 0; c < copies; ++c) t += cnt[c * s.n_dict + e];
                if (t) atomicAdd(reinterpret_cast<unsigned long long*>(s.counts) + e, t);
            }
            __syncthreads();
        }
    }
}

// One lane per dictionary entry, blockIdx.y = slot. Entry n_dict of the dictionary buffers is the NULL entry: its
// count is the NULL rows under the `where`, which a predicate evaluated over the entries may count (`c IS NULL`).
__global__ void __launch_bounds__(kBlock)
dict_fold_kernel(const DictSlot* __restrict__ slots, const DictPredOp* __restrict__ pops, int npops) {
    const int si = blockIdx.y;
    const DictSlot s = slots[si];
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e > s.n_dict) return;
    const int64_t* st = s.stats;
    const int64_t c = e < s.n_dict ? s.counts[e] : st[DS_WHERE_TRUE] - st[DS_NONNULL];
    if (c <= 0) return;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(s.fold);
    for (int p = 0; p < npops; ++p) {
        if (pops[p].slot != si) continue;
        if ((pops[p].pred_t[e >> 6] >> (e & 63)) & 1ull) atomicAdd(&pops[p].sums[0], (unsigned long long)c);
        if ((pops[p].pred_nn[e >> 6] >> (e & 63)) & 1ull) atomicAdd(&pops[p].sums[1], (unsigned long long)c);
    }
    if (e == s.n_dict) return;
    const int64_t o0 = s.dict_offsets[e], o1 = s.dict_offsets[e + 1];
    if (s.flags & SF_LEN) {
        const unsigned long long len = (unsigned long long)utf8_length(s.dict_data, o0, o1);  // >= 0
        atomicMax(&acc[DF_MINLEN], (unsigned long long)INT64_MAX - len);  // INT64_MAX - the shortest: every accumulator starts at 0
        atomicMax(&acc[DF_MAXLEN], len);
    }
    if (s.flags & SF_DTYPE) atomicAdd(&acc[DF_DT0 + classify_string(s.dict_data, o0, o1)], (unsigned long long)c);
    if (s.flags & SF_HLL) {
        const uint64_t x = xxh64_utf8(s.dict_data, o0, o1, SPARK_HLL_SEED);
        atomicMax(s.hll + hll_index(x), hll_rank(x));
    }
}

// One thread per op: the state dq_scan writes for the op over the decoded column (finalize_kernel,
// finalize_strings_kernel).
__global__ void dict_finalize_kernel(const DictSlot* __restrict__ slots, const DictOpMap* __restrict__ ops, int nops,
                                     int64_t nrows, dq_state* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nops) return;
    const DictOpMap om = ops[i];
    const DictSlot s = slots[om.slot];
    dq_state* st = out + om.op;
    for (int w = 0; w < DQ_HLL_NUM_WORDS; ++w) st->u.hll.words[w] = 0;
    st->kind = om.kind;
    const int64_t n = s.stats[DS_NONNULL];
    // conditionalCount(where) (A/Analyzer.scala:426-432): NULL when no row has a non-null `where` value
    const int64_t cond_count = om.has_where ? s.stats[DS_WHERE_TRUE] : nrows;
    const bool cond_present = om.has_where ? s.stats[DS_WHERE_NOTNULL] > 0 : true;
    int present = 0;
    switch (om.kind) {
        case DQ_OP_COMPLETENESS:
            st->u.num_matches_and_count.num_matches = n;
            st->u.num_matches_and_count.count = cond_count;
            present = nrows > 0 && cond_present;
            break;
        case DQ_OP_COMPLIANCE:
            st->u.num_matches_and_count.num_matches = (int64_t)om.sums[0];
            st->u.num_matches_and_count.count = cond_count;
            present = om.sums[1] > 0 && cond_present;
            break;
        case DQ_OP_MIN_LENGTH:
            st->u.dbl.value = (double)(INT64_MAX - s.fold[DF_MINLEN]);
            present = n > 0;
            break;
        case DQ_OP_MAX_LENGTH:
            st->u.dbl.value = (double)s.fold[DF_MAXLEN];
            present = n > 0;
            break;
        case DQ_OP_DATATYPE: {
            const int64_t* dt = s.fold + DF_DT0;
            st->u.datatype.num_fractional = dt[DT_FRACTIONAL];
            st->u.datatype.num_integral = dt[DT_INTEGRAL];
            st->u.datatype.num_boolean = dt[DT_BOOLEAN];
            st->u.datatype.num_string = dt[DT_STRING];
            st->u.datatype.num_null = nrows - (dt[1] + dt[2] + dt[3] + dt[4]);
            present = 1;
            break;
        }
        case DQ_OP_APPROX_COUNT_DISTINCT:
            // 6-bit registers, 10 per word, LSB first (C/StatefulHyperloglogPlus.scala:99-109)
            for (int w = 0; w < DQ_HLL_NUM_WORDS; ++w) {
                uint64_t word = 0;
                for (int k = 0; k < 10; ++k) {
                    const int idx = w * 10 + k;
                    if (idx < kHllRegs) word |= (uint64_t)(s.hll[idx] & 63u) << (6 * k);
                }
                st->u.hll.words[w] = (int64_t)word;
            }
            present = 1;
            break;
        default:
            break;
    }
    st->present = present;
}

// Memory-bound: 8 workgroups per CU, fewer when the column is short (the grid of the decimal128 scan).
int dict_counts_grid(int cus, int64_t nrows) {
    const int64_t want = (nrows + kDictTileRows - 1) / kDictTileRows;
    const int64_t cap = (int64_t)cus * 8;
    return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

void launch_dict_counts(const DictSlot* slots, int nslots, int64_t nrows, int grid, int lds_words, hipStream_t s) {
    hipLaunchKernelGGL(dict_counts_kernel, dim3(grid), dim3(kBlock), sizeof(uint32_t) * (size_t)lds_words, s, slots, nslots,
                       nrows);
}

void launch_dict_fold(const DictSlot* slots, int nslots, int max_entries, const DictPredOp* pops, int npops,
                      hipStream_t s) {
    hipLaunchKernelGGL(dict_fold_kernel, dim3((max_entries + 1 + kBlock - 1) / kBlock, nslots), dim3(kBlock), 0, s, slots,
                       pops, npops);
}

void launch_dict_finalize(const DictSlot* slots, const DictOpMap* ops, int nops, int64_t nrows, dq_state* out,
                          hipStream_t s) {
    hipLaunchKernelGGL(dict_finalize_kernel, dim3((nops + 63) / 64), dim3(64), 0, s, slots, ops, nops, nrows, out);
}

}  // namespace dq
