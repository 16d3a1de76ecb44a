// dq_dict.h — layouts shared by the host runtime (dq_api.cpp, call_plans.cpp) and the dictionary kernels (dict.hip).
// The layouts compile without HIP (-DDQ_HOST_ONLY, as dq_internal.h); the launchers after them need the HIP runtime.
#pragma once

#if !defined(DQ_HOST_ONLY)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dq_internal.h"

namespace dq {

constexpr int kDictVecPerWave = 2;                                     // 256-row groups (16-byte loads) a wave issues together
constexpr int kDictWordsPerWave = 4;                                   // 64-row steps (4-byte loads) of the tail loop
constexpr int kDictTileRows = (kBlock / 64) * kDictVecPerWave * 256;   // 2048 rows per workgroup per step
constexpr int kDictLdsWords = 16384;      // most 32-bit LDS counters of a workgroup (64 KiB: two workgroups per CU)
constexpr int kDictLdsCopyWords = 8192;   // counter copies are added only while they fit 32 KiB (four workgroups per CU)
constexpr int kDictLdsCopies = 8;         // most counter copies (chosen by lane); fewer when the dictionary is larger

// Per-slot row statistics (int64, device, zeroed per call).
enum DictStat : int { DS_NONNULL = 0, DS_WHERE_TRUE = 1, DS_WHERE_NOTNULL = 2, DS_BAD_INDEX = 3, DS_COUNT = 4 };
// Per-slot fold accumulators (int64, device): lengths, then the DataType class counts at DF_DT0 + DtClass.
enum DictFold : int { DF_MINLEN = 0, DF_MAXLEN = 1, DF_DT0 = 2, DF_COUNT = 8 };

// One (dictionary column, where) slot.
struct DictSlot {
    const int32_t* indices;
    const uint64_t* validity;     // nullptr = all valid (exactly ceil(nrows / 8) bytes are read)
    const uint64_t* where_t;      // where TRUE (padded bitmap) or nullptr
    const uint64_t* where_nn;     // where NOT NULL
    const uint8_t* dict_data;     // the dictionary's UTF-8 bytes (4-byte aligned, >= 16 readable bytes past the end)
    const int32_t* dict_offsets;  // n_dict + 2 offsets: entry n_dict is the NULL entry
    int64_t* counts;              // n_dict counts
    int64_t* stats;               // DS_COUNT
    int64_t* fold;                // DF_COUNT
    uint32_t* hll;                // kHllRegs registers
    int32_t n_dict;
    int32_t lds_copies;           // 0: 64-bit global atomics
    uint32_t flags;               // StrFlags: what the fold computes
    int32_t pad;
};

// A Compliance / PatternMatch op: the predicate's bitmaps over the slot's n_dict + 1 entries.
struct DictPredOp {
    const uint64_t* pred_t;
    const uint64_t* pred_nn;
    unsigned long long* sums;     // [0] rows with the predicate TRUE, [1] NOT NULL (under the where)
    int32_t slot;
    int32_t pad;
};

struct DictOpMap {
    int32_t op;                   // index into the dq_state output
    int32_t kind;                 // dq_op_kind
    int32_t slot;
    int32_t has_where;
    const unsigned long long* sums;  // DQ_OP_COMPLIANCE: its DictPredOp's sums
};

#if !defined(DQ_HOST_ONLY)
int dict_counts_grid(int cus, int64_t nrows);
void launch_dict_counts(const DictSlot* slots, int nslots, int64_t nrows, int grid, int lds_words, hipStream_t s);
void launch_dict_fold(const DictSlot* slots, int nslots, int max_entries, const DictPredOp* pops, int npops,
                      hipStream_t s);
void launch_dict_finalize(const DictSlot* slots, const DictOpMap* ops, int nops, int64_t nrows, dq_state* out,
                          hipStream_t s);
#endif  // !DQ_HOST_ONLY

}  // namespace dq
