// dq_split.h — the train / test membership of one row (dq_split_rows, dq_split_row_is_test), host and device.
//
// A row belongs to the TEST set iff the top 53 bits of XXH64.hashLong(global row index, seed) (dq_common.h), read as
// an integer, are below test_ratio * 2^53: each row independently with probability test_ratio, a function of
// (seed, global row index, ratio) alone ("Constraint suggestion").
#pragma once

#include <stdint.h>

#include "dq_common.h"

namespace dq {

// test_ratio in ]0, 1[ -> the exclusive upper bound of (hash >> 11) for a TEST row; the product is exact in a double's
// range and below 2^53, so the conversion is exact truncation.
DQ_HD uint64_t split_threshold(double test_ratio) { return (uint64_t)(test_ratio * 9007199254740992.0); }

DQ_HD bool split_row_is_test(int64_t global_row, uint64_t seed, uint64_t threshold) {
    return (xxh_long((uint64_t)global_row, seed) >> 11) < threshold;
}

}  // namespace dq
