// dq_device.h — small device-only helpers shared by the HIP kernels (never part of a DQ_HOST_ONLY build).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dq {

// Row r of a validity bitmap (64 rows per word, LSB first); nullptr = every row valid.
__device__ __forceinline__ bool row_valid(const uint64_t* validity, int64_t r) {
    return validity == nullptr || ((validity[r >> 6] >> (r & 63)) & 1ull);
}

// UTF-8 characters (non-continuation bytes): UTF8String.numChars for valid UTF-8.
__device__ __forceinline__ int utf8_chars(const uint8_t* s, int n) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += (s[i] & 0xC0) != 0x80;
    return c;
}

// The bytes of one wave's consecutive strings, rows [w0, wl) of a column, staged in the wave's LDS row `stage`
// (kStageWords words) by coalesced dword loads from the 4-byte aligned a0 (the bytes buffer is 4-byte aligned and
// padded, dq.h), so that the lanes then parse LDS, not scattered HBM bytes. Called by the whole wave. Returns the
// staged copy, based at byte a0 of the column, or nullptr when the range does not fit (parse from `bytes` then).
constexpr int kStageWords = 512;  // 2 KB per wave

__device__ __forceinline__ const uint8_t* stage_wave_bytes(uint32_t* stage, const uint8_t* bytes,
                                                           const int32_t* offsets, int64_t w0, int64_t wl, int lane,
                                                           int64_t& a0) {
    const uint8_t* sbase = nullptr;
    const int64_t b0 = offsets[w0], b1 = offsets[wl];
    a0 = b0 & ~(int64_t)3;
    const int64_t nwords = (b1 - a0 + 3) >> 2;  // dwords holding [b0, b1): nothing past the last byte
    if (nwords <= kStageWords) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bytes + a0);
        for (int64_t i = lane; i < nwords; i += 64) stage[i] = src[i];
        sbase = reinterpret_cast<const uint8_t*>(stage);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return sbase;
}

}  // namespace dq
