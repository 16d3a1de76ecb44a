// dq_strfn.h — the per-string device functions of the string-shaped ops, over UTF-8 bytes in HBM read as aligned
// little-endian dwords (the buffer has >= 16 readable bytes past its end): one copy for the per-row string scan
// (strings.hip) and the per-entry fold of dictionary-encoded columns (dict.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dq_common.h"

namespace dq {

namespace {

__device__ __forceinline__ uint32_t load_word(const uint8_t* base, int64_t aligned_off) {
    return *reinterpret_cast<const uint32_t*>(base + aligned_off);
}

__device__ __forceinline__ uint8_t byte_at(const uint8_t* base, int64_t off) { return base[off]; }

// UTF-8 characters (non-continuation bytes) in [o0, o1) — UTF8String.numChars for valid UTF-8.
__device__ int64_t utf8_length(const uint8_t* data, int64_t o0, int64_t o1) {
    if (o1 <= o0) return 0;
    int64_t cont = 0;
    const int64_t w0 = o0 & ~(int64_t)3;
    for (int64_t w = w0; w < o1; w += 4) {
        uint32_t x = load_word(data, w);
        uint32_t mask = 0xFFFFFFFFu;
        if (w < o0) mask &= 0xFFFFFFFFu << (8 * (o0 - w));
        if (w + 4 > o1) mask &= 0xFFFFFFFFu >> (8 * (w + 4 - o1));
        // continuation byte: bit 7 set, bit 6 clear
        const uint32_t c = x & ~(x << 1) & 0x80808080u & mask;
        cont += __popc(c);
    }
    return (o1 - o0) - cont;
}

// XXH64.hashUnsafeBytes over data[o0, o1) (seed 42), reading bytes through dword loads.
__device__ __forceinline__ uint64_t le64_at(const uint8_t* data, int64_t p) {
    const int64_t a = p & ~(int64_t)3;
    const int sh = (int)(p - a) * 8;
    const uint32_t w0 = load_word(data, a), w1 = load_word(data, a + 4), w2 = load_word(data, a + 8);
    const uint64_t lo = sh ? (((uint64_t)w1 << (32 - sh)) | (w0 >> sh)) : w0;
    const uint64_t hi = sh ? (((uint64_t)w2 << (32 - sh)) | (w1 >> sh)) : w1;
    return (lo & 0xFFFFFFFFull) | (hi << 32);
}
__device__ __forceinline__ uint32_t le32_at(const uint8_t* data, int64_t p) {
    const int64_t a = p & ~(int64_t)3;
    const int sh = (int)(p - a) * 8;
    const uint32_t w0 = load_word(data, a);
    if (!sh) return w0;
    const uint32_t w1 = load_word(data, a + 4);
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
}

__device__ uint64_t xxh64_utf8(const uint8_t* data, int64_t o0, int64_t o1, uint64_t seed) {
    const int64_t len = o1 - o0;
    int64_t p = o0;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = seed + P64_1 + P64_2, v2 = seed + P64_2, v3 = seed, v4 = seed - P64_1;
        const int64_t limit = o1 - 32;
        do {
            v1 = xxh_round(v1, le64_at(data, p));
            v2 = xxh_round(v2, le64_at(data, p + 8));
            v3 = xxh_round(v3, le64_at(data, p + 16));
            v4 = xxh_round(v4, le64_at(data, p + 24));
            p += 32;
        } while (p <= limit);
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = xxh_merge_round(h, v1);
        h = xxh_merge_round(h, v2);
        h = xxh_merge_round(h, v3);
        h = xxh_merge_round(h, v4);
    } else {
        h = seed + P64_5;
    }
    h += (uint64_t)len;
    while (p + 8 <= o1) {
        h ^= xxh_round(0, le64_at(data, p));
        h = rotl64(h, 27) * P64_1 + P64_4;
        p += 8;
    }
    if (p + 4 <= o1) {
        h ^= (uint64_t)le32_at(data, p) * P64_1;
        h = rotl64(h, 23) * P64_2 + P64_3;
        p += 4;
    }
    while (p < o1) {
        h ^= (uint64_t)byte_at(data, p) * P64_5;
        h = rotl64(h, 11) * P64_1;
        ++p;
    }
    return xxh_fmix(h);
}

enum DtClass : int { DT_NULL = 0, DT_FRACTIONAL = 1, DT_INTEGRAL = 2, DT_BOOLEAN = 3, DT_STRING = 4 };

// First position in [i, o1) that is not an ASCII digit (o1 if none), four bytes per step: a byte b is a digit iff
// t = b ^ 0x30 is < 10, i.e. neither t's bit 7 nor bit 7 of (t & 0x7F) + 0x76 is set (no carry crosses a byte).
__device__ __forceinline__ int64_t skip_digits(const uint8_t* data, int64_t i, int64_t o1) {
    while (i < o1) {
        const int64_t a = i & ~(int64_t)3;
        const int k = (int)(i - a);
        const uint32_t t = (load_word(data, a) >> (8 * k)) ^ 0x30303030u;
        const uint32_t nd = (((t & 0x7F7F7F7Fu) + 0x76767676u) | t) & 0x80808080u;
        const int nb = (int)(o1 - i < 4 - k ? o1 - i : 4 - k);  // bytes of this word inside the string
        if (nd) {
            const int pos = __builtin_ctz(nd) >> 3;
            if (pos < nb) return i + pos;
        }
        i += nb;
    }
    return o1;
}

// StatefulDataType's three full-match regexes over the UTF-8 bytes.
__device__ int classify_string(const uint8_t* data, int64_t o0, int64_t o1) {
    int64_t i = o0;
    if (i < o1) {
        const uint8_t c = byte_at(data, i);
        if (c == '-' || c == '+') ++i;
    }
    if (i < o1 && byte_at(data, i) == ' ') ++i;
    i = skip_digits(data, i, o1);
    if (i == o1) return DT_INTEGRAL;  // includes "" and a lone sign
    if (byte_at(data, i) == '.') {
        i = skip_digits(data, i + 1, o1);
        if (i == o1) return DT_FRACTIONAL;
    }
    const int64_t n = o1 - o0;
    if (n == 4 && byte_at(data, o0) == 't' && byte_at(data, o0 + 1) == 'r' && byte_at(data, o0 + 2) == 'u' &&
        byte_at(data, o0 + 3) == 'e')
        return DT_BOOLEAN;
    if (n == 5 && byte_at(data, o0) == 'f' && byte_at(data, o0 + 1) == 'a' && byte_at(data, o0 + 2) == 'l' &&
        byte_at(data, o0 + 3) == 's' && byte_at(data, o0 + 4) == 'e')
        return DT_BOOLEAN;
    return DT_STRING;
}

}  // namespace

}  // namespace dq
