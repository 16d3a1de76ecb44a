// dq_dec128.h — host+device arithmetic of DQ_TYPE_DECIMAL128 cells (Spark decimals of precision 19..38): one
// body for the scan kernel (decimal128.hip), the cast (cast.hip), the host state algebra (host_algebra.cpp) and the
// CPU tests (tests/sanitize/dec128_checks.cpp).
//
// A cell is a 16-byte little-endian two's-complement unscaled value, passed around as (lo, hi). Three pieces:
//   - exact sums: a sign-extended 128-bit cell added into a 192-bit two's-complement accumulator (three 64-bit
//     limbs, little-endian). 2^191 / 10^38 > 2^64 rows fit before the top limb could wrap, so any order of partial
//     sums gives the same bits;
//   - dec128_to_double: the double nearest to unscaled * 10^-scale, ties to even (Spark's Decimal.toDouble =
//     java.math.BigDecimal.doubleValue, which rounds correctly on both of its paths);
//   - dec128_spark_hash: XxHash64Function.hash of a precision > 18 decimal = XXH64 over
//     unscaledValue().toByteArray, the minimal big-endian two's-complement bytes.
// Only additions, subtractions, shifts and compares of 128-bit integers are used: no 128-bit division, no long
// double, no lookup table.
#pragma once

#include <stdint.h>

#include "dq_common.h"

namespace dq {

typedef unsigned __int128 u128;

struct Acc192 {
    uint64_t w[3];  // little-endian limbs, two's complement
};

DQ_HD void acc192_zero(Acc192& a) { a.w[0] = a.w[1] = a.w[2] = 0; }

// a += b (192 + 192, wrapping)
DQ_HD void acc192_add(Acc192& a, const Acc192& b) {
    u128 t = (u128)a.w[0] + b.w[0];
    a.w[0] = (uint64_t)t;
    t = (t >> 64) + a.w[1] + b.w[1];
    a.w[1] = (uint64_t)t;
    a.w[2] = a.w[2] + b.w[2] + (uint64_t)(t >> 64);
}

// a += sign-extended (lo, hi)
DQ_HD void acc192_add128(Acc192& a, uint64_t lo, uint64_t hi) {
    Acc192 b;
    b.w[0] = lo;
    b.w[1] = hi;
    b.w[2] = (uint64_t)((int64_t)hi >> 63);
    acc192_add(a, b);
}

// signed 128-bit a < b
DQ_HD bool dec128_less(uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi) {
    return (int64_t)ahi < (int64_t)bhi || (ahi == bhi && alo < blo);
}

DQ_HD int clz64_nz(uint64_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// number of bits of an unsigned 128-bit magnitude (0 for 0)
DQ_HD int bit_length128(uint64_t lo, uint64_t hi) {
    if (hi) return 128 - clz64_nz(hi);
    if (lo) return 64 - clz64_nz(lo);
    return 0;
}

// 10^s, 0 <= s <= 38 (10^38 < 2^127), by repeated multiplication: exact, no table
DQ_HD u128 pow10_u128(int s) {
    u128 r = 1;
    for (int i = 0; i < s; ++i) r = (r << 3) + (r << 1);
    return r;
}

// |sum| >= 10^38: the total no longer fits Spark's widest decimal(38, s)
DQ_HD bool acc192_overflows_38(const Acc192& a) {
    Acc192 m = a;
    if ((int64_t)a.w[2] < 0) {  // magnitude = -a
        u128 t = (u128)(~a.w[0]) + 1;
        m.w[0] = (uint64_t)t;
        t = (t >> 64) + (uint64_t)(~a.w[1]);
        m.w[1] = (uint64_t)t;
        m.w[2] = ~a.w[2] + (uint64_t)(t >> 64);
    }
    if (m.w[2]) return true;
    return (((u128)m.w[1] << 64) | m.w[0]) >= pow10_u128(38);
}

// The scale of a column, prepared once per slot (the scale is uniform over a column, so a wave shares it).
struct Dec128Scale {
    u128 d;       // 10^scale
    double dd;    // 10^scale as a double, exact for scale <= 22
    int32_t bits; // bit length of d
    int32_t scale;
};

DQ_HD Dec128Scale dec128_scale(int scale) {
    Dec128Scale p;
    p.scale = scale < 0 ? 0 : (scale > 38 ? 38 : scale);
    p.d = pow10_u128(p.scale);
    p.bits = bit_length128((uint64_t)p.d, (uint64_t)(p.d >> 64));
    double dd = 1.0;
    for (int i = 0; i < p.scale && i < 22; ++i) dd *= 10.0;  // every product <= 10^22 is exact in fp64
    p.dd = dd;
    return p;
}

DQ_HD double pow2_double(int e) {  // 2^e, -1022 <= e <= 1023
    union { uint64_t u; double d; } c;
    c.u = (uint64_t)(e + 1023) << 52;
    return c.d;
}

// The double nearest to m / d (ties to even) for 0 < m < 2^128, 0 < d < 2^127: binary long division. Numerator
// and divisor are aligned to the same bit length, so the quotient r0 / D lies in (1/2, 2); 57 restoring steps give
// q = floor(r0 / D * 2^56), 56 or 57 bits, and a sticky bit (remainder != 0): 53 kept bits, 3 or 4 rounding bits
// and the sticky bit decide the rounding exactly. The result is a 53-bit integer times a power of two in the
// normal range (2^-127 < m / d < 2^128), so the last two steps are exact.
DQ_HD double udiv128_to_double(u128 m, const Dec128Scale& p) {
    const int lm = bit_length128((uint64_t)m, (uint64_t)(m >> 64)), ld = p.bits;
    u128 r = m, D = p.d;
    if (lm >= ld) D <<= (lm - ld);
    else r <<= (ld - lm);
    uint64_t q = 0;
    bool carry = false;  // bit 128 of the doubled remainder (the aligned operands may fill all 128 bits)
    for (int i = 0; i < 57; ++i) {
        const bool ge = carry || r >= D;
        if (ge) r -= D;  // with carry: (2^128 + r) - D < D, so the wrapped difference is the true one
        q = (q << 1) | (ge ? 1u : 0u);
        carry = (uint64_t)(r >> 127) != 0;
        r <<= 1;
    }
    const int shift = (q >> 56) ? 4 : 3;
    uint64_t kept = q >> shift;
    const uint64_t rem = q & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    const bool sticky = r != 0;
    if (rem > half || (rem == half && (sticky || (kept & 1)))) ++kept;
    return (double)kept * pow2_double(lm - ld - 56 + shift);
}

// Java's fast path kept as ours: |unscaled| < 2^53 and scale <= 22 is one fp64 division of two exact operands,
// which rounds correctly; everything else takes the long division (zero included: it returns 0). On the device the
// choice is made per wave: the long division runs only when some active lane needs it, and then for every lane.
DQ_HD double dec128_to_double_scaled(uint64_t lo, uint64_t hi, const Dec128Scale& p) {
    const bool neg = (int64_t)hi < 0;
    u128 m = ((u128)hi << 64) | lo;
    if (neg) m = (u128)0 - m;
    const bool fast = m < ((u128)1 << 53) && p.scale <= 22;
    double r = (double)(uint64_t)m / p.dd;
#if defined(__HIP_DEVICE_COMPILE__)
    if (__ballot(!fast) != 0ull) {
        const double slow = udiv128_to_double(m, p);
        r = fast ? r : slow;
    }
#else
    if (!fast) r = udiv128_to_double(m, p);
#endif
    return neg ? -r : r;
}

// The double nearest to (hi:lo) * 10^-scale, for every 128-bit value and 0 <= scale <= 38.
DQ_HD double dec128_to_double(uint64_t lo, uint64_t hi, int scale) {
    return dec128_to_double_scaled(lo, hi, dec128_scale(scale));
}

// Decimal.toLong: the unscaled value divided by 10^scale truncating toward zero, then its low 64 bits
// (BigDecimal.longValue). Restoring division of the magnitude, one quotient bit per step.
DQ_HD int64_t dec128_to_long_scaled(uint64_t lo, uint64_t hi, const Dec128Scale& p) {
    const bool neg = (int64_t)hi < 0;
    u128 m = ((u128)hi << 64) | lo;
    if (neg) m = (u128)0 - m;
    const int lm = bit_length128((uint64_t)m, (uint64_t)(m >> 64));
    u128 q = 0;
    if (lm >= p.bits) {
        const int steps = lm - p.bits;  // quotient has at most steps + 1 bits
        u128 D = p.d << steps;
        for (int i = 0; i <= steps; ++i) {
            q <<= 1;
            if (m >= D) {
                m -= D;
                q |= 1;
            }
            D >>= 1;
        }
    }
    const uint64_t ql = (uint64_t)q;
    return (int64_t)(neg ? (uint64_t)0 - ql : ql);
}

// ---- exact, order-free moments -------------------------------------------------------------------------------
// StandardDeviation's partials in fp64 (Welford / Chan) round differently for every cut of the rows (lanes,
// workgroups, chunks). The per-row doubles x = +-m * 2^e (m < 2^53) are instead also summed exactly: S1 = sum x in
// units of 2^-180 and S2 = sum x^2 in units of 2^-360, as signed 32-bit digits added into 64-bit counters on a fixed
// grid of 32-bit limbs (12 limbs for S1, 20 for S2: |x| of a decimal128 cell lies in [2^-127, 2^128) or is 0).
// Integer adds are exact in any order, so every cut of the rows gives the same (n, S1, S2), and avg = S1 / n,
// m2 = S2 - S1^2 / n are rounded once from exact rationals on the host.
constexpr int kMomS1Limbs = 12, kMomS2Limbs = 20, kMomLimbs = kMomS1Limbs + kMomS2Limbs;
constexpr int kMomS1Bias = 180, kMomS2Bias = 360;

// Calls add(limb index in [0, 32), signed value of |value| < 2^32) for every digit of x and x^2.
template <class Add>
DQ_HD void moment_digits(double x, Add add) {
    union { double d; uint64_t u; } c;
    c.d = x;
    const int E = (int)((c.u >> 52) & 0x7ff);
    if (E == 0) return;  // zero (a decimal128 cell never converts to a subnormal)
    const uint64_t m = (c.u & ((1ull << 52) - 1)) | (1ull << 52);
    const int e = E - 1075;
    const bool neg = (c.u >> 63) != 0;
    {
        const int p = e + kMomS1Bias, limb = p >> 5, sh = p & 31;
        const u128 v = (u128)m << sh;  // < 2^85
        for (int k = 0; k < 3; ++k) {
            const int64_t d = (int64_t)(uint32_t)(v >> (32 * k));
            add(limb + k, neg ? -d : d);
        }
    }
    {
        const u128 q = (u128)m * m;  // < 2^106
        const int p = 2 * e + kMomS2Bias, limb = kMomS1Limbs + (p >> 5), sh = p & 31;
        const uint64_t lo = (uint64_t)q, hi = (uint64_t)(q >> 64);
        const uint64_t v0 = lo << sh;
        const uint64_t v1 = (hi << sh) | (sh ? lo >> (64 - sh) : 0ull);
        const uint64_t v2 = sh ? hi >> (64 - sh) : 0ull;
        add(limb + 0, (int64_t)(uint32_t)v0);
        add(limb + 1, (int64_t)(v0 >> 32));
        add(limb + 2, (int64_t)(uint32_t)v1);
        add(limb + 3, (int64_t)(v1 >> 32));
        add(limb + 4, (int64_t)(uint32_t)v2);
    }
}

DQ_HD uint64_t bswap64(uint64_t x) { return __builtin_bswap64(x); }

// XXH64 with `seed` over the minimal big-endian two's-complement bytes of (hi:lo): java.math.BigInteger.toByteArray
// has bitLength / 8 + 1 bytes, where bitLength of a negative v is that of ~v (0 -> 00, -1 -> ff, 128 -> 00 80,
// -128 -> 80). The byte string is at most 16 bytes, so XXH64 runs its short-input tail only; the bytes are taken
// from two 64-bit words holding the string in memory order (the value shifted up to its top byte, byte-reversed).
DQ_HD uint64_t dec128_spark_hash(uint64_t lo, uint64_t hi, uint64_t seed) {
    const bool neg = (int64_t)hi < 0;
    const int bl = neg ? bit_length128(~lo, ~hi) : bit_length128(lo, hi);
    int rem = bl / 8 + 1;  // 1..16
    const u128 v = (((u128)hi << 64) | lo) << (8 * (16 - rem));
    const uint64_t w0 = bswap64((uint64_t)(v >> 64)), w1 = bswap64((uint64_t)v);
    uint64_t h = seed + P64_5 + (uint64_t)rem;
    uint64_t cur = w0;
    if (rem >= 8) {
        h ^= xxh_round(0, w0);
        h = rotl64(h, 27) * P64_1 + P64_4;
        cur = w1;
        rem -= 8;
        if (rem >= 8) {
            h ^= xxh_round(0, w1);
            h = rotl64(h, 27) * P64_1 + P64_4;
            cur = 0;
            rem -= 8;
        }
    }
    if (rem >= 4) {
        h ^= (cur & 0xffffffffull) * P64_1;
        h = rotl64(h, 23) * P64_2 + P64_3;
        cur >>= 32;
        rem -= 4;
    }
    for (; rem > 0; --rem) {
        h ^= (cur & 0xffull) * P64_5;
        h = rotl64(h, 11) * P64_1;
        cur >>= 8;
    }
    return xxh_fmix(h);
}

}  // namespace dq
