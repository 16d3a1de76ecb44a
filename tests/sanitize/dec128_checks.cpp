// Host-only checks of deequ_amd/csrc/dq_dec128.h under AddressSanitizer + UndefinedBehaviorSanitizer: the 192-bit
// accumulate, the signed 128-bit compare, and -- against expected values the caller computed with an exact model
// (tests/decimal128_model.py) -- dec128_to_double, Decimal.toLong and Spark's hash of every case of the file named
// by argv[1]. One case per line, hexadecimal: lo hi scale double-bits long-bits hash. The hash is also checked
// against xxh_bytes over an independently built java.math.BigInteger.toByteArray. Exit 0 = every check held.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../deequ_amd/csrc/dq_dec128.h"

using namespace dq;

static int failures = 0;
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            if (failures < 20) fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                            \
        }                                                                          \
    } while (0)

static uint64_t bits_of(double d) {
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}

// BigInteger.toByteArray, byte by byte: drop leading sign bytes while the next byte keeps the sign.
static int java_bytes(uint64_t lo, uint64_t hi, uint8_t* out) {
    uint8_t be[16];
    for (int i = 0; i < 8; ++i) {
        be[i] = (uint8_t)(hi >> (56 - 8 * i));
        be[8 + i] = (uint8_t)(lo >> (56 - 8 * i));
    }
    const uint8_t sign = (be[0] & 0x80) ? 0xff : 0x00;
    int first = 0;
    while (first < 15 && be[first] == sign && ((be[first + 1] & 0x80) == (sign & 0x80))) ++first;
    memcpy(out, be + first, 16 - first);
    return 16 - first;
}

static void check_acc192() {
    Acc192 a;
    acc192_zero(a);
    acc192_add128(a, ~0ull, 0);  // 2^64 - 1
    acc192_add128(a, 1, 0);      // carry into limb 1
    CHECK(a.w[0] == 0 && a.w[1] == 1 && a.w[2] == 0);
    acc192_add128(a, ~0ull, ~0ull);  // -1: borrow back through limb 0
    CHECK(a.w[0] == ~0ull && a.w[1] == 0 && a.w[2] == 0);
    acc192_zero(a);
    acc192_add128(a, ~0ull, 0x7fffffffffffffffull);  // 2^127 - 1, twice: carry into limb 2
    acc192_add128(a, ~0ull, 0x7fffffffffffffffull);
    CHECK(a.w[0] == ~0ull - 1 && a.w[1] == ~0ull && a.w[2] == 0);
    acc192_add128(a, 2, 0);
    CHECK(a.w[0] == 0 && a.w[1] == 0 && a.w[2] == 1);
    acc192_zero(a);
    acc192_add128(a, 0, 0x8000000000000000ull);  // -2^127, twice
    acc192_add128(a, 0, 0x8000000000000000ull);
    CHECK(a.w[0] == 0 && a.w[1] == 0 && a.w[2] == ~0ull);
    Acc192 b = a;
    acc192_add(a, b);  // -2^129
    CHECK(a.w[0] == 0 && a.w[1] == 0 && a.w[2] == ~0ull - 1);
    // 10^38 is the first overflowing total, on both sides
    const u128 lim = pow10_u128(38);
    Acc192 t;
    acc192_zero(t);
    acc192_add128(t, (uint64_t)(lim - 1), (uint64_t)((lim - 1) >> 64));
    CHECK(!acc192_overflows_38(t));
    acc192_add128(t, 1, 0);
    CHECK(acc192_overflows_38(t));
    acc192_zero(t);
    const u128 nl = (u128)0 - lim;
    acc192_add128(t, (uint64_t)nl, (uint64_t)(nl >> 64));
    CHECK(acc192_overflows_38(t));
    acc192_add128(t, 1, 0);
    CHECK(!acc192_overflows_38(t));
    // compare
    CHECK(dec128_less(~0ull, ~0ull, 0, 0));                       // -1 < 0
    CHECK(!dec128_less(0, 0, ~0ull, ~0ull));
    CHECK(dec128_less(0, 0x8000000000000000ull, ~0ull, ~0ull));   // min < -1
    CHECK(dec128_less(~0ull, 0, 0, 1));                           // 2^64 - 1 < 2^64
    CHECK(!dec128_less(5, 7, 5, 7));
}

int main(int argc, char** argv) {
    check_acc192();
    long ncases = 0;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        uint64_t lo, hi, db, lb, hb;
        int scale;
        while (fscanf(f, "%" SCNx64 " %" SCNx64 " %d %" SCNx64 " %" SCNx64 " %" SCNx64, &lo, &hi, &scale, &db, &lb, &hb) == 6) {
            ++ncases;
            const uint64_t got = bits_of(dec128_to_double(lo, hi, scale));
            if (got != db && failures < 20)
                fprintf(stderr, "to_double(%016" PRIx64 ":%016" PRIx64 ", %d) = %016" PRIx64 ", expected %016" PRIx64 "\n", hi, lo,
                        scale, got, db);
            CHECK(got == db);
            {  // the exact-moment digits of that double: in range, and S1's three digits rebuild +-m << shift
                double dv;
                memcpy(&dv, &got, 8);
                int calls = 0, first = -1;
                u128 s1 = 0;
                bool negd = false;
                moment_digits(dv, [&](int limb, int64_t d) {
                    CHECK(limb >= 0 && limb < kMomLimbs && d > -(1ll << 32) && d < (1ll << 32));
                    if (calls < 3) {
                        if (calls == 0) first = limb;
                        CHECK(limb == first + calls && limb < kMomS1Limbs);
                        negd |= d < 0;
                        s1 |= (u128)(uint64_t)(d < 0 ? -d : d) << (32 * calls);
                    } else {
                        CHECK(limb >= kMomS1Limbs && d >= 0);
                    }
                    ++calls;
                });
                const int E = (int)((got >> 52) & 0x7ff);
                if (E == 0) {
                    CHECK(calls == 0);
                } else {
                    const uint64_t m = (got & ((1ull << 52) - 1)) | (1ull << 52);
                    const int p = E - 1075 + kMomS1Bias;
                    CHECK(calls == 8 && first == (p >> 5) && s1 == ((u128)m << (p & 31)) && negd == ((got >> 63) != 0));
                }
            }
            CHECK((uint64_t)dec128_to_long_scaled(lo, hi, dec128_scale(scale)) == lb);
            const uint64_t h = dec128_spark_hash(lo, hi, SPARK_HLL_SEED);
            CHECK(h == hb);
            uint8_t jb[16];
            const int n = java_bytes(lo, hi, jb);
            CHECK(h == xxh_bytes(jb, n, SPARK_HLL_SEED));
        }
        fclose(f);
    }
    if (failures) {
        fprintf(stderr, "dec128_checks: %d failures\n", failures);
        return 1;
    }
    printf("dec128_checks: ok %ld cases\n", ncases);
    return 0;
}
