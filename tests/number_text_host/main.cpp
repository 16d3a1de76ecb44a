// Host build (-DDQ_HOST_ONLY, no HIP) of the device number <-> text routines (deequ_amd/csrc/dq_parse.h,
// java_dtoa.h), driven by tests/test_number_text_host.py. One case per stdin line, one answer per stdout line:
//   P <string bytes in hex>   ->  <ok 0|1> <slow 0|1> <double bits, 16 hex digits>      java_parse_double
//   L <string bytes in hex>   ->  <ok 0|1> <value>                                      spark_string_to_long
//   D <double bits in hex>    ->  the text of java_double_to_chars
//   F <float bits in hex>     ->  the text of java_float_to_chars
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dq_parse.h"
#include "java_dtoa.h"

static int unhex(const char* s, uint8_t* out, int cap) {
    int n = 0;
    for (; s[0] && s[1] && s[0] != '\n' && n < cap; s += 2) {
        unsigned v;
        if (sscanf(s, "%2x", &v) != 1) return -1;
        out[n++] = (uint8_t)v;
    }
    return n;
}

int main() {
    static char line[4096];
    static uint8_t bytes[2048];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == 0 || line[1] != ' ') continue;
        const char kind = line[0];
        if (kind == 'P' || kind == 'L') {
            const int n = unhex(line + 2, bytes, (int)sizeof bytes);
            if (n < 0) return 2;
            if (kind == 'P') {
                double d = 0.0;
                bool slow = false;
                const bool ok = dq::java_parse_double(bytes, n, d, slow);
                printf("%d %d %016llx\n", ok ? 1 : 0, slow ? 1 : 0, (unsigned long long)(ok ? dq::parse_double_bits(d) : 0));
            } else {
                int64_t v = 0;
                const bool ok = dq::spark_string_to_long(bytes, n, v);
                printf("%d %lld\n", ok ? 1 : 0, (long long)(ok ? v : 0));
            }
        } else if (kind == 'D' || kind == 'F') {
            const unsigned long long u = strtoull(line + 2, nullptr, 16);
            uint8_t buf[32];
            int n;
            if (kind == 'D') {
                n = dq::java_double_to_chars(dq::parse_bits_double((uint64_t)u), buf);
            } else {
                union { uint32_t u; float f; } c;
                c.u = (uint32_t)u;
                n = dq::java_float_to_chars(c.f, buf);
            }
            fwrite(buf, 1, (size_t)n, stdout);
            fputc('\n', stdout);
        } else {
            return 2;
        }
    }
    return 0;
}
