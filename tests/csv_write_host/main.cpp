// Host build (-DDQ_HOST_ONLY, no HIP) of the CSV writer's per-cell code (deequ_amd/csrc/dq_csv_cell.h over dq_format.h
// and java_dtoa.h), driven by tests/test_csv_write_host.py. One case per stdin line, one answer per stdout line:
//   T <spark type> <decimal scale> <the cell's bits, hex>  ->  the text of csv_typed_text
//   S <string bytes in hex, or "-" for the empty string>   ->  <quoted 0|1> <quotes> <file length> <the cell as written, hex>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dq_csv_cell.h"

int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == 'T') {
            int type = 0, scale = 0;
            unsigned long long bits = 0;
            if (sscanf(line + 1, "%d %d %llx", &type, &scale, &bits) != 3) return 2;
            uint64_t cell = bits;  // little-endian: the low bytes are the narrow types' value
            uint8_t buf[dq::kCsvCellText];
            const int n = dq::csv_typed_text(type, &cell, 0, scale, buf);
            if (n < 0 || n > dq::kCsvCellText) return 3;
            fwrite(buf, 1, (size_t)n, stdout);
            fputc('\n', stdout);
        } else if (line[0] == 'S') {
            std::vector<uint8_t> s;
            for (const char* p = line + 2; p[0] && p[1] && p[0] != '\n' && p[0] != '-'; p += 2) {
                unsigned v;
                if (sscanf(p, "%2x", &v) != 1) return 2;
                s.push_back((uint8_t)v);
            }
            int64_t quotes = 0;
            const bool quoted = dq::csv_needs_quotes(s.data(), (int64_t)s.size(), &quotes);
            const int64_t len = dq::csv_quoted_length((int64_t)s.size(), quoted, quotes);
            std::vector<uint8_t> out((size_t)len + 1, 0xEE);  // one guard byte past the cell
            if (quoted) {
                if (dq::csv_quoted_copy(out.data(), s.data(), (int64_t)s.size()) != len) return 4;
            } else if (len) {
                memcpy(out.data(), s.data(), (size_t)len);
            }
            if (out[(size_t)len] != 0xEE) return 5;
            printf("%d %lld %lld ", quoted ? 1 : 0, (long long)quotes, (long long)len);
            for (int64_t i = 0; i < len; ++i) printf("%02x", out[(size_t)i]);
            fputc('\n', stdout);
        } else {
            return 2;
        }
    }
    return 0;
}
