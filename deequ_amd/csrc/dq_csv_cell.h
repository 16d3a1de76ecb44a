// dq_csv_cell.h — one cell of the CSV writer (host + device code): the text of a typed cell, the quoting
// decision of a STRING cell, its quoted length and the quoted copy. csv_write.hip calls these from its kernels; a
// host-only build (-DDQ_HOST_ONLY, no HIP: tests/csv_write_host/) runs the same code against the model.
//
// A non-NULL cell's text is Spark 2.2's Cast(x AS STRING). A STRING cell is its bytes, enclosed in quotes with every
// '"' doubled iff it holds ',', '"', LF or CR or is empty; no other cell is ever quoted. A NULL cell is zero bytes.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/dq.h"
#include "dq_format.h"
#include "java_dtoa.h"

namespace dq {

constexpr int kCsvCellText = 40;  // bytes a typed cell's text needs at the most (a TIMESTAMP of a six-digit year: 29)

// The byte forces quotes around its cell.
DQ_HD bool csv_special_byte(uint32_t c) { return c == ',' || c == '"' || c == '\n' || c == '\r'; }

// The text of row `row` of a fixed-width column into buf (kCsvCellText bytes); its length, -1 for a type that has no
// text here (STRING, DECIMAL128).
DQ_HD int csv_typed_text(int spark_type, const void* values, int64_t row, int decimal_scale, uint8_t* buf) {
    switch (spark_type) {
        case DQ_TYPE_BOOLEAN: {
            const bool v = static_cast<const uint8_t*>(values)[row] != 0;
            const char* s = v ? "true" : "false";
            const int n = v ? 4 : 5;
            for (int k = 0; k < n; ++k) buf[k] = (uint8_t)s[k];
            return n;
        }
        case DQ_TYPE_BYTE: return rx::format_long(static_cast<const int8_t*>(values)[row], buf);
        case DQ_TYPE_SHORT: return rx::format_long(static_cast<const int16_t*>(values)[row], buf);
        case DQ_TYPE_INT: return rx::format_long(static_cast<const int32_t*>(values)[row], buf);
        case DQ_TYPE_LONG: return rx::format_long(static_cast<const int64_t*>(values)[row], buf);
        case DQ_TYPE_FLOAT: return java_float_to_chars(static_cast<const float*>(values)[row], buf);
        case DQ_TYPE_DOUBLE: return java_double_to_chars(static_cast<const double*>(values)[row], buf);
        case DQ_TYPE_DECIMAL: return rx::format_decimal(static_cast<const int64_t*>(values)[row], decimal_scale, buf);
        case DQ_TYPE_DATE: return rx::format_date_days(static_cast<const int32_t*>(values)[row], buf);
        case DQ_TYPE_TIMESTAMP: return rx::format_timestamp_utc(static_cast<const int64_t*>(values)[row], buf);
        default: return -1;
    }
}

// Whether the `len` bytes at s are written in quotes; *quotes receives the '"' bytes among them.
DQ_HD bool csv_needs_quotes(const uint8_t* s, int64_t len, int64_t* quotes) {
    bool special = len == 0;
    int64_t nq = 0;
    for (int64_t i = 0; i < len; ++i) {
        special |= csv_special_byte(s[i]);
        nq += s[i] == '"';
    }
    *quotes = nq;
    return special;
}

// The bytes a STRING cell of `len` bytes with `quotes` '"' bytes takes in the file.
DQ_HD int64_t csv_quoted_length(int64_t len, bool quoted, int64_t quotes) { return quoted ? len + quotes + 2 : len; }

// The cell in quotes, every '"' doubled; returns the bytes written (csv_quoted_length).
DQ_HD int64_t csv_quoted_copy(uint8_t* dst, const uint8_t* s, int64_t len) {
    int64_t n = 0;
    dst[n++] = '"';
    for (int64_t i = 0; i < len; ++i) {
        const uint8_t b = s[i];
        dst[n++] = b;
        if (b == '"') dst[n++] = '"';
    }
    dst[n++] = '"';
    return n;
}

}  // namespace dq
