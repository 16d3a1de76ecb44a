// csv.hip — a CSV file's bytes, resident in HBM, into columns on gfx950 (Table.from_csv(path, device=...)).
//
// The dialect is csv.reader's default (',' delimiter, '"' quote, doubled-quote escape) and the typing is the host
// path's (_csv_infer / _csv_field_type in table.py); input csv.reader reads leniently is refused, never guessed
// (DESIGN.md §3i). q(i) = number of '"' bytes before byte i; byte i is outside quotes when q(i) is even.
//
//   1. csv_quotes_kernel   one workgroup per tile of kCsvTile bytes, one lane per 64 bytes: the lane's quote mask,
//                          the tile's quote count (rocPRIM exclusive scan -> the tile's starting parity) and the offset
//                          of the tile's last quote (the file's last is the unpaired one when the total is odd).
//   2. csv_mark_kernel     the same tiling: quote / comma / LF / CR masks of the lane's 64 bytes; the prefix-XOR
//                          ladder inside the word, a ballot of lane parities across the wave, LDS across the four
//                          waves and the tile's parity give "inside quotes" per byte. Out: one bit per byte for
//                          "LF outside quotes" (record terminator) and "comma outside quotes" (field delimiter), the
//                          tile's terminator count, and an atomicMin of the offending offset of each anomaly kind.
//                          The rules look one byte back and two ahead: those bytes come from memory, so lane and
//                          tile boundaries are no special case.
//   3. csv_rows_kernel     terminator positions scattered into row_start[records + 1] (tile bases from a scan).
//   4. csv_fields_kernel   one lane per record: walks the SET BITS of the delimiter bitmap between the record's
//                          bounds (not the bytes) for the first ncols field spans, reads each field once for its
//                          unquoted length and its class, writes the 8-byte span record, and reduces per column the
//                          class OR, the non-NULL count, the ambiguous count and the first ambiguous row (per wave
//                          by shuffles and ballots, per workgroup in LDS, then one global atomic per workgroup).
//   5. csv_lengths_kernel / csv_gather_kernel (STRING) and csv_parse_kernel (INT / LONG / DOUBLE / BOOLEAN): one
//                          column from its span records; validity words by wave ballot; the parsers are dq_parse.h's.
//
// Launch counts depend on neither the rows nor the bytes. Every load is bounds-checked against nbytes: the file buffer
// needs no padding.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include <rocprim/device/device_scan.hpp>

#include "dq_common.h"
#include "dq_internal.h"
#include "dq_parse.h"

namespace dq {

constexpr int kCsvBlock = 256;
constexpr int kCsvWaves = kCsvBlock / 64;
constexpr int kCsvTile = kCsvBlock * 64;  // bytes per workgroup (native.CSV_TILE_BYTES)
static_assert(kCsvTile == DQ_CSV_TILE_BYTES, "dq.h and the kernels disagree on the tile");

constexpr uint32_t kCsvNone = 0xFFFFFFFFu;

// Field classes (dq.h DQ_CSV_CLASS_*).
constexpr uint32_t kClsInt = DQ_CSV_CLASS_INT, kClsLong = DQ_CSV_CLASS_LONG, kClsDouble = DQ_CSV_CLASS_DOUBLE,
                   kClsBool = DQ_CSV_CLASS_BOOLEAN, kClsString = DQ_CSV_CLASS_STRING;

struct CsvMasks {
    uint64_t quote, comma, lf, cr;
};

// The masks of the 64 bytes at `base` (bit i = byte base + i); bytes at and past n read as 0.
__device__ __forceinline__ CsvMasks csv_load_masks(const uint8_t* __restrict__ data, int64_t base, int64_t n) {
    CsvMasks m = {0, 0, 0, 0};
    if (base + 64 <= n) {
        const uint4* p = reinterpret_cast<const uint4*>(data + base);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint4 q = p[v];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t c = (w[k] >> (8 * b)) & 0xFFu;
                    const int bit = v * 16 + k * 4 + b;
                    m.quote |= (uint64_t)(c == '"') << bit;
                    m.comma |= (uint64_t)(c == ',') << bit;
                    m.lf |= (uint64_t)(c == '\n') << bit;
                    m.cr |= (uint64_t)(c == '\r') << bit;
                }
            }
        }
    } else {
        for (int i = 0; i < 64 && base + i < n; ++i) {
            const uint32_t c = data[base + i];
            m.quote |= (uint64_t)(c == '"') << i;
            m.comma |= (uint64_t)(c == ',') << i;
            m.lf |= (uint64_t)(c == '\n') << i;
            m.cr |= (uint64_t)(c == '\r') << i;
        }
    }
    return m;
}

__device__ __forceinline__ uint32_t csv_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct CsvStatus {
    uint32_t anomaly[3];   // smallest offending offset of kinds 1..3 (kCsvNone: none)
    uint32_t pad;
};

// tile_quotes[t] = the quotes of tile t; tile_last[t] = the offset of its last quote + 1 (0: none). Plain stores: an
// atomicMax on one word from every wave of a file full of quotes serialises (2.35 ms of a 1e7-row file's 19.5 ms).
__global__ void __launch_bounds__(kCsvBlock)
csv_quotes_kernel(const uint8_t* __restrict__ data, int64_t n, uint32_t* __restrict__ tile_quotes,
                  uint32_t* __restrict__ tile_last) {
    __shared__ uint32_t wsum[kCsvWaves];
    __shared__ uint32_t wlast[kCsvWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = ((int64_t)blockIdx.x * kCsvBlock + threadIdx.x) * 64;
    uint64_t q = 0;
    if (base < n) q = csv_load_masks(data, base, n).quote;
    const uint32_t total = csv_wave_sum((uint32_t)__popcll(q));
    uint32_t last = q ? (uint32_t)(base + 63 - __clzll((long long)q)) + 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) last = max(last, (uint32_t)__shfl_xor(last, d, 64));
    if (lane == 0) {
        wsum[wave] = total;
        wlast[wave] = last;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0, l = 0;
        for (int k = 0; k < kCsvWaves; ++k) {
            t += wsum[k];
            l = max(l, wlast[k]);
        }
        tile_quotes[blockIdx.x] = t;
        tile_last[blockIdx.x] = l;
    }
}

__global__ void __launch_bounds__(kCsvBlock)
csv_mark_kernel(const uint8_t* __restrict__ data, int64_t n, const uint32_t* __restrict__ tile_quote_base,
                uint64_t* __restrict__ term_bits, uint64_t* __restrict__ delim_bits, uint32_t* __restrict__ tile_terms,
                CsvStatus* __restrict__ st) {
    __shared__ uint32_t wpar[kCsvWaves];
    __shared__ uint32_t wterm[kCsvWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t word = (int64_t)blockIdx.x * kCsvBlock + threadIdx.x;
    const int64_t base = word * 64;
    CsvMasks m = {0, 0, 0, 0};
    if (base < n) m = csv_load_masks(data, base, n);
    // parity of the quotes at and before each byte of the word, then across lanes, waves and tiles
    uint64_t p = m.quote;
    p ^= p << 1;
    p ^= p << 2;
    p ^= p << 4;
    p ^= p << 8;
    p ^= p << 16;
    p ^= p << 32;
    const unsigned long long odd = __ballot(__popcll(m.quote) & 1);
    if (lane == 0) wpar[wave] = (uint32_t)__popcll(odd) & 1u;
    __syncthreads();
    uint32_t carry = tile_quote_base[blockIdx.x] & 1u;
    for (int k = 0; k < wave; ++k) carry ^= wpar[k];
    carry ^= (uint32_t)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
    const uint64_t inside = (p << 1) ^ (carry ? ~0ull : 0ull);  // bit i: q(base + i) is odd
    const uint64_t term = m.lf & ~inside, delim = m.comma & ~inside;
    term_bits[word] = term;
    delim_bits[word] = delim;
    // the neighbours of the word: one byte back, two ahead
    const int64_t nx = base + 64;
    const uint32_t prev = base > 0 && base <= n ? data[base - 1] : 0x100u;  // 0x100: start of file
    const uint32_t next1 = nx < n ? data[nx] : 0x100u, next2 = nx + 1 < n ? data[nx + 1] : 0x100u;
    const uint64_t lf_follows = (m.lf >> 1) | ((uint64_t)(next1 == '\n') << 63);
    const uint64_t crlf = m.cr & lf_follows;
    // kind 1: an opening quote not at the start of the file and not after ',', LF or '"'
    const uint64_t prev_ok = ((m.comma | m.lf | m.quote) << 1) |
                             (uint64_t)(prev == 0x100u || prev == ',' || prev == '\n' || prev == '"');
    const uint64_t bad1 = m.quote & ~inside & ~prev_ok;
    // kind 2: a closing quote not before the end of the file, ',', LF, CR LF or '"'
    uint64_t ok = m.comma | m.lf | m.quote | crlf;
    if (n >= base && n < nx) ok |= 1ull << (n - base);
    const bool next_ok = nx >= n || next1 == ',' || next1 == '\n' || next1 == '"' || (next1 == '\r' && next2 == '\n');
    const uint64_t bad2 = m.quote & inside & ~((ok >> 1) | ((uint64_t)next_ok << 63));
    // kind 3: a CR outside quotes without an LF after it
    const uint64_t bad3 = m.cr & ~inside & ~lf_follows;
    if (__any((bad1 | bad2 | bad3) != 0)) {
        if (bad1) atomicMin(&st->anomaly[0], (uint32_t)(base + __ffsll((long long)bad1) - 1));
        if (bad2) atomicMin(&st->anomaly[1], (uint32_t)(base + __ffsll((long long)bad2) - 1));
        if (bad3) atomicMin(&st->anomaly[2], (uint32_t)(base + __ffsll((long long)bad3) - 1));
    }
    const uint32_t nterm = csv_wave_sum((uint32_t)__popcll(term));
    if (lane == 0) wterm[wave] = nterm;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < kCsvWaves; ++k) t += wterm[k];
        tile_terms[blockIdx.x] = t;
    }
}

// row_start[0] = 0, row_start[r + 1] = (position of terminator r) + 1; the caller sets the entry of a last record
// without a terminator.
__global__ void __launch_bounds__(kCsvBlock)
csv_rows_kernel(const uint64_t* __restrict__ term_bits, const uint32_t* __restrict__ tile_term_base,
                uint32_t* __restrict__ row_start) {
    __shared__ uint32_t wsum[kCsvWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t word = (int64_t)blockIdx.x * kCsvBlock + threadIdx.x;
    uint64_t t = term_bits[word];
    const uint32_t mine = (uint32_t)__popcll(t);
    uint32_t incl = mine;  // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t at = tile_term_base[blockIdx.x] + incl - mine;
    for (int k = 0; k < wave; ++k) at += wsum[k];
    if (word == 0) row_start[0] = 0;
    while (t) {
        const int b = __ffsll((long long)t) - 1;
        t &= t - 1;
        row_start[++at] = (uint32_t)(word * 64 + b + 1);
    }
}

struct CsvSpan {
    uint32_t start;  // first content byte (after the opening quote of a quoted field)
    uint32_t len;    // unquoted length (0: NULL) | kCsvEscaped when the content holds "" pairs
};
constexpr uint32_t kCsvEscaped = 0x80000000u;

struct CsvColumnStats {
    uint32_t classes;
    uint32_t pad;
    unsigned long long valid, ambiguous, first_ambiguous_row;
};

// The 8 bytes at p as one (unaligned) load, little-endian; `avail` >= 1 bytes are readable there, the rest read as 0.
__device__ __forceinline__ uint64_t csv_load8(const uint8_t* __restrict__ p, int64_t avail) {
    uint64_t w = 0;
    if (avail >= 8) {
        __builtin_memcpy(&w, p, 8);
    } else {
        for (int k = 0; k < (int)avail; ++k) w |= (uint64_t)p[k] << (8 * k);
    }
    return w;
}

__device__ __forceinline__ constexpr uint64_t csv_word(const char* s, int n) {
    uint64_t w = 0;
    for (int k = 0; k < n; ++k) w |= (uint64_t)(uint8_t)s[k] << (8 * k);
    return w;
}

// The class of the unquoted value of `len` content bytes at p (_csv_field_type for an ASCII value that does not end in
// LF), read 8 bytes a load (`avail` >= len bytes are readable at p); `nq` receives the quotes inside, `amb` whether the
// value holds a byte >= 0x80 or ends in LF.
__device__ uint32_t csv_classify(const uint8_t* __restrict__ p, int len, int64_t avail, int& nq, bool& amb) {
    enum { S0, SIGN, INT, INTDOT, FRAC, DOT, E, ESIGN, EXP, FAIL };
    int st = S0, quotes = 0, sig = 0;
    bool hi = false, neg = false;
    uint64_t v = 0, w0 = 0;
    uint32_t c = 0;
    for (int i = 0; i < len; i += 8) {
        uint64_t w = csv_load8(p + i, avail - i);
        if (i == 0) w0 = w;
        const int m = len - i < 8 ? len - i : 8;
        for (int k = 0; k < m; ++k, w >>= 8) {
            c = (uint32_t)w & 0xFFu;
            hi |= c >= 0x80;
            quotes += c == '"';
            const bool dig = c >= '0' && c <= '9';
            switch (st) {
                case S0:
                    if (c == '+' || c == '-') { st = SIGN; neg = c == '-'; }
                    else if (dig) st = INT;
                    else if (c == '.') st = DOT;
                    else st = FAIL;
                    break;
                case SIGN: st = dig ? INT : (c == '.' ? DOT : FAIL); break;
                case INT: st = dig ? INT : (c == '.' ? INTDOT : ((c == 'e' || c == 'E') ? E : FAIL)); break;
                case INTDOT:
                case FRAC: st = dig ? FRAC : ((c == 'e' || c == 'E') ? E : FAIL); break;
                case DOT: st = dig ? FRAC : FAIL; break;
                case E: st = dig ? EXP : ((c == '+' || c == '-') ? ESIGN : FAIL); break;
                case ESIGN:
                case EXP: st = dig ? EXP : FAIL; break;
                default: break;
            }
            if (st == INT && (sig > 0 || c != '0')) {  // significant digits of an integer (20 and more: beyond 64 bits)
                if (sig < 19) v = v * 10 + (c - '0');
                ++sig;
            }
        }
    }
    nq = quotes;
    amb = hi || (len > 0 && c == '\n');  // c: the last byte
    if (st == INT) {
        if (sig > 19) return kClsDouble;
        if (v < (1ull << 31) || (neg && v == (1ull << 31))) return kClsInt;
        if (v < (1ull << 63) || (neg && v == (1ull << 63))) return kClsLong;
        return kClsDouble;
    }
    if (st == INTDOT || st == FRAC || st == EXP) return kClsDouble;
    // the literals, from the first word (a byte >= 0x80 never equals a letter, with or without the case bit)
    if (len == 3 && (w0 & 0xFFFFFFull) == csv_word("NaN", 3)) return kClsDouble;
    if (len == 8 && w0 == csv_word("Infinity", 8)) return kClsDouble;
    if (len == 9 && w0 == csv_word("-Infinit", 8) && c == 'y') return kClsDouble;
    if (len == 4 && ((w0 | 0x20202020ull) & 0xFFFFFFFFull) == csv_word("true", 4)) return kClsBool;
    if (len == 5 && ((w0 | 0x2020202020ull) & 0xFFFFFFFFFFull) == csv_word("false", 5)) return kClsBool;
    return kClsString;
}

// Workgroups stride over tiles of kCsvBlock records and keep the per-column class OR and counts of the first lds_cols
// columns in LDS (3 words a column), flushed with one global atomic each at the end: one global atomic per wave and
// column on the same two cache lines bound the kernel (12.7 of a 1e7-row file's 17 ms). Columns past lds_cols go to
// global memory directly.
constexpr int kCsvLdsCols = 4096;

__global__ void __launch_bounds__(kCsvBlock)
csv_fields_kernel(const uint8_t* __restrict__ data, int64_t n, const uint64_t* __restrict__ delim_bits,
                  const uint32_t* __restrict__ row_start, int64_t nrows, int skip, int ncols, int lds_cols,
                  CsvSpan* __restrict__ spans, CsvColumnStats* __restrict__ stats) {
    extern __shared__ uint32_t acc[];  // [3 * lds_cols]: classes, non-NULL fields, ambiguous fields
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 3 * lds_cols; i += kCsvBlock) acc[i] = 0;
    __syncthreads();
    const int64_t ntiles = (nrows + kCsvBlock - 1) / kCsvBlock;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * kCsvBlock + threadIdx.x;
        const bool live = r < nrows;
        uint32_t s = 0, e = 0;
        if (live) {
            s = row_start[r + skip];
            e = row_start[r + skip + 1] - 1;
            if (e > s && data[e - 1] == '\r') --e;
        }
        uint32_t at = s;   // start of the next field
        bool more = live;  // the record still has a field at `at`
        for (int c = 0; c < ncols; ++c) {
            uint32_t cls = 0, ambig = 0, valid = 0;
            if (more) {
                // the next delimiter in [at, e): the first set bit of the bitmap from `at` on
                uint32_t fe = e;
                uint32_t w = at >> 6;
                uint64_t bits = at < e ? delim_bits[w] & (~0ull << (at & 63)) : 0ull;
                while (at < e) {
                    if (bits) {
                        const uint32_t d = (w << 6) + (uint32_t)__ffsll((long long)bits) - 1;
                        if (d < e) fe = d;
                        break;
                    }
                    if (((w + 1) << 6) >= e) break;
                    bits = delim_bits[++w];
                }
                uint32_t cs = at, ce = fe;
                if (ce > cs && data[cs] == '"') {  // quoted: the content between the enclosing quotes
                    ++cs;
                    ce = ce - 1 > cs ? ce - 1 : cs;
                }
                int nq = 0;
                bool amb = false;
                const uint32_t k = csv_classify(data + cs, (int)(ce - cs), n - (int64_t)cs, nq, amb);
                const uint32_t len = (ce - cs) - (uint32_t)(nq >> 1);
                spans[(int64_t)c * nrows + r] = CsvSpan{cs, len | (nq ? kCsvEscaped : 0u)};
                if (len) {
                    valid = 1;
                    if (amb) ambig = 1;
                    else cls = k;
                }
                more = fe < e;
                at = fe + 1;
            } else if (live) {
                spans[(int64_t)c * nrows + r] = CsvSpan{0, 0};
            }
            // per column: OR of the classes, counts, the first ambiguous row
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) cls |= __shfl_xor(cls, d, 64);
            const unsigned long long vb = __ballot(valid), ab = __ballot(ambig);
            if (lane == 0) {
                if (c < lds_cols) {
                    if (cls) atomicOr(&acc[3 * c], cls);
                    if (vb) atomicAdd(&acc[3 * c + 1], (uint32_t)__popcll(vb));
                    if (ab) atomicAdd(&acc[3 * c + 2], (uint32_t)__popcll(ab));
                } else {
                    if (cls) atomicOr(&stats[c].classes, cls);
                    if (vb) atomicAdd(&stats[c].valid, (unsigned long long)__popcll(vb));
                    if (ab) atomicAdd(&stats[c].ambiguous, (unsigned long long)__popcll(ab));
                }
                if (ab) atomicMin(&stats[c].first_ambiguous_row, (unsigned long long)(r + __ffsll((long long)ab) - 1));
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < lds_cols; c += kCsvBlock) {
        if (acc[3 * c]) atomicOr(&stats[c].classes, acc[3 * c]);
        if (acc[3 * c + 1]) atomicAdd(&stats[c].valid, (unsigned long long)acc[3 * c + 1]);
        if (acc[3 * c + 2]) atomicAdd(&stats[c].ambiguous, (unsigned long long)acc[3 * c + 2]);
    }
}

// lens[r] = the unquoted length of row r (lens[nrows] = 0) and the validity words.
__global__ void __launch_bounds__(kCsvBlock)
csv_lengths_kernel(const CsvSpan* __restrict__ spans, int64_t nrows, int32_t* __restrict__ lens,
                   uint64_t* __restrict__ validity) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kCsvBlock + threadIdx.x;
    const uint32_t len = r < nrows ? (spans[r].len & ~kCsvEscaped) : 0u;
    if (r <= nrows) lens[r] = (int32_t)len;
    const unsigned long long vb = __ballot(len != 0);
    if (validity && lane == 0 && (r >> 6) < ((nrows + 63) >> 6)) validity[r >> 6] = vb;
}

__global__ void __launch_bounds__(kCsvBlock)
csv_gather_kernel(const uint8_t* __restrict__ data, const CsvSpan* __restrict__ spans, int64_t nrows,
                  const int32_t* __restrict__ offsets, uint8_t* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kCsvBlock + threadIdx.x;
    if (r == nrows) {  // the read-past padding of the dword loads
        uint8_t* z = out + offsets[nrows];
        for (int k = 0; k < 16; ++k) z[k] = 0;
    }
    if (r >= nrows) return;
    const CsvSpan sp = spans[r];
    const uint32_t len = sp.len & ~kCsvEscaped;
    const uint8_t* src = data + sp.start;
    uint8_t* dst = out + offsets[r];
    if (!(sp.len & kCsvEscaped)) {
        for (uint32_t k = 0; k < len; ++k) dst[k] = src[k];
        return;
    }
    for (uint32_t k = 0; k < len; ++k) {  // "" -> "
        const uint8_t b = *src;
        dst[k] = b;
        src += b == '"' ? 2 : 1;
    }
}

// One typed column: T = int32_t / int64_t / double / uint8_t (BOOLEAN). *slow += the cells whose rounding the device
// parser cannot decide.
template <typename T>
__global__ void __launch_bounds__(kCsvBlock)
csv_parse_kernel(const uint8_t* __restrict__ data, const CsvSpan* __restrict__ spans, int64_t nrows,
                 T* __restrict__ out, uint64_t* __restrict__ validity, unsigned int* __restrict__ slow) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kCsvBlock + threadIdx.x;
    bool ok = false;
    if (r < nrows) {
        const CsvSpan sp = spans[r];
        const int len = (int)(sp.len & ~kCsvEscaped);
        const uint8_t* p = data + sp.start;
        T v = T(0);
        if (len > 0) {
            if constexpr (sizeof(T) == 1) {
                v = (T)((p[0] | 0x20) == 't');
                ok = true;
            } else if constexpr (std::is_floating_point<T>::value) {
                double d = 0.0;
                bool s = false;
                ok = java_parse_double(p, len, d, s);
                if (s) atomicAdd(slow, 1u);
                v = ok ? d : 0.0;
            } else {
                int64_t l = 0;
                ok = spark_string_to_long(p, len, l);
                v = ok ? (T)l : T(0);
                if (!ok) atomicAdd(slow, 1u);  // the class admitted only in-range integers: not reached
            }
        }
        out[r] = v;
    }
    const unsigned long long vb = __ballot(ok);
    if (validity && lane == 0 && (r >> 6) < ((nrows + 63) >> 6)) validity[r >> 6] = vb;
}

static int csv_blocks(int64_t n) { return (int)std::max<int64_t>(1, (n + kCsvBlock - 1) / kCsvBlock); }

}  // namespace dq

// The index of one file: the span records of its (row, column) cells, column-major.
struct dq_csv {
    const uint8_t* data;
    int64_t nbytes, nrows;
    int32_t ncols;
    dq::CsvSpan* spans;
    size_t spans_bytes;
};

extern "C" {

int dq_csv_index(dq_ctx* ctx, const uint8_t* bytes, int64_t nbytes, int32_t ncols, int32_t skip_records, dq_csv** out,
                 dq_csv_result* result, dq_csv_column_report* reports) {
    if (!ctx || !bytes || !out || !result || !reports || nbytes < 1 || ncols < 1 || skip_records < 0 || skip_records > 1)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_index: invalid arguments");
    *out = nullptr;
    memset(result, 0, sizeof(*result));
    memset(reports, 0, sizeof(*reports) * (size_t)ncols);
    if (dq::ctx_num_subs(ctx) != 0)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_csv_index: multi-device contexts are not supported");
    if (nbytes >= ((int64_t)1 << 31))
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_csv_index: files of 2^31 bytes and more are not supported");
    if ((uintptr_t)bytes & 15) return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_csv_index: the bytes must be 16-B aligned");
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::ScratchBuffers buf(ctx);
    const int64_t ntiles = (nbytes + dq::kCsvTile - 1) / dq::kCsvTile;
    const int64_t nwords = ntiles * dq::kCsvBlock;
    uint32_t *tile_quotes = nullptr, *tile_qbase = nullptr, *tile_terms = nullptr, *tile_tbase = nullptr, *tile_last = nullptr;
    uint64_t *term_bits = nullptr, *delim_bits = nullptr;
    dq::CsvStatus* dst = nullptr;
    const size_t tb_bytes = sizeof(uint32_t) * (size_t)(ntiles + 1);
    DQ_CTX_HIP(ctx, buf.alloc((void**)&tile_quotes, tb_bytes));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&tile_qbase, tb_bytes));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&tile_terms, tb_bytes));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&tile_tbase, tb_bytes));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&tile_last, tb_bytes));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&term_bits, sizeof(uint64_t) * (size_t)nwords));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&delim_bits, sizeof(uint64_t) * (size_t)nwords));
    DQ_CTX_HIP(ctx, buf.alloc((void**)&dst, sizeof(dq::CsvStatus)));
    dq::CsvStatus hst;
    memset(&hst, 0, sizeof(hst));
    hst.anomaly[0] = hst.anomaly[1] = hst.anomaly[2] = dq::kCsvNone;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(dst, &hst, sizeof(hst), hipMemcpyHostToDevice, s));
    DQ_CTX_HIP(ctx, hipMemsetAsync(tile_quotes + ntiles, 0, sizeof(uint32_t), s));
    DQ_CTX_HIP(ctx, hipMemsetAsync(tile_terms + ntiles, 0, sizeof(uint32_t), s));
    // 1. quote counts per tile -> the tiles' starting parities
    hipLaunchKernelGGL(dq::csv_quotes_kernel, dim3((unsigned)ntiles), dim3(dq::kCsvBlock), 0, s, bytes, nbytes, tile_quotes,
                       tile_last);
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_CSV_QUOTES]++;
    size_t tb = 0;
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, tile_quotes, tile_qbase, 0u, (size_t)(ntiles + 1),
                                            rocprim::plus<uint32_t>(), s));
    void* tmp = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc(&tmp, tb));
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(tmp, tb, tile_quotes, tile_qbase, 0u, (size_t)(ntiles + 1),
                                            rocprim::plus<uint32_t>(), s));
    // 2. terminator / delimiter bitmaps, anomalies, terminators per tile
    hipLaunchKernelGGL(dq::csv_mark_kernel, dim3((unsigned)ntiles), dim3(dq::kCsvBlock), 0, s, bytes, nbytes, tile_qbase,
                       term_bits, delim_bits, tile_terms, dst);
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_CSV_MARK]++;
    DQ_CTX_HIP(ctx, rocprim::exclusive_scan(tmp, tb, tile_terms, tile_tbase, 0u, (size_t)(ntiles + 1),
                                            rocprim::plus<uint32_t>(), s));
    uint32_t total_quotes = 0, nterm = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&total_quotes, tile_qbase + ntiles, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&nterm, tile_tbase + ntiles, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&hst, dst, sizeof(hst), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    // the refusal with the smallest offset (the lower kind on a tie); kind 4 sits at the unpaired (last) quote
    int64_t best = -1;
    int kind = 0;
    for (int k = 0; k < 3; ++k)
        if (hst.anomaly[k] != dq::kCsvNone && (best < 0 || (int64_t)hst.anomaly[k] < best)) {
            best = hst.anomaly[k];
            kind = k + 1;
        }
    if (total_quotes & 1u) {
        std::vector<uint32_t> last((size_t)ntiles);
        DQ_CTX_HIP(ctx, hipMemcpyAsync(last.data(), tile_last, sizeof(uint32_t) * (size_t)ntiles, hipMemcpyDeviceToHost, s));
        DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        int64_t at = -1;
        for (int64_t t = ntiles - 1; t >= 0 && at < 0; --t)
            if (last[(size_t)t]) at = (int64_t)last[(size_t)t] - 1;
        if (at >= 0 && (best < 0 || at < best)) {
            best = at;
            kind = 4;
        }
    }
    if (kind) {
        result->refusal_kind = kind;
        result->refusal_offset = best;
        return DQ_OK;
    }
    // 3. record starts
    uint32_t* row_start = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&row_start, sizeof(uint32_t) * ((size_t)nterm + 2)));
    hipLaunchKernelGGL(dq::csv_rows_kernel, dim3((unsigned)ntiles), dim3(dq::kCsvBlock), 0, s, term_bits, tile_tbase,
                       row_start);
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_CSV_ROWS]++;
    const uint32_t past = (uint32_t)nbytes + 1;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(row_start + nterm + 1, &past, sizeof(past), hipMemcpyHostToDevice, s));
    uint32_t last_start = 0;  // a last record without a terminator counts when it has at least one byte
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&last_start, row_start + nterm, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    const int64_t records = (int64_t)nterm + ((int64_t)last_start < nbytes ? 1 : 0);
    const int64_t nrows = std::max<int64_t>(records - skip_records, 0);
    result->nrows = nrows;
    dq_csv* h = new dq_csv();
    h->data = bytes;
    h->nbytes = nbytes;
    h->nrows = nrows;
    h->ncols = ncols;
    h->spans = nullptr;
    h->spans_bytes = 0;
    for (int c = 0; c < ncols; ++c) reports[c].first_ambiguous_row = -1;
    if (nrows == 0) {
        *out = h;
        return DQ_OK;
    }
    h->spans_bytes = sizeof(dq::CsvSpan) * (size_t)nrows * (size_t)ncols;
    h->spans = (dq::CsvSpan*)dq::scratch_alloc(ctx, h->spans_bytes);
    if (!h->spans) {
        delete h;
        return dq::ctx_fail(ctx, DQ_ERR_OUT_OF_MEMORY, "dq_csv_index: out of device memory for the span records");
    }
    // 4. field spans, classes and ambiguity reports
    dq::CsvColumnStats* dstats = nullptr;
    std::vector<dq::CsvColumnStats> hstats((size_t)ncols);
    for (auto& st : hstats) {
        memset(&st, 0, sizeof(st));
        st.first_ambiguous_row = ~0ull;
    }
    int rc = DQ_OK;
    do {
        if (buf.alloc((void**)&dstats, sizeof(dq::CsvColumnStats) * (size_t)ncols) != hipSuccess ||
            hipMemcpyAsync(dstats, hstats.data(), sizeof(dq::CsvColumnStats) * (size_t)ncols, hipMemcpyHostToDevice, s) !=
                hipSuccess) {
            rc = DQ_ERR_DEVICE;
            break;
        }
        const int lds_cols = std::min<int>(ncols, dq::kCsvLdsCols);
        const int grid = (int)std::min<int64_t>(dq::csv_blocks(nrows), (int64_t)dq::ctx_cus(ctx) * 8);
        hipLaunchKernelGGL(dq::csv_fields_kernel, dim3((unsigned)grid), dim3(dq::kCsvBlock),
                           sizeof(uint32_t) * 3 * (size_t)lds_cols, s, bytes, nbytes, delim_bits, row_start, nrows,
                           (int)skip_records, (int)ncols, lds_cols, h->spans, dstats);
        ctx->kernel_launches[DQ_KERNEL_CSV_FIELDS]++;
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(hstats.data(), dstats, sizeof(dq::CsvColumnStats) * (size_t)ncols, hipMemcpyDeviceToHost, s) !=
                hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            rc = DQ_ERR_DEVICE;
    } while (0);
    if (rc != DQ_OK) {
        dq::scratch_release(ctx, h->spans, h->spans_bytes);
        delete h;
        return dq::ctx_fail(ctx, rc, "dq_csv_index: the field pass failed on the device");
    }
    for (int c = 0; c < ncols; ++c) {
        reports[c].classes = (int32_t)hstats[c].classes;
        reports[c].valid = (int64_t)hstats[c].valid;
        reports[c].ambiguous = (int64_t)hstats[c].ambiguous;
        reports[c].first_ambiguous_row = hstats[c].ambiguous ? (int64_t)hstats[c].first_ambiguous_row : -1;
    }
    *out = h;
    return DQ_OK;
}

int dq_csv_field(dq_ctx* ctx, const dq_csv* csv, int64_t row, int32_t col, int64_t* start, int32_t* length,
                 int32_t* escaped) {
    if (!ctx || !csv || !start || !length || !escaped || row < 0 || row >= csv->nrows || col < 0 || col >= csv->ncols)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_field: invalid arguments");
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    dq::CsvSpan sp;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&sp, csv->spans + (int64_t)col * csv->nrows + row, sizeof(sp), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    *start = sp.start;
    *length = (int32_t)(sp.len & ~dq::kCsvEscaped);
    *escaped = (sp.len & dq::kCsvEscaped) ? 1 : 0;
    return DQ_OK;
}

int dq_csv_column(dq_ctx* ctx, const dq_csv* csv, int32_t col, int32_t spark_type, void* out_values, uint8_t* out_validity,
                  int32_t* out_offsets, int64_t* out_bytes) {
    if (!ctx || !csv || col < 0 || col >= csv->ncols)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_column: invalid arguments");
    if (dq::ctx_num_subs(ctx) != 0)
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_csv_column: multi-device contexts are not supported");
    const bool is_string = spark_type == DQ_TYPE_STRING;
    int esize = 0;
    switch (spark_type) {
        case DQ_TYPE_STRING: esize = 1; break;
        case DQ_TYPE_BOOLEAN: esize = 1; break;
        case DQ_TYPE_INT: esize = 4; break;
        case DQ_TYPE_LONG:
        case DQ_TYPE_DOUBLE: esize = 8; break;
        default: return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, "dq_csv_column: the type must be STRING, BOOLEAN, INT, LONG or DOUBLE");
    }
    if (is_string && (!out_offsets || !out_bytes))
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_column: a string column needs out_offsets and out_bytes");
    if (!is_string && csv->nrows > 0 && !out_values)
        return dq::ctx_fail(ctx, DQ_ERR_INVALID_ARGUMENT, "dq_csv_column: no output buffer");
    if (((uintptr_t)out_validity & 7) || ((uintptr_t)out_offsets & 3) ||
        (!is_string && ((uintptr_t)out_values & (uintptr_t)(esize - 1))))
        return dq::ctx_fail(ctx, DQ_ERR_ALIGNMENT, "dq_csv_column: misaligned buffer");
    if (out_bytes) *out_bytes = 0;
    const int64_t nrows = csv->nrows;
    DQ_CTX_HIP(ctx, hipSetDevice(dq::ctx_device(ctx)));
    hipStream_t s = dq::ctx_stream(ctx);
    if (nrows == 0) {
        if (is_string) {
            if (!out_values) DQ_CTX_HIP(ctx, hipMemsetAsync(out_offsets, 0, sizeof(int32_t), s));
            else DQ_CTX_HIP(ctx, hipMemsetAsync(out_values, 0, 16, s));
            DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        }
        return DQ_OK;
    }
    dq::ScratchBuffers buf(ctx);
    const dq::CsvSpan* spans = csv->spans + (int64_t)col * nrows;
    uint64_t* ov = (uint64_t*)out_validity;
    if (is_string && !out_values) {  // sizing call: offsets, validity, total bytes
        int32_t* lens = nullptr;
        DQ_CTX_HIP(ctx, buf.alloc((void**)&lens, sizeof(int32_t) * (size_t)(nrows + 1)));
        hipLaunchKernelGGL(dq::csv_lengths_kernel, dim3((unsigned)dq::csv_blocks(nrows + 1)), dim3(dq::kCsvBlock), 0, s, spans,
                           nrows, lens, ov);
        DQ_CTX_HIP(ctx, hipGetLastError());
        ctx->kernel_launches[DQ_KERNEL_CSV_COLUMN]++;
        size_t tb = 0;
        DQ_CTX_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, lens, out_offsets, 0, (size_t)(nrows + 1), rocprim::plus<int32_t>(), s));
        void* tmp = nullptr;
        DQ_CTX_HIP(ctx, buf.alloc(&tmp, tb));
        DQ_CTX_HIP(ctx, rocprim::exclusive_scan(tmp, tb, lens, out_offsets, 0, (size_t)(nrows + 1), rocprim::plus<int32_t>(), s));
        int32_t total = 0;
        DQ_CTX_HIP(ctx, hipMemcpyAsync(&total, out_offsets + nrows, sizeof(total), hipMemcpyDeviceToHost, s));
        DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        *out_bytes = total;
        return DQ_OK;
    }
    if (is_string) {  // copy call: out_offsets holds the sizing call's offsets; out_values has their total + 16 bytes
        hipLaunchKernelGGL(dq::csv_gather_kernel, dim3((unsigned)dq::csv_blocks(nrows + 1)), dim3(dq::kCsvBlock), 0, s,
                           csv->data, spans, nrows, out_offsets, (uint8_t*)out_values);
        DQ_CTX_HIP(ctx, hipGetLastError());
        ctx->kernel_launches[DQ_KERNEL_CSV_COLUMN]++;
        int32_t total = 0;
        DQ_CTX_HIP(ctx, hipMemcpyAsync(&total, out_offsets + nrows, sizeof(total), hipMemcpyDeviceToHost, s));
        DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
        *out_bytes = total;
        return DQ_OK;
    }
    unsigned int* dslow = nullptr;
    DQ_CTX_HIP(ctx, buf.alloc((void**)&dslow, sizeof(unsigned int)));
    DQ_CTX_HIP(ctx, hipMemsetAsync(dslow, 0, sizeof(unsigned int), s));
    const dim3 g((unsigned)dq::csv_blocks(nrows)), b(dq::kCsvBlock);
    switch (spark_type) {
        case DQ_TYPE_BOOLEAN: hipLaunchKernelGGL(dq::csv_parse_kernel<uint8_t>, g, b, 0, s, csv->data, spans, nrows, (uint8_t*)out_values, ov, dslow); break;
        case DQ_TYPE_INT: hipLaunchKernelGGL(dq::csv_parse_kernel<int32_t>, g, b, 0, s, csv->data, spans, nrows, (int32_t*)out_values, ov, dslow); break;
        case DQ_TYPE_LONG: hipLaunchKernelGGL(dq::csv_parse_kernel<int64_t>, g, b, 0, s, csv->data, spans, nrows, (int64_t*)out_values, ov, dslow); break;
        default: hipLaunchKernelGGL(dq::csv_parse_kernel<double>, g, b, 0, s, csv->data, spans, nrows, (double*)out_values, ov, dslow); break;
    }
    DQ_CTX_HIP(ctx, hipGetLastError());
    ctx->kernel_launches[DQ_KERNEL_CSV_COLUMN]++;
    unsigned int hslow = 0;
    DQ_CTX_HIP(ctx, hipMemcpyAsync(&hslow, dslow, sizeof(hslow), hipMemcpyDeviceToHost, s));
    DQ_CTX_HIP(ctx, hipStreamSynchronize(s));
    if (hslow) {
        char msg[256];
        snprintf(msg, sizeof(msg),
                 "dq_csv_column: %u cells of column %d need the arbitrary-precision path of a correctly rounded parse "
                 "(more than 19 significant digits on a rounding boundary), or do not fit the column's type",
                 hslow, (int)col);
        return dq::ctx_fail(ctx, DQ_ERR_UNSUPPORTED, msg);
    }
    return DQ_OK;
}

void dq_csv_free(dq_ctx* ctx, dq_csv* csv) {
    if (!csv) return;
    if (csv->spans && ctx) dq::scratch_release(ctx, csv->spans, csv->spans_bytes);
    delete csv;
}

}  // extern "C"
