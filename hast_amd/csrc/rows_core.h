// rows_core.h -- the rules of `classify`'s output table (printBarcodeInfos, classify.cpp:93-102) and of the three barcode lists of
// --phase-reads, once: the order of the rows, the call of a barcode, the text of a row.  Plain integer and double code: the kernels
// (rows_kernels.hip), the host model (rows_host.h) and tests/native/test_rows_core.cpp step the same functions, so that the table
// `classify --rows device` formats in HBM and the one the host threads format can never disagree.
//
// A barcode is a text record of 16 bytes, as the device dictionary keeps them by id (name_claim.h): rec[0] = its length (0..15),
// rec[1 .. 1 + length) its text; what lies behind the text is not looked at.
//
// FLOATING POINT.  row_hap divides and multiplies doubles and compares the products, exactly as hast_get_hap (hast_api.cpp) does on the
// host.  The two agree bit for bit only because the device's f64 divide is IEEE (correctly rounded): the Makefile passes no fast-math
// flag (-ffast-math, -fhip-fp32-correctly-rounded-divide-sqrt is about f32 only, -munsafe-fp-atomics is about atomics) and none may
// be added to the rule of rows_kernels.o; nor is there an fma to contract, a multiply follows a divide.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROWS_HD __host__ __device__ __forceinline__
#else
#define ROWS_HD inline
#endif

namespace hast {
namespace rows {

constexpr uint32_t kMaxText = 15;
constexpr uint32_t kMaxRow = kMaxText + 1 + 2 + 1 + 20 + 1 + 20 + 1;      // text \t -1 \t 2^64-1 \t 2^64-1 \n = 61
constexpr uint32_t kMaxLine = kMaxText + 1;                               // a list line: text \n

struct Key {
    uint64_t hi, lo;
};

ROWS_HD uint32_t text_len(const uint8_t rec[16]) { return rec[0] < kMaxText ? rec[0] : kMaxText; }

// THE ORDER.  key = the 15 text bytes, zero padded, as one big-endian number, and behind them the length byte: 128 bits, hi = text
// bytes 0..7, lo = text bytes 8..14 and the length.  Unsigned order on (hi, lo) is the order of sort_rows (classify_main.cpp), that
// of std::map<std::string>: byte-wise lexicographic with unsigned bytes, a prefix in front of what it is a prefix of.  For two
// different texts A (a bytes) and B (b bytes), a <= b:
//   * they first differ at a position p < a, inside both: the padded keys agree in the bytes in front of p and differ in byte p, which
//     is A[p] against B[p] -- the byte that decides the lexicographic order decides the keys, the more significant one.
//   * A is a prefix of B (a < b).  A sorts first.  The keys agree in bytes 0 .. a-1; behind them A's key holds padding zeros and B's
//     holds B[a .. b).  If one of those is not 0x00, the first such byte makes B's key the larger one: the zeros lose.  If they are
//     all 0x00 ("ab" against "ab\0"), all 15 text bytes of the keys agree and the length byte, the least significant one, decides:
//     a < b, A first.
//   * equal texts have equal keys, and only they: the length byte tells texts apart that differ only in trailing 0x00 bytes.
// Ids are one per text, so no two rows have the same 128-bit key: the ORDER has no ties for a sort to break.  The device's sort of it
// does: it is two 64-bit passes, by lo and then by hi (rows_api.cpp), and the pass by hi must be stable -- rows with the same first
// eight bytes have equal keys there and keep the order the pass by lo left.  Never an unstable sort in its place.
ROWS_HD Key row_key(const uint8_t rec[16]) {
    const uint32_t n = text_len(rec);
    Key k = {0, 0};
    for (uint32_t i = 0; i < 8; ++i) k.hi = (k.hi << 8) | (i < n ? rec[1 + i] : 0u);
    for (uint32_t i = 8; i < kMaxText; ++i) k.lo = (k.lo << 8) | (i < n ? rec[1 + i] : 0u);
    k.lo = (k.lo << 8) | n;
    return k;
}

// THE CALL (getHap, classify.cpp:66-86; hast_get_hap): 0, 1 or -1.  The same sequence of double operations: convert, divide, multiply,
// two compares.
ROWS_HD int row_hap(const uint8_t rec[16], uint64_t c0, uint64_t c1, uint64_t n0, uint64_t n1, double w0, double w1) {
    const uint32_t n = text_len(rec);
    const uint8_t *t = rec + 1;
    if ((n == 5 && t[0] == '0' && t[1] == '_' && t[2] == '0' && t[3] == '_' && t[4] == '0') || (n == 3 && t[0] == '0' && t[1] == '_' && t[2] == '0') ||
        (n == 1 && t[0] == '0'))
        return -1;
    if (c0 > 0 && c1 > 0) {
        double df0 = double(c0) / double(n0);
        double df1 = double(c1) / double(n1);
        df0 *= w0;
        df1 *= w1;
        if (df0 > df1) return 0;
        if (df1 > df0) return 1;
        return -1;
    }
    if (c0 > 0) return 0;
    if (c1 > 0) return 1;
    return -1;
}

// the list of --phase-reads a call puts its barcode on: 1 paternal (hap 0), 2 maternal (hap 1), 3 homozygous (-1), as write_lists does
ROWS_HD uint32_t row_list(int hap) { return hap == 0 ? 1u : hap == 1 ? 2u : 3u; }

// a barcode that itself holds '#' or '/': awk cuts its list line short, the router is the host's then
ROWS_HD bool has_sep(const uint8_t rec[16]) {
    const uint32_t n = text_len(rec);
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) any = any || rec[1 + i] == '#' || rec[1 + i] == '/';
    return any;
}

// decimal digits of v: 1 .. 20
ROWS_HD uint32_t dec_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}
// v in decimal at p; returns the digits written.  P: anything indexable that takes bytes (the kernels pass a pointer into LDS)
template <class P> ROWS_HD uint32_t put_dec(P p, uint64_t v) {
    const uint32_t n = dec_len(v);
    for (uint32_t i = n; i-- > 0;) {
        p[i] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return n;
}

// text \t hap \t c0 \t c1 \n, -1 for hap < 0; the counts in full (the reference prints `int`: the same digits up to INT_MAX)
ROWS_HD uint32_t row_len(const uint8_t rec[16], int hap, uint64_t c0, uint64_t c1) {
    return text_len(rec) + 1 + (hap < 0 ? 2u : 1u) + 1 + dec_len(c0) + 1 + dec_len(c1) + 1;
}
template <class P> ROWS_HD uint32_t put_row(P p, const uint8_t rec[16], int hap, uint64_t c0, uint64_t c1) {
    const uint32_t n = text_len(rec);
    uint32_t at = 0;
    for (uint32_t i = 0; i < n; ++i) p[at++] = rec[1 + i];
    p[at++] = '\t';
    if (hap < 0) {
        p[at++] = '-';
        p[at++] = '1';
    } else
        p[at++] = (uint8_t)('0' + hap);
    p[at++] = '\t';
    at += put_dec(p + at, c0);
    p[at++] = '\t';
    at += put_dec(p + at, c1);
    p[at++] = '\n';
    return at;
}
// a list line: text \n
ROWS_HD uint32_t line_len(const uint8_t rec[16]) { return text_len(rec) + 1; }
template <class P> ROWS_HD uint32_t put_line(P p, const uint8_t rec[16]) {
    const uint32_t n = text_len(rec);
    for (uint32_t i = 0; i < n; ++i) p[i] = rec[1 + i];
    p[n] = '\n';
    return n + 1;
}

ROWS_HD bool past_int(uint64_t c0, uint64_t c1) { return c0 > 0x7FFFFFFFull || c1 > 0x7FFFFFFFull; }

}  // namespace rows
}  // namespace hast
