// rr_core.h -- "read rows": the text of stage 03's per-read rows (`classify_read --rows device`), worked out from the votes alone.
// Plain integer code: the kernels (rr_kernels.hip), the direct host stepping of tests/native/test_rr_core.cpp and the sizing of the row
// buffers all step the same functions; rr_host.h (format_rows, with snprintf) is the checker and the route of every fallback.
//
//   row      name \t haplotype0|haplotype1 \t D \n      or      name \t ambiguous \t 0.0 \n        (s03:110-133, 215-216)
//            The class is rb::class_of over rb::density, the bins' rule, and D the density of the class that won.
//   D        what printf("%0.6f", d) prints for the double d = (double)v / (double)t, from the double's bits: d = m 2^-s with m the 53-bit
//            significand and s = 1075 - biased exponent, P = m 10^6 (below 2^73: two 64-bit words), q = P >> s, r = P mod 2^s,
//            h = 2^(s-1); q is rounded up when r > h, or when r == h and q is odd (glibc rounds the exact value to even: 1/128 prints
//            0.007812 and 3/128 prints 0.023438).  s >= 128: q = 0.  The text is q / 10^6, '.', q % 10^6 on six digits.
//   precondition   both set sizes are at least 1, so d is finite, at most 2^32 - 1 (s >= 21) and never subnormal: no "inf", no "nan".
//            The density printed is always above 0: haplotype0 wins only with d0 >= d1 and one of them above 0.
//   row_bytes   the length of that text: the only sizing rule.  The part behind the name is at most kMaxTail bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#include "rb_core.h"

namespace hast {
namespace rr {

constexpr uint32_t kMaxTail = 31;                // "\thaplotypeN\t" (12) + 10 digits + '.' + 6 digits + '\n' = 30
constexpr uint64_t kMillion = 1000000;

// a * b as two 64-bit words
RS_HD void mul_64x64(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    *hi = __umul64hi(a, b);
    *lo = a * b;
#else
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    *lo = (mid << 32) | (uint32_t)p00;
    *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
#endif
}

// q of the rule above: d 10^6 rounded to the nearest integer, ties to even, for a finite d in [0, 2^53)
RS_HD uint64_t fixed6(double d) {
    uint64_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = (uint64_t)__double_as_longlong(d);
#else
    memcpy(&bits, &d, 8);
#endif
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7ffu;
    if (e == 0 || e > 1074) return 0;            // zero (subnormals, and what the precondition rules out, do not occur)
    const uint64_t m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    const uint32_t s = 1075 - e;                 // 1 .. 1074
    if (s >= 128) return 0;
    uint64_t hi, lo;
    mul_64x64(m, kMillion, &hi, &lo);
    uint64_t q, r_hi, r_lo, h_hi, h_lo;
    if (s < 64) {
        q = (lo >> s) | (hi << (64 - s));
        r_hi = 0;
        r_lo = lo & ((1ull << s) - 1);
        h_hi = 0;
        h_lo = 1ull << (s - 1);
    } else {
        q = hi >> (s - 64);
        r_hi = s == 64 ? 0 : hi & ((1ull << (s - 64)) - 1);
        r_lo = lo;
        h_hi = s == 64 ? 0 : 1ull << (s - 65);
        h_lo = s == 64 ? 1ull << 63 : 0;
    }
    const bool above = r_hi > h_hi || (r_hi == h_hi && r_lo > h_lo), tie = r_hi == h_hi && r_lo == h_lo;
    return q + ((above || (tie && (q & 1))) ? 1 : 0);
}

RS_HD uint32_t dec_digits(uint64_t x) {
    uint32_t n = 1;
    while (x >= 10) {
        x /= 10;
        ++n;
    }
    return n;
}

// the class of a read and the q of the density its row prints (0 for ambiguous)
RS_HD void row_of(uint32_t v0, uint32_t v1, uint32_t t0, uint32_t t1, uint32_t *cls, uint64_t *q) {
    const double d0 = rb::density(v0, (double)t0), d1 = rb::density(v1, (double)t1);
    *cls = rb::class_of(d0, d1);
    *q = *cls == rb::kAmbiguous ? 0 : fixed6(*cls == rb::kHap1 ? d1 : d0);
}

// bytes of the row behind the name
RS_HD uint32_t tail_bytes(uint32_t cls, uint64_t q) { return cls == rb::kAmbiguous ? 15 : 12 + dec_digits(q / kMillion) + 8; }
RS_HD uint64_t row_bytes(uint32_t name_len, uint32_t cls, uint64_t q) { return (uint64_t)name_len + tail_bytes(cls, q); }

// The part of the row behind the name, stored byte by byte at p (tail_bytes(cls, q) of them; no array of its own: a kernel keeps
// it in registers).  Returns the bytes written.
RS_HD uint32_t put_tail(uint8_t *p, uint32_t cls, uint64_t q) {
    if (cls == rb::kAmbiguous) {
        const char *const text = "\tambiguous\t0.0\n";
        for (uint32_t i = 0; i < 15; ++i) p[i] = (uint8_t)text[i];
        return 15;
    }
    const char *const label = "\thaplotype";
    for (uint32_t i = 0; i < 10; ++i) p[i] = (uint8_t)label[i];
    p[10] = (uint8_t)('0' + cls);
    p[11] = '\t';
    uint64_t ip = q / kMillion;
    uint32_t fp = (uint32_t)(q % kMillion);
    const uint32_t nd = dec_digits(ip);
    for (uint32_t i = nd; i-- > 0;) {
        p[12 + i] = (uint8_t)('0' + ip % 10);
        ip /= 10;
    }
    p[12 + nd] = '.';
    for (uint32_t i = 6; i-- > 0;) {
        p[13 + nd + i] = (uint8_t)('0' + fp % 10);
        fp /= 10;
    }
    p[19 + nd] = '\n';
    return 20 + nd;
}

}  // namespace rr
}  // namespace hast
