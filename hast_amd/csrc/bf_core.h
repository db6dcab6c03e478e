// bf_core.h -- the rule of stage 02's per-barcode read count (the line of assemble_by_supernova.sh that writes barcode_freq.txt:
// an awk one-liner with the separators '#' and '/' over the read-1 file), once.  Plain integer code that the device kernel
// (k_fq_field2, fq_kernels.hip), the host model (bf_host.h) and tests/native/test_bf_core.cpp step alike.
//
// Lines are numbered from 1 over the inflated stream; a line ends at '\n', an unterminated last line is a line.  Only lines
// 1, 5, 9, ... count (nothing is validated: no '@', no '+'; an empty line in such a place is a header line without fields).  The
// header line is split at every '#' and every '/'.  A line without a separator has at most one field and is not counted
// ("no field").  Otherwise the KEY is the second field: the bytes between the first separator and the next one, or the end of the
// line.  It may be empty; tabs, spaces, '\r' and NUL are ordinary bytes; there is no length limit; "0_0_0" is a key like any other.
// (The field rule of the routing kernel k_route_class -- neither classify's parseName nor fake_10x's key.)
#pragma once
#include <stdint.h>

#ifndef HAST_HD                 // (as name_claim.h and hast_common.h define it: whichever comes first)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HAST_HD __host__ __device__ __forceinline__
#else
#define HAST_HD inline
#endif
#endif

namespace hast {
namespace bf {

constexpr uint32_t kMaxText = 15;                 // bytes of a key a 16-byte text record holds (length byte + text)
constexpr uint32_t kLongMark = 0xFFu;             // length byte of a record whose key is longer: the naming kernel passes it by
constexpr uint32_t kNoFieldLen = 0xFFFFFFFFu;     // field length written for a header line without a field 2
constexpr uint32_t kNotOwnedLen = 0xFFFFFFFEu;    // ... and for a candidate that is not a header line of this block

HAST_HD bool is_sep(uint8_t c) { return c == '#' || c == '/'; }

// field 2 of the header line [line, line + n) (without its '\n'): false when the line has no separator; else [start, start + len)
HAST_HD bool field2(const uint8_t *line, uint64_t n, uint64_t &start, uint64_t &len) {
    uint64_t a = 0;
    while (a < n && !is_sep(line[a])) ++a;
    if (a == n) return false;
    uint64_t b = a + 1;
    while (b < n && !is_sep(line[b])) ++b;
    start = a + 1;
    len = b - a - 1;
    return true;
}

// the 16-byte text record of a key of at most kMaxText bytes: byte 0 its length, bytes 1.. the text, the rest zero -- as four
// little-endian words, the key format of the device dictionary (name_claim.h)
HAST_HD void text_record(const uint8_t *key, uint32_t len, uint32_t w[4]) {
    w[0] = len; w[1] = 0; w[2] = 0; w[3] = 0;
    for (uint32_t j = 0; j < len; ++j) w[(j + 1) >> 2] |= (uint32_t)key[j] << (8 * ((j + 1) & 3));
}
// records the dictionary does not number: a key of more than kMaxText bytes (the host counts it), a line without field 2 and a
// candidate that is no header line of the block (nobody counts those)
HAST_HD void long_record(uint32_t w[4]) { w[0] = kLongMark; w[1] = 0; w[2] = 0; w[3] = 0; }
HAST_HD void nofield_record(uint32_t w[4]) { w[0] = kLongMark; w[1] = 1; w[2] = 0; w[3] = 0; }

}  // namespace bf
}  // namespace hast
