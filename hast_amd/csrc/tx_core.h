// tx_core.h -- the rules by which a pair of stLFR FASTQ records becomes a pair of 10x records (stage 02's fake_10x.pl).  Plain
// integer code, written so that device kernels can step the same functions as the host model (tx_host.h,
// tests/native/test_tx_core.cpp) does.
//
// Record i of read 1 (its lines 4i .. 4i+3) goes with record i of read 2, whatever the headers say; nothing is validated.
// The KEY of a read-1 record: its header line without the '\n' (a '\r' stays), cut at its first tab; the text after the FIRST '#'
// up to the next '#' or '/' or the end.  No '#' in front of the tab: the empty key.  (Neither classify's parseName nor awk's
// -F '#|/' field 2.)  A key the map does not hold drops both records.  A key it holds makes the pair number N (kept pairs, from
// 1, 64 bits) and
//   read 1:  @ST-E0:0:SIMULATE:8:0:0:<N> 1:N:0:NAAGTGCT\n            read 2:  @ST-E0:0:SIMULATE:8:0:0:<N> 2:N:0:NAAGTGCT\n
//            <value>ATCGAGN<line 2>                                            <line 2>
//            <line 3>                                                          <line 3>
//            FFFFFFFFFFFFFFFFFFFFFF#<line 4, every '!' a '#'>                  <line 4, every '!' a '#'>
// with the lines as they are, their '\n' included.  22 'F' and one '#', whatever the value's length.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TX_HD __host__ __device__ __forceinline__
#else
#define TX_HD inline
#endif

namespace hast {
namespace tx {

constexpr uint32_t kMaxKey = 15, kMaxValue = 16;          // what a device path can take (16-byte text records): keys of 1 .. 15 bytes, values of 0 .. 16
constexpr uint32_t kNameHead = 24, kNameTail = 16, kSeqMid = 7, kQualHead = 23;

TX_HD uint8_t name_head(uint32_t i) { return (uint8_t)"@ST-E0:0:SIMULATE:8:0:0:"[i]; }
TX_HD uint8_t name_tail(uint32_t i, int side) { return i == 1 ? (uint8_t)('1' + side) : (uint8_t)" 1:N:0:NAAGTGCT\n"[i]; }
TX_HD uint8_t seq_mid(uint32_t i) { return (uint8_t)"ATCGAGN"[i]; }
TX_HD uint8_t qual_head(uint32_t i) { return i < 22 ? (uint8_t)'F' : (uint8_t)'#'; }
TX_HD uint8_t qual(uint8_t c) { return c == '!' ? (uint8_t)'#' : c; }

TX_HD uint32_t dec_width(uint64_t n) {
    uint32_t w = 1;
    while (n >= 10) { n /= 10; ++w; }
    return w;
}
// digit p (0: the first one) of n, written with w digits
TX_HD uint8_t dec_digit(uint64_t n, uint32_t w, uint32_t p) {
    for (uint32_t i = p + 1; i < w; ++i) n /= 10;
    return (uint8_t)('0' + n % 10);
}

// the key of the header line buf[lo, hi) (hi: its '\n', or where the input ends)
TX_HD void key_of(const uint8_t *buf, uint64_t lo, uint64_t hi, uint64_t *klo, uint64_t *khi) {
    uint64_t p = lo;
    while (p < hi && buf[p] != '\t' && buf[p] != '#') ++p;
    if (p >= hi || buf[p] == '\t') { *klo = *khi = lo; return; }
    const uint64_t a = ++p;
    while (p < hi && buf[p] != '\t' && buf[p] != '#' && buf[p] != '/') ++p;
    *klo = a;
    *khi = p;
}

// bytes of the name line of pair n, and of both records of a kept pair: v = the value's length, l234 = the bytes of lines 2 .. 4
// with their newlines
TX_HD uint32_t name_len(uint64_t n) { return kNameHead + dec_width(n) + kNameTail; }
TX_HD uint32_t rec1_len(uint64_t n, uint32_t v, uint32_t l234) { return name_len(n) + v + kSeqMid + kQualHead + l234; }
TX_HD uint32_t rec2_len(uint64_t n, uint32_t l234) { return name_len(n) + l234; }

// byte j of what stands in front of read 1's line 2: the name line, the value, ATCGAGN
TX_HD uint8_t rec1_front(uint64_t n, uint32_t w, const uint8_t *value, uint32_t v, uint32_t j) {
    if (j < kNameHead) return name_head(j);
    j -= kNameHead;
    if (j < w) return dec_digit(n, w, j);
    j -= w;
    if (j < kNameTail) return name_tail(j, 0);
    j -= kNameTail;
    if (j < v) return value[j];
    return seq_mid(j - v);
}
TX_HD uint8_t rec2_front(uint64_t n, uint32_t w, uint32_t j) {
    if (j < kNameHead) return name_head(j);
    j -= kNameHead;
    if (j < w) return dec_digit(n, w, j);
    return name_tail(j - w, 1);
}

}  // namespace tx
}  // namespace hast
