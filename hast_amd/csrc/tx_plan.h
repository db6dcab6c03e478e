// tx_plan.h -- what the device step of the stLFR -> 10x conversion decides per record, beside the rules of tx_core.h: the map as a
// table a kernel can read, the key of a header as that table's key, and the PLAN of a pair -- where its lines lie and what both of its
// output records are, byte by byte.  TX_HD integer code: the kernels (tx_kernels.hip) and the sequential model of
// tests/native/test_tx_plan.cpp step these very functions.
//
// THE TABLE.  Read-only, open addressing with linear probing over TableSlot (48 bytes), n_slots a power of two >= 2 * keys (load <=
// 0.5, so a probe sequence always ends at an empty slot).  key = the 16-byte text record of name_claim.h: byte 0 the key's length
// (1 .. 15), bytes 1 .. length the key, zeros behind, read as four little-endian words; hashed with name_hash, home slot = hash &
// (n_slots - 1).  A slot whose key[0] is 0 is empty (no key has length 0: a map with the empty key is not device_ok).  value[0 .. v)
// are the value's bytes, v = 0 .. 16.
//
// THE STEP over two buffers r1 / r2, nl1 / nl2 = the offsets of their newlines (32 bits: see tx_device.h for the arithmetic):
//   m = min(n_nl1 / 4, n_nl2 / 4) pairs; record i of a side is its lines 4i .. 4i+3; consumed = the byte behind record m-1.
//   pair i is kept when key_record() of its read-1 header gives a key and table_find() a slot.
//   N of a kept pair = used + 1 + (kept pairs in front of it); plan_pair() gives the extents and both record lengths,
//   rec1_byte() / rec2_byte() byte j of the two output records.  Whoever emits, emits through these two.
#pragma once
#include <stdint.h>

#include "name_claim.h"
#include "tx_core.h"

namespace hast {
namespace tx {

struct TableSlot {
    uint32_t key[4];           // the text record; key[0] == 0: empty
    uint8_t value[16];
    uint32_t v;                // bytes of value
    uint32_t pad[3];
};
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// slots for n_keys keys: the power of two that keeps the load at or under 0.5 (at least 2)
TX_HD uint64_t table_slots_for(uint64_t n_keys) {
    uint64_t n = 2;
    while (n < 2 * n_keys) n <<= 1;
    return n;
}

// the text record of key[0, len), len = 1 .. 15
TX_HD void pack_key(const uint8_t *key, uint32_t len, uint32_t out[4]) {
    uint64_t lo = len, hi = 0;                                   // (two words, not an indexed array: a kernel keeps them in registers)
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t at = i + 1;
        if (at < 8) lo |= (uint64_t)key[i] << (8 * at);
        else hi |= (uint64_t)key[i] << (8 * (at - 8));
    }
    out[0] = (uint32_t)lo; out[1] = (uint32_t)(lo >> 32);
    out[2] = (uint32_t)hi; out[3] = (uint32_t)(hi >> 32);
}

// the slot that holds `key`, or kNoSlot
TX_HD uint32_t table_find(const TableSlot *table, uint32_t n_slots, const uint32_t key[4]) {
    const uint32_t mask = n_slots - 1;
    uint32_t at = name_hash(key) & mask;
    for (uint32_t probes = 0; probes < n_slots; ++probes) {
        const TableSlot &s = table[at];
        if (s.key[0] == 0) return kNoSlot;
        if (s.key[0] == key[0] && s.key[1] == key[1] && s.key[2] == key[2] && s.key[3] == key[3]) return at;
        at = (at + 1) & mask;
    }
    return kNoSlot;
}

// The key of the header line buf[lo, hi) (hi: its '\n') as a text record.  false: the key is empty or longer than 15 bytes -- no
// device_ok map holds it, the pair is dropped.
TX_HD bool key_record(const uint8_t *buf, uint64_t lo, uint64_t hi, uint32_t out[4]) {
    uint64_t klo, khi;
    key_of(buf, lo, hi, &klo, &khi);
    const uint64_t len = khi - klo;
    if (len < 1 || len > kMaxKey) return false;
    pack_key(buf + klo, (uint32_t)len, out);
    return true;
}

// the pairs a step takes, and the byte behind the m-th record of a side (nl: its newline offsets)
TX_HD uint32_t pairs_of(uint32_t n_nl1, uint32_t n_nl2) { return (n_nl1 < n_nl2 ? n_nl1 : n_nl2) / 4; }
TX_HD uint64_t consumed_of(const uint32_t *nl, uint32_t m) { return m ? (uint64_t)nl[4 * (uint64_t)m - 1] + 1 : 0; }
// [*lo, *hi): the header of record i without its '\n'
TX_HD void header_of(const uint32_t *nl, uint32_t i, uint64_t *lo, uint64_t *hi) {
    *lo = i ? (uint64_t)nl[4 * (uint64_t)i - 1] + 1 : 0;
    *hi = nl[4 * (uint64_t)i];
}

struct Plan {
    uint32_t s1, q1, e1;       // read 1: where line 2 starts, where line 4 starts, the byte behind line 4's '\n'
    uint32_t s2, q2, e2;       // read 2, the same
    uint32_t w;                // digits of N
    uint32_t front1, front2;   // bytes in front of line 2 in the two output records
    uint32_t rec1_len, rec2_len;   // 0 for a dropped pair
};

// the plan of pair i: kept? its N, v = the bytes of its value
TX_HD Plan plan_pair(const uint32_t *nl1, const uint32_t *nl2, uint32_t i, bool kept, uint64_t n, uint32_t v) {
    const uint64_t at = 4 * (uint64_t)i;
    Plan p;
    p.s1 = nl1[at] + 1; p.q1 = nl1[at + 2] + 1; p.e1 = nl1[at + 3] + 1;
    p.s2 = nl2[at] + 1; p.q2 = nl2[at + 2] + 1; p.e2 = nl2[at + 3] + 1;
    p.w = dec_width(n);
    p.front1 = kNameHead + p.w + kNameTail + v + kSeqMid;
    p.front2 = kNameHead + p.w + kNameTail;
    p.rec1_len = kept ? rec1_len(n, v, p.e1 - p.s1) : 0;
    p.rec2_len = kept ? rec2_len(n, p.e2 - p.s2) : 0;
    return p;
}

// byte j of read 1's output record: name, value, ATCGAGN | lines 2 and 3 as they are | 22 F and a '#' | line 4 through qual()
TX_HD uint8_t rec1_byte(const Plan &p, const uint8_t *r1, uint64_t n, const uint8_t *value, uint32_t v, uint32_t j) {
    if (j < p.front1) return rec1_front(n, p.w, value, v, j);
    j -= p.front1;
    const uint32_t mid = p.q1 - p.s1;
    if (j < mid) return r1[p.s1 + j];
    j -= mid;
    if (j < kQualHead) return qual_head(j);
    return qual(r1[p.q1 + (j - kQualHead)]);
}
// byte j of read 2's: name | lines 2 and 3 as they are | line 4 through qual()
TX_HD uint8_t rec2_byte(const Plan &p, const uint8_t *r2, uint64_t n, uint32_t j) {
    if (j < p.front2) return rec2_front(n, p.w, j);
    j -= p.front2;
    const uint32_t mid = p.q2 - p.s2;
    if (j < mid) return r2[p.s2 + j];
    return qual(r2[p.q2 + (j - mid)]);
}

}  // namespace tx
}  // namespace hast
