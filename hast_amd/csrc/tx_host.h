// tx_host.h -- the host model of the stLFR -> 10x conversion (fake_10x.pl): the map file, and the conversion of two buffers of raw
// FASTQ over the rules of tx_core.h, the script's behaviour at the end of its inputs included.  Plain C++, no GPU: behind
// hast_tx_map_* / hast_tx_pair_host (tx_api.cpp), and stepped by tests/native/test_tx_core.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "tx_core.h"
#include "tx_plan.h"

namespace hast {
namespace tx {

// The map file as perl reads it: every line chomped and split at tabs, map[field 0] = field 1, a later line wins, a line without a
// tab maps its key to the empty string.  (An empty line is the empty key.)
struct Map {
    std::unordered_map<std::string, std::string> kv;
    bool device_ok = true;
    std::string reason = "none";           // why the device path cannot take this map
};

inline void map_parse(const uint8_t *text, size_t n, Map &m) {
    m.kv.clear();
    for (size_t at = 0; at < n;) {
        const uint8_t *nl = static_cast<const uint8_t *>(memchr(text + at, '\n', n - at));
        const size_t end = nl ? (size_t)(nl - text) : n;
        const uint8_t *t1 = static_cast<const uint8_t *>(memchr(text + at, '\t', end - at));
        const size_t k_end = t1 ? (size_t)(t1 - text) : end;
        std::string value;
        if (t1) {
            const uint8_t *t2 = static_cast<const uint8_t *>(memchr(t1 + 1, '\t', end - (k_end + 1)));
            value.assign(reinterpret_cast<const char *>(t1 + 1), (t2 ? (size_t)(t2 - text) : end) - (k_end + 1));
        }
        m.kv[std::string(reinterpret_cast<const char *>(text + at), k_end - at)] = value;
        at = end + 1;
    }
    bool empty_key = false, long_key = false, long_value = false;
    for (const auto &e : m.kv) {
        empty_key |= e.first.empty();
        long_key |= e.first.size() > kMaxKey;
        long_value |= e.second.size() > kMaxValue;
    }
    m.device_ok = !(empty_key || long_key || long_value);
    m.reason = empty_key ? "empty key" : long_key ? "key longer than 15 bytes" : long_value ? "value longer than 16 bytes" : "none";
}

// the map as the table of tx_plan.h (device_ok maps only: keys of 1 .. 15 bytes, values of 0 .. 16); what a device step uploads
inline void table_build(const Map &m, std::vector<TableSlot> &table) {
    table.assign((size_t)table_slots_for(m.kv.size()), TableSlot{});
    const uint32_t mask = (uint32_t)table.size() - 1;
    for (const auto &e : m.kv) {
        uint32_t k[4];
        pack_key(reinterpret_cast<const uint8_t *>(e.first.data()), (uint32_t)e.first.size(), k);
        uint32_t at = name_hash(k) & mask;
        while (table[at].key[0]) at = (at + 1) & mask;
        TableSlot &s = table[at];
        memcpy(s.key, k, sizeof k);
        memcpy(s.value, e.second.data(), e.second.size());
        s.v = (uint32_t)e.second.size();
    }
}

struct State {
    uint64_t used = 0, headers = 0;        // N so far, read-1 headers so far
};

// the script's progress lines for the headers (before, after]
inline void progress_lines(uint64_t before, uint64_t after, std::string &out) {
    for (uint64_t mb = before / 1000000 + 1; mb * 1000000 <= after; ++mb) out += "process " + std::to_string(mb) + " (Mb) pair of reads now  \n";
}

struct Lines {                             // perl's <FH>: the next line with its '\n', the unterminated rest, or nothing
    const uint8_t *p;
    size_t n, at = 0;
    bool next(size_t *lo, size_t *hi) {
        if (at >= n) return false;
        const uint8_t *nl = static_cast<const uint8_t *>(memchr(p + at, '\n', n - at));
        *lo = at;
        at = *hi = nl ? (size_t)(nl - p) + 1 : n;
        return true;
    }
};

// the byte behind the whole records (four newlines each) of buf, at most `most` of them; *n_rec = how many
inline size_t whole_records(const uint8_t *buf, size_t n, uint64_t most, uint64_t *n_rec) {
    size_t at = 0, end = 0;
    uint64_t rec = 0;
    for (uint32_t lines = 0; rec < most && at < n;) {
        const uint8_t *nl = static_cast<const uint8_t *>(memchr(buf + at, '\n', n - at));
        if (!nl) break;
        at = (size_t)(nl - buf) + 1;
        if (++lines == 4) { lines = 0; ++rec; end = at; }
    }
    *n_rec = rec;
    return end;
}

// One step.  mode kNotFinal: the m = min(whole records of r1, of r2) first pairs, *c1 / *c2 = the byte behind them; the caller
// carries the rest in front of the next bytes.  kFinal: the inputs end here -- everything, the way the script ends: missing lines
// are empty strings, an unterminated line gets no newline, a partial read-1 record whose key the map holds is numbered.
// kRead2Ended: r2 is all that is left of read 2 while read 1 goes on -- the whole records of r1, paired with what r2 still has and
// then with nothing, as the script does; *c2 = what they took of r2.
enum { kNotFinal = 0, kFinal = 1, kRead2Ended = 2 };
// the mode of the next step over what has been read and not converted yet; eof1 / eof2 = that input has been read to its end
inline int step_mode(bool eof1, bool eof2, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2) {
    uint64_t rec1, rec2;
    whole_records(r1, n1, 1, &rec1);
    whole_records(r2, n2, 1, &rec2);
    if (eof1 && !rec1 && (eof2 || rec2)) return kFinal;          // read 1 ends here: the script takes one more record of read 2 at the most
    if (eof2 && !rec2) return kRead2Ended;
    return kNotFinal;
}
inline void pair_host(const Map &map, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2, int mode, State &st, std::string &out1, std::string &out2,
                      size_t *c1, size_t *c2) {
    size_t lim1 = n1, lim2 = n2;
    if (mode != kFinal) {
        uint64_t m1, m2 = ~0ull;
        whole_records(r1, n1, ~0ull, &m1);
        if (mode == kNotFinal) whole_records(r2, n2, ~0ull, &m2);
        const uint64_t m = m1 < m2 ? m1 : m2;
        lim1 = whole_records(r1, n1, m, &m1);
        if (mode == kNotFinal) lim2 = whole_records(r2, n2, m, &m2);
    }
    *c1 = lim1;
    Lines a{r1, lim1}, b{r2, lim2};
    size_t lo, hi;
    std::string key;
    while (a.next(&lo, &hi)) {
        ++st.headers;
        uint64_t klo, khi;
        key_of(r1, lo, hi > lo && r1[hi - 1] == '\n' ? hi - 1 : hi, &klo, &khi);
        key.assign(reinterpret_cast<const char *>(r1 + klo), khi - klo);
        const auto it = map.kv.find(key);
        if (it == map.kv.end()) {
            for (int i = 0; i < 3; ++i) a.next(&lo, &hi);
            for (int i = 0; i < 4; ++i) b.next(&lo, &hi);
            continue;
        }
        const uint64_t n = ++st.used;
        const uint32_t w = dec_width(n), v = (uint32_t)it->second.size();
        const uint8_t *value = reinterpret_cast<const uint8_t *>(it->second.data());
        for (uint32_t j = 0; j < kNameHead + w + kNameTail + v + kSeqMid; ++j) out1 += (char)rec1_front(n, w, value, v, j);
        for (int line = 2; line <= 4; ++line) {
            const bool have = a.next(&lo, &hi);
            if (line == 4)
                for (uint32_t j = 0; j < kQualHead; ++j) out1 += (char)qual_head(j);
            if (!have) continue;
            if (line < 4) out1.append(reinterpret_cast<const char *>(r1 + lo), hi - lo);
            else
                for (size_t j = lo; j < hi; ++j) out1 += (char)qual(r1[j]);
        }
        b.next(&lo, &hi);
        for (uint32_t j = 0; j < kNameHead + w + kNameTail; ++j) out2 += (char)rec2_front(n, w, j);
        for (int line = 2; line <= 4; ++line) {
            if (!b.next(&lo, &hi)) continue;
            if (line < 4) out2.append(reinterpret_cast<const char *>(r2 + lo), hi - lo);
            else
                for (size_t j = lo; j < hi; ++j) out2 += (char)qual(r2[j]);
        }
    }
    *c2 = mode == kFinal ? n2 : b.at;
}

}  // namespace tx
}  // namespace hast
