// rows_host.h -- the host model of the output table of `classify --rows device`: what the kernels of rows_kernels.hip leave, by the
// functions of rows_core.h and in the kernels' own steps (a key, a call and the lengths per id; the ids ordered by key; the rows and
// the list lines written in that order).  tests/native/test_rows_core.cpp holds it to an independent model in Python.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "rows_core.h"

namespace hast {
namespace rows {

struct Tables {
    std::string table, list[3];
    std::vector<uint8_t> cls;                      // by id: row_list of its call
    std::vector<uint32_t> order;                   // ids in row order
    bool any_sep = false, past_int = false;
};

// text16[n][16], counts[n][4] = {c0, c1, neg, reserved} as the context's counters lie
inline void build(const uint8_t *text16, const uint64_t *counts, size_t n, uint64_t n0, uint64_t n1, double w0, double w1, Tables *out) {
    *out = Tables();
    std::vector<Key> key(n);
    std::vector<int8_t> hap(n);
    out->cls.resize(n);
    out->order.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *rec = text16 + 16 * i;
        const uint64_t c0 = counts[4 * i], c1 = counts[4 * i + 1];
        key[i] = row_key(rec);
        hap[i] = (int8_t)row_hap(rec, c0, c1, n0, n1, w0, w1);
        out->cls[i] = (uint8_t)row_list(hap[i]);
        out->order[i] = (uint32_t)i;
        out->any_sep = out->any_sep || has_sep(rec);
        out->past_int = out->past_int || past_int(c0, c1);
    }
    std::stable_sort(out->order.begin(), out->order.end(), [&](uint32_t a, uint32_t b) { return key[a].lo < key[b].lo; });
    std::stable_sort(out->order.begin(), out->order.end(), [&](uint32_t a, uint32_t b) { return key[a].hi < key[b].hi; });
    uint8_t buf[kMaxRow];
    for (size_t r = 0; r < n; ++r) {
        const uint32_t i = out->order[r];
        const uint8_t *rec = text16 + 16 * (size_t)i;
        const uint64_t c0 = counts[4 * (size_t)i], c1 = counts[4 * (size_t)i + 1];
        const uint32_t m = put_row(buf, rec, hap[i], c0, c1);
        if (m != row_len(rec, hap[i], c0, c1)) out->table += "<row_len != put_row>";     // (never: the test compares the texts)
        out->table.append(reinterpret_cast<const char *>(buf), m);
        out->list[out->cls[i] - 1].append(reinterpret_cast<const char *>(buf), put_line(buf, rec));
    }
}

}  // namespace rows
}  // namespace hast
