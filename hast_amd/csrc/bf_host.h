// bf_host.h -- the host model of stage 02's per-barcode read count (bf_core.h has the rule): a stream, whole or in pieces of any
// size with the line phase carried from piece to piece, to a map key -> count.  It is the checker of the tests, the route of
// `barcode_freq --count host`, and what the device route hands everything to that the device leaves behind: keys longer than a text
// record, keys that arrive once a tally's dictionary has given out its last id, the partial record at a file's end.
// Host only: bf_core.h and the standard library.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "bf_core.h"

namespace hast {
namespace bf {

struct Model {
    std::unordered_map<std::string, uint64_t> counts;
    uint64_t header_lines = 0, counted = 0, no_field = 0;

    void add_key(const uint8_t *key, size_t len, uint64_t n = 1) {
        counts[std::string(reinterpret_cast<const char *>(key), len)] += n;
    }
    // a header line without its '\n'
    void add_header(const uint8_t *line, size_t n) {
        ++header_lines;
        uint64_t start = 0, len = 0;
        if (!field2(line, n, start, len)) { ++no_field; return; }
        ++counted;
        add_key(line + start, (size_t)len);
    }

    // ---- a stream in pieces: begin() at its first byte, feed() any number of times, finish() at its end
    void begin() {
        phase_ = 0;
        open_ = false;
        partial_.clear();
    }
    void feed(const uint8_t *p, size_t n) {
        for (size_t at = 0; at < n;) {
            const uint8_t *nl = static_cast<const uint8_t *>(memchr(p + at, '\n', n - at));
            const size_t end = nl ? (size_t)(nl - p) : n;
            if (phase_ == 0) {
                if (!nl || open_) {                               // a header line that lies in more than one piece
                    partial_.append(reinterpret_cast<const char *>(p + at), end - at);
                    open_ = true;
                }
                if (nl) {
                    if (open_) add_header(reinterpret_cast<const uint8_t *>(partial_.data()), partial_.size());
                    else add_header(p + at, end - at);
                    partial_.clear();
                    open_ = false;
                }
            }
            if (!nl) break;
            phase_ = (phase_ + 1) & 3;
            at = end + 1;
        }
    }
    // the end of the stream: an unterminated last line is a line
    void finish() {
        if (phase_ == 0 && open_) add_header(reinterpret_cast<const uint8_t *>(partial_.data()), partial_.size());
        begin();
    }
    void whole(const uint8_t *p, size_t n) {
        begin();
        feed(p, n);
        finish();
    }

  private:
    uint32_t phase_ = 0;           // lines completed so far, mod 4: 0 = inside (or in front of) a header line
    bool open_ = false;            // bytes of the current header line are waiting in partial_
    std::string partial_;
};

typedef std::vector<std::pair<std::string, uint64_t>> Rows;

// rows from any number of sources -> one row per key, byte-wise ascending, counts of equal keys summed
inline void merge_rows(Rows &rows) {
    std::sort(rows.begin(), rows.end(), [](const std::pair<std::string, uint64_t> &a, const std::pair<std::string, uint64_t> &b) {
        const size_t m = std::min(a.first.size(), b.first.size());
        const int c = m ? memcmp(a.first.data(), b.first.data(), m) : 0;
        return c ? c < 0 : a.first.size() < b.first.size();
    });
    size_t out = 0;
    for (size_t i = 0; i < rows.size(); ++i) {
        if (out && rows[out - 1].first == rows[i].first) rows[out - 1].second += rows[i].second;
        else {
            if (out != i) rows[out] = std::move(rows[i]);
            ++out;
        }
    }
    rows.resize(out);
}

// key \t count \n per row, the count in plain decimal
inline void print_rows(const Rows &rows, std::string &out) {
    char num[24];
    for (const std::pair<std::string, uint64_t> &r : rows) {
        out.append(r.first);
        out.push_back('\t');
        int n = 0;
        uint64_t v = r.second;
        do { num[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (n) out.push_back(num[--n]);
        out.push_back('\n');
    }
}

}  // namespace bf
}  // namespace hast
