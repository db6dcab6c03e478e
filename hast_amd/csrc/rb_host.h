// rb_host.h -- the host model of the read bins: the three runs of a view by the functions of rb_core.h, the way the kernels k_rb_* of
// rs_kernels.hip step them (a lane per record: class and extent; the records of a class back to back, in input order).  It is what
// `classify_read --ingest host --bin-reads` and every fallback of the device route write, and what tests/native/test_rb_core.cpp
// reads files through, view by view.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rb_core.h"
#include "rs_host.h"

namespace hast {
namespace rb {

struct Extent {
    uint64_t lo, hi;
};
struct Runs {
    std::string run[kClasses];
    uint64_t count[kClasses] = {0, 0, 0};
    void clear() {
        for (uint32_t c = 0; c < kClasses; ++c) run[c].clear(), count[c] = 0;
    }
};

// the extents of the records that rs::frame finds in the view buf[0, n), in its order
inline void extents(int format, const uint8_t *buf, size_t n, bool last, std::vector<Extent> *out) {
    out->clear();
    std::vector<uint32_t> nl, hdr;
    for (size_t i = 0; i < n; ++i)
        if (buf[i] == '\n') nl.push_back((uint32_t)i);
    const uint32_t n_nl = (uint32_t)nl.size();
    uint32_t lo, hi;
    if (format == RS_FASTQ) {
        for (uint32_t i = 0; i < rs::fq_records(n_nl); ++i) {
            fq_extent(nl.data(), i, &lo, &hi);
            out->push_back({lo, hi});
        }
        return;
    }
    for (uint32_t j = 0; j < n_nl; ++j)
        if (rs::fa_class(buf, rs::line_lo(nl.data(), j), nl[j]) == rs::kHeader) hdr.push_back(j);
    const uint32_t m = (uint32_t)hdr.size();
    for (uint32_t r = 0; r < rs::fa_records(m, last); ++r) {
        fa_extent(nl.data(), n_nl, hdr.data(), m, r, &lo, &hi);
        out->push_back({lo, hi});
    }
}

// n records of the view buf: ext[i] their extents, votes[2 i], votes[2 i + 1] their hits; appended to the runs of their classes
inline void append_runs(const uint8_t *buf, const Extent *ext, const uint32_t *votes, size_t n, uint32_t total0, uint32_t total1, Runs *out) {
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = read_class(votes[2 * i], votes[2 * i + 1], total0, total1);
        out->run[c].append(reinterpret_cast<const char *>(buf) + ext[i].lo, ext[i].hi - ext[i].lo);
        ++out->count[c];
    }
}

// What a FASTQ file's end leaves behind its last complete record (rs::fq_tail): if it is a record, its bytes as they lie, plus one '\n'
// if they do not end in one, to the run of the class of its votes.  False: the format error.
inline bool append_tail(const uint8_t *tail, size_t n, const uint32_t *votes, uint32_t total0, uint32_t total1, Runs *out) {
    rs::Tail t;
    if (!rs::fq_tail(tail, n, &t)) return false;
    if (!t.record) return true;
    const uint32_t c = read_class(votes[0], votes[1], total0, total1);
    out->run[c].append(reinterpret_cast<const char *>(tail), n);
    if (tail[n - 1] != '\n') out->run[c] += '\n';
    ++out->count[c];
    return true;
}

}  // namespace rb
}  // namespace hast
