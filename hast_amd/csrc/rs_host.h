// rs_host.h -- the host model of the read-stream framer: one view framed into records by the functions of rs_core.h, the way the
// kernels of rs_kernels.hip step them (a newline index, the lines' classes, a prefix sum of the sequence bytes, a pass per record).
// tests/native/test_rs_core.cpp reads files through it block by block, as the feed of rs_api.cpp does.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rs_core.h"

namespace hast {
namespace rs {

struct Record {
    uint32_t name_pos, name_len;       // in the view
    std::string seq;
};
struct Framed {
    uint64_t consumed = 0, bases = 0;
    uint32_t flags = 0;
    uint32_t headers = 0;              // FASTA: header lines in the view (the caller's seen_header)
    std::vector<Record> recs;          // none when flags has RS_FORMAT_ERROR
};

inline void frame(int format, const uint8_t *buf, size_t n, bool last, bool seen_header, Framed *out) {
    *out = Framed();
    std::vector<uint32_t> nl;
    for (size_t i = 0; i < n; ++i)
        if (buf[i] == '\n') nl.push_back((uint32_t)i);
    const uint32_t n_nl = (uint32_t)nl.size();
    if (format == RS_FASTQ) {
        const uint32_t n_rec = fq_records(n_nl);
        out->consumed = fq_consumed(nl.data(), n_nl);
        for (uint32_t r = 0; r < n_rec; ++r) {
            const uint32_t lo = line_lo(nl.data(), 4 * r), hi = nl[4 * r];
            if (fq_bad_header(buf, lo, hi)) out->flags |= RS_FORMAT_ERROR;
            Record rec;
            name_of(lo, hi, &rec.name_pos, &rec.name_len);
            rec.seq.assign(reinterpret_cast<const char *>(buf) + hi + 1, nl[4 * r + 1] - (hi + 1));
            out->bases += rec.seq.size();
            out->recs.push_back(rec);
        }
    } else {
        // line_dst[j]: sequence bytes of the lines in front of line j; hdr[r]: the line of header r
        std::vector<uint32_t> line_dst(n_nl + 1, 0), hdr;
        for (uint32_t j = 0; j < n_nl; ++j) {
            const uint32_t lo = line_lo(nl.data(), j), hi = nl[j], cls = fa_class(buf, lo, hi);
            if (cls == kBad) out->flags |= RS_FORMAT_ERROR;
            if (cls == kHeader) hdr.push_back(j);
            line_dst[j + 1] = line_dst[j] + fa_seq_len(cls, lo, hi);
        }
        const uint32_t m = (uint32_t)hdr.size(), n_rec = fa_records(m, last);
        out->headers = m;
        out->consumed = fa_consumed(nl.data(), n_nl, n, m, m ? hdr[m - 1] : 0, last, seen_header);
        for (uint32_t r = 0; r < n_rec; ++r) {
            const uint32_t first = hdr[r] + 1, end = r + 1 < m ? hdr[r + 1] : n_nl;
            Record rec;
            name_of(line_lo(nl.data(), hdr[r]), nl[hdr[r]], &rec.name_pos, &rec.name_len);
            for (uint32_t j = first; j < end; ++j) {
                const uint32_t lo = line_lo(nl.data(), j);
                rec.seq.append(reinterpret_cast<const char *>(buf) + lo, line_dst[j + 1] - line_dst[j]);
            }
            out->bases += rec.seq.size();
            out->recs.push_back(rec);
        }
    }
    if (out->flags & RS_FORMAT_ERROR) {
        out->recs.clear();
        out->bases = 0;
    }
}

// What a FASTQ file's end leaves behind its last complete record (fewer than four newlines), read as the reference's loop reads
// it: a record iff the header line is terminated; its sequence is the next piece, terminated or not.  False: the format error.
struct Tail {
    bool record = false;
    std::string name, seq;
};
inline bool fq_tail(const uint8_t *buf, size_t n, Tail *out) {
    *out = Tail();
    const std::string tail = n ? std::string(reinterpret_cast<const char *>(buf), n) : std::string();
    const size_t he = tail.find('\n');
    if (he == std::string::npos) return true;
    const std::string head = tail.substr(0, he);
    if (!head.empty() && head[0] == '>') return false;
    const size_t s0 = he + 1, se = tail.find('\n', s0);
    out->record = true;
    out->name = head.empty() ? head : head.substr(1);
    out->seq = tail.substr(s0, se == std::string::npos ? std::string::npos : se - s0);
    return true;
}

}  // namespace rs
}  // namespace hast
