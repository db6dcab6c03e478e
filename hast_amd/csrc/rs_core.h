// rs_core.h -- "read stream": the rules by which a view of raw FASTA or four-line FASTQ becomes the reads of stage 03's per-read
// classifier (`classify_read --ingest device`).  Plain integer code: the framing kernels (rs_kernels.hip) and the host model
// (rs_host.h, tests/native/test_rs_core.cpp) step the same functions.
//
// The rules are the reference reader's (two getline loops) as classify_read_main.cpp's host route restates them for blocks.  A view
// is bytes[0, n): what the view before left unframed, then new bytes.  Lines are the newline-terminated ones; nl[j] is the offset
// of the view's j-th newline, line j is [line_lo(nl, j), nl[j]).
//   FASTQ  record i = lines 4i .. 4i+3.  Name: the header line minus its first byte (an empty header: an empty name).  Sequence: line
//          4i+1 as it lies, '\r' included.  Lines 4i+2, 4i+3 are not looked at.  A non-empty header that starts with '>' is the format
//          error.  consumed = the byte behind the last 4n-th newline; what a file's end leaves (fewer than four newlines) is the
//          caller's tail.
//   FASTA  an empty line is skipped; a line that starts with '>' is a header, with '@' or '+' the format error; any other line is a
//          sequence line, appended as it lies to the record of the last header in front of it (to none before the file's first
//          header).  With headers h0 .. h(m-1) in the view, records h0 .. h(m-2) are complete; not last: consumed = the line start of
//          h(m-1), or, with m = 0, the byte behind the last newline before the file's first header and 0 after it (the whole view is
//          one record's middle); last: h(m-1) ends with the last terminated line and everything is consumed -- the unterminated last
//          line is dropped.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

// the formats and the flags of hast_rs_block (include/hast.h has the same values under HAST_RS_*)
#define RS_FASTA 0
#define RS_FASTQ 1
#define RS_FORMAT_ERROR 1u
#define RS_RECORD_TOO_LONG 4u

namespace hast {
namespace rs {

enum : uint32_t { kEmpty = 0, kHeader = 1, kSeq = 2, kBad = 3 };      // what a FASTA line is

RS_HD uint32_t line_lo(const uint32_t *nl, uint32_t j) { return j ? nl[j - 1] + 1 : 0; }

// FASTA: the class of the line [lo, hi)
RS_HD uint32_t fa_class(const uint8_t *buf, uint32_t lo, uint32_t hi) {
    if (hi == lo) return kEmpty;
    const uint8_t c = buf[lo];
    return c == '>' ? kHeader : (c == '@' || c == '+') ? kBad : kSeq;
}
// ... and the bytes it adds to the open record
RS_HD uint32_t fa_seq_len(uint32_t cls, uint32_t lo, uint32_t hi) { return cls == kSeq ? hi - lo : 0; }

// the name of the header line [lo, hi): the line minus its first byte
RS_HD void name_of(uint32_t lo, uint32_t hi, uint32_t *pos, uint32_t *len) {
    *pos = lo + (hi > lo ? 1 : 0);
    *len = hi - *pos;
}

// FASTQ: the header line [lo, hi) belongs to a FASTA file
RS_HD bool fq_bad_header(const uint8_t *buf, uint32_t lo, uint32_t hi) { return hi > lo && buf[lo] == '>'; }
RS_HD uint32_t fq_records(uint32_t n_nl) { return n_nl / 4; }
RS_HD uint64_t fq_consumed(const uint32_t *nl, uint32_t n_nl) { return n_nl / 4 ? (uint64_t)nl[4 * (uint64_t)(n_nl / 4) - 1] + 1 : 0; }

// FASTA: records of a view with m headers, and what the view consumes (last_hdr: the line index of h(m-1), any value when m = 0)
RS_HD uint32_t fa_records(uint32_t m, bool last) { return last ? m : m ? m - 1 : 0; }
RS_HD uint64_t fa_consumed(const uint32_t *nl, uint32_t n_nl, uint64_t n, uint32_t m, uint32_t last_hdr, bool last, bool seen_header) {
    if (last) return n;
    if (m) return line_lo(nl, last_hdr);
    if (seen_header) return 0;
    return n_nl ? (uint64_t)nl[n_nl - 1] + 1 : 0;
}

}  // namespace rs
}  // namespace hast
