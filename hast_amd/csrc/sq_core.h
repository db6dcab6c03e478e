// sq_core.h -- the rules by which a block of raw four-line FASTQ becomes the k-mer counter's base stream (stage 00 ingest on the
// device).  Plain integer code: the framing kernels (sq_kernels.hip) and the host model (tests/native/test_sq_core.cpp) step the same
// functions.  The rules for FASTA (namespace sqfa, `--device-fasta`) are at the end of the file.
//
// The stream is what SeqParser (seqstream.h) hands its sink: for every record the bytes of the sequence line, the '\r's in front of
// the line break stripped, then one '\n'.  The device path takes exactly the inputs on which "a record is four lines" and SeqParser
// agree, and refuses every other block as a whole.  Record i of a block is its lines 4i .. 4i+3; with the lengths taken after the
// trailing '\r's are stripped (SeqParser::line):
//   header     length >= 1, first byte '@'
//   sequence   length Ls; if Ls > 0 its first byte is not '+' (the parser would take the line for the separator line)
//   third line length >= 1, first byte '+'
//   quality    length == Ls
// A record yields Ls + 1 bytes, also when Ls == 0 (the parser calls separator() at the '+' line).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SQ_HD __host__ __device__ __forceinline__
#else
#define SQ_HD inline
#endif

// the flags of hast_sq_result (include/hast.h has the same values under HAST_SQ_*)
#define SQ_NOT_FOUR_LINE 1u
#define SQ_NO_RECORD 2u

namespace hast {
namespace sq {

constexpr uint32_t kNoBad = 0xFFFFFFFFu;         // first_bad of a block that breaks no rule

// length of the line [lo, hi) without the '\r's at its end
SQ_HD uint32_t line_len(const uint8_t *buf, uint32_t lo, uint32_t hi) {
    while (hi > lo && buf[hi - 1] == '\r') --hi;
    return hi - lo;
}

// Record whose first line starts at `start` and whose four lines end with the newlines at n0 < n1 < n2 < n3 (offsets into buf).
// True when it keeps the rules; then the sequence is buf[start_seq, start_seq + ls).
SQ_HD bool record(const uint8_t *buf, uint32_t start, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t *seq_at, uint32_t *ls) {
    const uint32_t lh = line_len(buf, start, n0), l_s = line_len(buf, n0 + 1, n1), lp = line_len(buf, n1 + 1, n2), lq = line_len(buf, n2 + 1, n3);
    *seq_at = n0 + 1;
    *ls = l_s;
    if (lh < 1 || buf[start] != '@') return false;
    if (l_s > 0 && buf[n0 + 1] == '+') return false;
    if (lp < 1 || buf[n1 + 1] != '+') return false;
    return lq == l_s;
}

// record i of a block from its newline index: nl[j] is the offset of the block's j-th newline
SQ_HD bool record_at(const uint8_t *buf, const uint32_t *nl, uint32_t i, uint32_t *seq_at, uint32_t *ls) {
    const uint32_t start = i ? nl[4 * (uint64_t)i - 1] + 1 : 0;
    return record(buf, start, nl[4 * (uint64_t)i], nl[4 * (uint64_t)i + 1], nl[4 * (uint64_t)i + 2], nl[4 * (uint64_t)i + 3], seq_at, ls);
}

}  // namespace sq

// ---- FASTA (`unshared_kmers --device-fasta`): the stream SeqParser hands its sink in FASTA mode, view by view ----------------------
// A view is [bytes carried from the view before | new bytes].  Its lines are the newline-terminated ones and, in a view framed with
// `last`, the bytes behind the last newline if there are any (SeqParser::finish).  Per line, the '\r's at its end stripped:
//   length 0        nothing
//   first byte '>'  a header: one record; one '\n' if a record is open, i.e. a header came earlier in this INPUT -- in an earlier view
//                   (open_in) or earlier in this one
//   anything else   the line's bytes as they lie, '@' and '+' lines and non-bases included (the counter breaks at non-bases)
// With `last` one closing '\n' follows if a record is open at the end of the view.  There is no format error behind an input's first
// byte.  The kernels (sq_fasta_kernels.hip) and the host model (tests/native/test_sq_fasta.cpp) step these functions.
#define SQ_FA_OPEN 1u
#define SQ_FA_LAST 2u

namespace sqfa {

constexpr uint32_t kNothing = 0, kHeader = 1, kSequence = 2;

// lines of a view of n_in bytes with n_nl newlines, nl[j] the offset of the j-th
SQ_HD uint32_t n_lines(const uint32_t *nl, uint32_t n_nl, uint64_t n_in, bool last) {
    const uint64_t behind = n_nl ? (uint64_t)nl[n_nl - 1] + 1 : 0;
    return n_nl + (last && behind < n_in ? 1u : 0u);
}
SQ_HD uint32_t line_lo(const uint32_t *nl, uint32_t j) { return j ? nl[j - 1] + 1 : 0; }
SQ_HD uint32_t line_hi(const uint32_t *nl, uint32_t n_nl, uint64_t n_in, uint32_t j) { return j < n_nl ? nl[j] : (uint32_t)n_in; }

// class of the line [lo, hi); *len: its length without the '\r's at its end
SQ_HD uint32_t line_class(const uint8_t *buf, uint32_t lo, uint32_t hi, uint32_t *len) {
    *len = sq::line_len(buf, lo, hi);
    return *len == 0 ? kNothing : buf[lo] == '>' ? kHeader : kSequence;
}

// What a line puts into the stream if every header emitted its '\n': the sums of these are what the kernels scan.  Only the view's
// first header may emit none, so with `raw` the sum over the lines in front of a line and `hdrs` the headers among them:
SQ_HD uint32_t raw_emit(uint32_t cls, uint32_t len) { return cls == kHeader ? 1u : cls == kSequence ? len : 0u; }
// ... the line's bytes start at
SQ_HD uint32_t line_dst(uint32_t raw, uint32_t hdrs, bool open_in) { return raw - (!open_in && hdrs ? 1u : 0u); }
// ... and it emits
SQ_HD uint32_t emit(uint32_t cls, uint32_t len, uint32_t hdrs, bool open_in) {
    return cls == kHeader ? (open_in || hdrs ? 1u : 0u) : cls == kSequence ? len : 0u;
}

// the results of a view with m headers whose lines' raw_emit sum to raw_total
SQ_HD uint64_t consumed(const uint32_t *nl, uint32_t n_nl, uint64_t n_in, bool last) { return last ? n_in : n_nl ? (uint64_t)nl[n_nl - 1] + 1 : 0; }
SQ_HD uint32_t closing(uint32_t m, bool open_in, bool last) { return last && (open_in || m) ? 1u : 0u; }
SQ_HD uint64_t bases(uint32_t raw_total, uint32_t m) { return raw_total - m; }

}  // namespace sqfa
}  // namespace hast
