// rb_core.h -- "read bins": the rules by which `classify_read --bin-reads` routes every read, as its bytes lie in the input, to one of
// three runs (haplotype0, haplotype1, ambiguous).  Plain integer and double code: the kernels (rs_kernels.hip: k_rb_*) and the host
// model (rb_host.h, tests/native/test_rb_core.cpp) step the same functions, and so do the rows (format_rows of rr_host.h, rr_core.h),
// so that a row and a bin can never disagree.
//
//   class    from the votes v0, v1 and the two set sizes t0, t1 (s03:110-133, 215-216): d0 = (double)v0 / t0, d1 = (double)v1 / t1;
//            neither above 0: ambiguous (2); else d1 > d0: haplotype1 (1); else haplotype0 (0).  A set size of 0 (inf, NaN) goes through
//            the same expressions.  The division is IEEE fp64 on both sides: no build of this project turns on fast-math.
//   extent   of a record in a view, in the terms of rs_core.h (nl[], line_lo, hdr_line[]):
//            FASTQ  record i = [line_lo(4i), nl[4i+3] + 1): the extents tile [0, consumed).
//            FASTA  record r = [line_lo(hdr_line[r]), line_lo(hdr_line[r+1])); the last record of a file's last view ends behind the
//                   view's last newline.  Blank lines and '\r' inside an extent stay as they lie; what belongs to no record (junk in
//                   front of a file's first header, an unterminated last line) is written nowhere.
//   run      the extents of one class, back to back, in input order.
#pragma once
#include <stdint.h>

#include "rs_core.h"

namespace hast {
namespace rb {

enum : uint32_t { kHap0 = 0, kHap1 = 1, kAmbiguous = 2, kClasses = 3 };

RS_HD double density(uint32_t votes, double total) { return (double)votes / total; }
RS_HD uint32_t class_of(double d0, double d1) {
    if (!(d0 > 0) && !(d1 > 0)) return kAmbiguous;
    return d1 > d0 ? kHap1 : kHap0;
}
RS_HD uint32_t read_class(uint32_t v0, uint32_t v1, uint32_t t0, uint32_t t1) { return class_of(density(v0, (double)t0), density(v1, (double)t1)); }

// FASTQ: record i of a view with the newline index nl
RS_HD void fq_extent(const uint32_t *nl, uint32_t i, uint32_t *lo, uint32_t *hi) {
    *lo = rs::line_lo(nl, 4 * i);
    *hi = nl[4 * i + 3] + 1;
}
// FASTA: record r of a view with n_nl newlines and m header lines (r = m - 1 is a record only in a file's last view)
RS_HD void fa_extent(const uint32_t *nl, uint32_t n_nl, const uint32_t *hdr_line, uint32_t m, uint32_t r, uint32_t *lo, uint32_t *hi) {
    *lo = rs::line_lo(nl, hdr_line[r]);
    *hi = rs::line_lo(nl, r + 1 < m ? hdr_line[r + 1] : n_nl);
}

}  // namespace rb
}  // namespace hast
