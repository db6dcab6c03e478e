// commit_plan.h -- the PLAN of a partitioned commit (hast_kernels.hip, "partitioned commit"): how many barcodes a bin spans, how many
// bins there are, what a bin can hold, and where everything lies in the scratch buffer.  Host-only integer code, no HIP: the allocator
// (hast_api.cpp) and the launcher (hast_kernels.hip) share this one description, tests/native/test_commit_plan.cpp steps it on its own.
//
// THE SCRATCH, every region on a 256-byte border:
//   [over_n       2 x u64   ] lengths of the overflow list; launches alternate between the two (see below)
//   [lines        n_bins x 128 B] word 0 of a bin's line = bin_fill (records reserved), word 1 = bin_valid (first failed reservation);
//                               a bin has a line of its own: the reservations of different bins never meet in one line
//   [bin_recs     n_bins x cap x u32] compressed records (span_bits of barcode inside the bin, 8 + 8 bits of votes)
//   [over_ids     n_reads x u32 ] what found no room in its bin ...
//   [over_votes   n_reads x u64 ] ... as rows k_commit_votes reads
//
// THE SCRATCH CLEANS ITSELF.  It is initialised when it is laid out (lines = {0, 0xFFFFFFFF}, over_n = {0, 0}); afterwards the
// workgroup of bin b in k_commit_bins, the last reader of line b, puts it back to {0, 0xFFFFFFFF}, and a launch that counts its
// overflow in over_n[p] puts over_n[p ^ 1] -- which the launch before it has long read -- back to 0.  No fill per launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hast {
namespace commit {

constexpr uint32_t kMinSpanBits = 8, kMaxSpanBits = 13;      // 256 .. 8192 barcodes per bin (span + 8 + 8 bits per record, 12 B of LDS per barcode)
constexpr uint32_t kMaxBins = 4096;                          // k_commit_partition scans 4 bins per thread
constexpr uint32_t kGroupRecs = 16384;                       // records a workgroup of k_commit_partition takes
constexpr uint32_t kMaxVotes = 255;                          // a vote is 8 bits of a record
constexpr size_t kLine = 128, kLineWords = kLine / 4, kAlign = 256;

// ~1000 bins where the barcodes allow it; span_override (a measurement switch) replaces the choice when it is in range
inline uint32_t span_bits_for(size_t n_barcodes, uint32_t span_override = 0) {
    if (span_override >= kMinSpanBits && span_override <= kMaxSpanBits) return span_override;
    uint32_t lg = 0;
    while (lg < 63 && ((size_t)1 << lg) < n_barcodes) ++lg;
    const uint32_t want = lg > 10 ? lg - 10 : 0;
    return want < kMinSpanBits ? kMinSpanBits : (want > kMaxSpanBits ? kMaxSpanBits : want);
}

struct Plan {
    uint32_t span_bits, n_bins, cap;                         // cap: records a bin holds
    size_t over_n_at, lines_at, recs_at, over_ids_at, over_votes_at, bytes;
    size_t lds_partition, lds_bins;                          // dynamic LDS of the two kernels
};

inline size_t align_up(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }

inline Plan plan_for(size_t n_reads, size_t n_barcodes, uint32_t span_override = 0) {
    Plan p;
    p.span_bits = span_bits_for(n_barcodes, span_override);
    const uint64_t bins = ((uint64_t)n_barcodes + ((uint64_t)1 << p.span_bits) - 1) >> p.span_bits;
    p.n_bins = (uint32_t)(bins < 0xFFFFFFFFull ? bins : 0xFFFFFFFFull);
    const uint64_t mean = p.n_bins ? ((uint64_t)n_reads + p.n_bins - 1) / p.n_bins : 0;
    const uint64_t cap = mean + mean / 2 + 2048;
    p.cap = (uint32_t)(cap < 0x7FFFFFFFull ? cap : 0x7FFFFFFFull);
    p.over_n_at = 0;
    p.lines_at = kAlign;
    p.recs_at = align_up(p.lines_at + (size_t)p.n_bins * kLine);
    p.over_ids_at = align_up(p.recs_at + (size_t)p.n_bins * p.cap * 4);
    p.over_votes_at = align_up(p.over_ids_at + n_reads * 4);
    p.bytes = align_up(p.over_votes_at + n_reads * 8);
    p.lds_partition = (size_t)p.n_bins * 12 + (size_t)kGroupRecs * 4;
    p.lds_bins = (size_t)12 << p.span_bits;
    return p;
}

// possible: votes that fit a byte, bins the scan covers, 32-bit record indices, sums of a bin that fit 32 + 32 bits of LDS;
// worth it (unless forced): enough bins to fill the GPU and a large batch
inline bool usable(const Plan &p, size_t n_reads, uint32_t max_votes, bool forced) {
    if (max_votes > kMaxVotes || p.n_bins < 1 || p.n_bins > kMaxBins || n_reads < 1 || n_reads >= ((size_t)1 << 31)) return false;
    if ((uint64_t)p.cap * kMaxVotes >= ((uint64_t)1 << 32)) return false;
    return forced || (p.n_bins >= 128 && n_reads >= ((size_t)1 << 21));
}

// the largest dynamic LDS either kernel can be launched with (what their function attribute is raised to, once)
constexpr size_t kMaxLdsPartition = (size_t)kMaxBins * 12 + (size_t)kGroupRecs * 4, kMaxLdsBins = (size_t)12 << kMaxSpanBits;

}  // namespace commit
}  // namespace hast
