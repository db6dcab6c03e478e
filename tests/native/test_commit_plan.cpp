// test_commit_plan.cpp -- the plan of the partitioned commit (hast_amd/csrc/commit_plan.h) on its own, host only: for a grid of
// (reads, barcodes, span override) the bins cover the barcodes, the regions of the scratch are disjoint, aligned and inside its
// bytes, a bin's two counters share one 128-byte line that no other bin touches, and usable() refuses what the kernels cannot hold.
//   test_commit_plan        exit 0 and "commit plan ok: <plans> plans" on stderr; 1 and the first broken rule otherwise
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../hast_amd/csrc/commit_plan.h"

using namespace hast::commit;

static int fails = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, "\n");                                \
            if (++fails > 20) exit(1);                            \
        }                                                         \
    } while (0)

static void check_plan(size_t n_reads, size_t n_bc, uint32_t span) {
    const Plan p = plan_for(n_reads, n_bc, span);
#define AT "reads %zu barcodes %zu span %u", n_reads, n_bc, span
    CHECK(p.span_bits >= kMinSpanBits && p.span_bits <= kMaxSpanBits, AT);
    if (span >= kMinSpanBits && span <= kMaxSpanBits) CHECK(p.span_bits == span, AT);
    else CHECK(p.span_bits == span_bits_for(n_bc), AT);
    // the bins cover the barcodes and the last one is not empty
    CHECK(((uint64_t)p.n_bins << p.span_bits) >= n_bc, AT);
    CHECK(n_bc == 0 ? p.n_bins == 0 : ((uint64_t)(p.n_bins - 1) << p.span_bits) < n_bc, AT);
    // a bin holds at least the mean and some slack (or as much as 31 bits say: such a plan is not usable)
    if (p.n_bins) CHECK(p.cap == 0x7FFFFFFFu || ((uint64_t)p.cap * p.n_bins >= n_reads && p.cap >= 2048), AT);
    // regions: in this order, each on a 256-byte border, none overlapping, all inside the scratch
    const size_t at[6] = {p.over_n_at, p.lines_at, p.recs_at, p.over_ids_at, p.over_votes_at, p.bytes};
    const size_t len[5] = {2 * sizeof(uint64_t), (size_t)p.n_bins * kLine, (size_t)p.n_bins * p.cap * 4, n_reads * 4, n_reads * 8};
    for (int r = 0; r < 5; ++r) {
        CHECK(at[r] % kAlign == 0, AT);
        CHECK(at[r] + len[r] <= at[r + 1], AT);
    }
    CHECK(p.bytes % kAlign == 0, AT);
    // a bin's fill and valid words (as the kernels address them): one 128-byte line, and bin b's is the b-th line of the region
    CHECK(p.lines_at % kLine == 0, AT);
    const uint32_t probe[] = {0, 1, 2, p.n_bins / 2, p.n_bins ? p.n_bins - 1 : 0};
    for (uint32_t b : probe) {
        if (b >= p.n_bins) continue;
        const size_t fill = p.lines_at + ((size_t)b * kLineWords) * 4, valid = p.lines_at + ((size_t)b * kLineWords + 1) * 4;
        CHECK(fill / kLine == valid / kLine, AT);
        CHECK(fill / kLine - p.lines_at / kLine == b, AT);
        CHECK(valid + 4 <= p.recs_at, AT);
    }
    // LDS of the two kernels
    CHECK(p.lds_bins == (size_t)12 << p.span_bits && p.lds_bins <= kMaxLdsBins && kMaxLdsBins <= 160 * 1024, AT);
    CHECK(p.lds_partition == (size_t)p.n_bins * 12 + (size_t)kGroupRecs * 4, AT);
    // usable: what it must refuse, forced or not
    for (int forced = 0; forced < 2; ++forced) {
        CHECK(!usable(p, n_reads, 256, forced), AT);
        CHECK(!usable(p, n_reads, 1u << 20, forced), AT);
        const bool u = usable(p, n_reads, 255, forced);
        if (n_reads >= ((size_t)1 << 31) || n_reads == 0 || p.n_bins == 0 || p.n_bins > kMaxBins || (uint64_t)p.cap * 255 >= ((uint64_t)1 << 32)) CHECK(!u, AT);
        else if (forced) CHECK(u && usable(p, n_reads, 0, true) && usable(p, n_reads, 130, true), AT);
        else CHECK(u == (p.n_bins >= 128 && n_reads >= ((size_t)1 << 21)), AT);
        if (u) {
            CHECK(p.lds_partition <= kMaxLdsPartition && kMaxLdsPartition <= 160 * 1024, AT);
            CHECK((uint64_t)p.n_bins * p.cap < ((uint64_t)1 << 40), AT);
        }
    }
#undef AT
}

int main() {
    std::vector<size_t> reads = {0, 1, 2, 255, 16383, 16384, 16385, 40000, (size_t)1 << 21, ((size_t)1 << 21) - 1, 5000000, 48000000, ((size_t)1 << 31) - 1,
                                 (size_t)1 << 31, ((size_t)1 << 31) + 1, (size_t)1 << 33};
    std::vector<size_t> barcodes = {0, 1, 255, 256, 257, 511, 512, 513, 1000, 65536, 65537, 262144, 262145, 1 << 20, (1 << 20) + 1, 2000000, 10000000,
                                    ((size_t)kMaxBins << kMaxSpanBits) - 1, (size_t)kMaxBins << kMaxSpanBits, ((size_t)kMaxBins << kMaxSpanBits) + 1, (size_t)1 << 31};
    for (uint32_t sb = kMinSpanBits; sb <= kMaxSpanBits; ++sb) {                 // one past every bin border of every span
        barcodes.push_back(((size_t)3 << sb) + 1);
        barcodes.push_back((size_t)3 << sb);
    }
    size_t plans = 0;
    for (size_t r : reads)
        for (size_t b : barcodes)
            for (uint32_t span : {0u, 7u, 8u, 11u, 12u, 13u, 14u}) {
                check_plan(r, b, span);
                ++plans;
            }
    // the named refusals, spelled out
    {
        const Plan p = plan_for(48000000, 10000000);
        CHECK(p.span_bits == 13 && p.n_bins == 1221 && usable(p, 48000000, 130, false) && !usable(p, 48000000, 256, true), "C3");
        CHECK(!usable(plan_for((size_t)1 << 31, 10000000), (size_t)1 << 31, 130, true), "2^31 reads");
        const Plan one = plan_for(48000000, 1);                                  // one bin of 48M reads: cap * 255 >= 2^32
        CHECK(one.n_bins == 1 && (uint64_t)one.cap * 255 >= ((uint64_t)1 << 32) && !usable(one, 48000000, 130, true), "cap * 255");
        const Plan small = plan_for(40000, 1000);
        CHECK(small.n_bins == 4 && small.span_bits == 8 && small.cap == 10000 + 5000 + 2048 && usable(small, 40000, 130, true) && !usable(small, 40000, 130, false), "4 bins");
    }
    if (fails) return 1;
    fprintf(stderr, "commit plan ok: %zu plans\n", plans);
    return 0;
}
