// rs_device.h -- what rs_kernels.hip and rs_api.cpp share: a view of raw FASTA / FASTQ in HBM -> the reads of the per-read classifier
// (starts + lengths), their names back to back, and what the view consumes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nl_index.h"
#include "rs_core.h"

namespace hast {

struct RsState {               // device memory, copied to the host after the framing
    uint64_t consumed, records, bases, name_bytes;
    uint32_t flags;
    uint32_t n_nl;             // newlines of the view
    uint32_t n_hdr, seq_total; // FASTA: header lines; sequence bytes of all sequence lines
};

constexpr uint32_t kRsTile = 256;            // lines / records per tile of the prefix sums

// the scratch a view of up to max_view bytes needs in the worst case: all newlines, or FASTA records of two bytes (">\n")
struct RsScratchPlan {
    size_t tile_cnt, nl, line_tile_h, line_tile_s, line_dst, hdr_line, name_pos, name_len, name_tile, name_off, off, len, votes, state, total;
    size_t max_rec;
};
inline RsScratchPlan rs_scratch_plan(int format, size_t max_view) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const bool fasta = format == RS_FASTA;
    const size_t max_lines = max_view + 1, line_tiles = max_lines / kRsTile + 2;
    const size_t max_rec = (fasta ? max_view / 2 : max_view / 4) + 1, rec_tiles = max_rec / kRsTile + 2;
    RsScratchPlan p;
    size_t at = 0;
    p.tile_cnt = at;    at += up(nl_tiles(max_view) * 4);
    p.nl = at;          at += up(nl_index_words(max_view) * 4);
    p.line_tile_h = at; at += fasta ? up(line_tiles * 4) : 0;
    p.line_tile_s = at; at += fasta ? up(line_tiles * 4) : 0;
    p.line_dst = at;    at += fasta ? up((max_lines + 1) * 4) : 0;
    p.hdr_line = at;    at += fasta ? up(max_rec * 4) : 0;
    p.name_pos = at;    at += up(max_rec * 4);
    p.name_len = at;    at += up(max_rec * 4);
    p.name_tile = at;   at += up(rec_tiles * 4);
    p.name_off = at;    at += up((max_rec + 1) * 4);
    p.off = at;         at += up(max_rec * 8);
    p.len = at;         at += up(max_rec * 4);
    p.votes = at;       at += up(max_rec * 8);
    p.state = at;       at += up(sizeof(RsState));
    p.total = at;
    p.max_rec = max_rec;
    return p;
}

// Frames the view d_base[origin, origin + n) (d_base 16-byte aligned, n < 2^32 - 8192).  When the stream has run: the state block
// holds the result; off[r] / len[r] are the reads -- FASTQ: inside d_base, where they lie; FASTA: inside d_seq (room for n bytes,
// 16-byte aligned), compacted back to back -- and d_names (room for n bytes) / name_off[records + 1] the names.  Nothing outside the
// view is read; nothing is written at or behind d_seq + bases or d_names + name_bytes.
hipError_t launch_rs_frame(int format, const uint8_t *d_base, size_t origin, size_t n, bool last, bool seen_header, uint8_t *d_seq, uint8_t *d_names,
                           uint8_t *d_scratch, const RsScratchPlan &plan, hipStream_t s);

// ---- the read bins (`classify_read --bin-reads`, rules: rb_core.h) --------------------------------------------------------------
struct RbState {               // device memory, copied to the host behind the partition
    uint64_t count[3], raw_bytes[3];   // records and bytes per class
    uint64_t total;                    // raw_bytes[0] + [1] + [2]: the runs lie back to back in the output buffer
};

// scratch of its own, allocated when the bins are first switched on: per record its place and its offset in the output
struct RbScratchPlan {
    size_t order, dst, tile_cnt, tile_bytes, state, total;
};
inline RbScratchPlan rb_scratch_plan(const RsScratchPlan &rs) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t rec_tiles = rs.max_rec / kRsTile + 2;
    RbScratchPlan p;
    size_t at = 0;
    p.order = at;      at += up(rs.max_rec * 4);
    p.dst = at;        at += up((rs.max_rec + 1) * 4);
    p.tile_cnt = at;   at += up(3 * rec_tiles * 4);
    p.tile_bytes = at; at += up(3 * rec_tiles * 4);
    p.state = at;      at += up(sizeof(RbState));
    p.total = at;
    return p;
}

// Behind launch_rs_frame and the classification of the same view, on the same stream: the records of the view d_base[origin, origin + n)
// are classed by their votes (plan.votes of d_scratch) against the two set sizes and their extents copied to d_out (16-byte aligned,
// room for n bytes) as three runs back to back, class 0 first.  When the stream has run, the RbState of d_rb says how long they are.
// Nothing outside the view is read; nothing is written at or behind d_out + total.
hipError_t launch_rb_bin(int format, const uint8_t *d_base, size_t origin, size_t n, uint32_t total0, uint32_t total1, const uint8_t *d_scratch,
                         const RsScratchPlan &plan, uint8_t *d_rb, const RbScratchPlan &rb, uint8_t *d_out, hipStream_t s);

// ---- the rows (`classify_read --rows device`, rules: rr_core.h; kernels: rr_kernels.hip) -----------------------------------------
struct RrState {               // device memory, copied to the host behind the rows
    uint64_t total;            // bytes of all rows, whether they were written or not
    uint64_t count[3];         // reads per class
    uint32_t written;          // 1: the rows lie in the output; 0: they did not fit and not one byte was stored
    uint32_t pad;
};

// scratch for the rows of up to max_rec reads: per tile of kRsTile reads the bytes of its rows (64 bits) and its reads per class
struct RrScratchPlan {
    size_t tile_bytes, tile_cnt, state, total;
};
inline RrScratchPlan rr_scratch_plan(size_t max_rec) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t rec_tiles = max_rec / kRsTile + 2;
    RrScratchPlan p;
    size_t at = 0;
    p.tile_bytes = at; at += up(rec_tiles * 8);
    p.tile_cnt = at;   at += up(3 * rec_tiles * 4);
    p.state = at;      at += up(sizeof(RrState));
    p.total = at;
    return p;
}

// The rows of the n reads (n < 2^32) with the names d_names[d_name_off[r], d_name_off[r + 1]) and the votes d_votes[2 r], d_votes[2 r + 1]
// against the set sizes t0, t1 (both at least 1), back to back in read order to d_out (room for cap bytes).  When the stream has run,
// the RrState of d_rr holds the size and the counts; rows that need more than cap bytes, or 2^32 and more, are not written: nothing
// is stored at or behind d_out + min(total, cap) either way.  Reads the names and votes only.
hipError_t launch_rr_rows(const uint8_t *d_names, const uint32_t *d_name_off, const uint32_t *d_votes, size_t n, uint32_t t0, uint32_t t1, uint8_t *d_rr,
                          const RrScratchPlan &plan, uint8_t *d_out, uint64_t cap, hipStream_t s);

}  // namespace hast
