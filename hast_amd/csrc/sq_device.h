// sq_device.h -- what sq_kernels.hip and sq_api.cpp share: raw four-line FASTQ in HBM -> the k-mer counter's base stream in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nl_index.h"
#include "sq_core.h"

namespace hast {

struct SqState {               // device memory; its first 40 bytes are hast_sq_result
    uint64_t consumed, out_bytes, records, bases;
    uint32_t flags, first_bad;
    uint32_t n_nl, n_rec;      // newlines of the block, records framed (n_nl / 4)
};

constexpr uint32_t kSqRecTile = 256;     // records per tile of the prefix sum of the output lengths

// the scratch a block of up to max_in bytes needs in the worst case, a block that is all newlines
struct SqScratchPlan {
    size_t tile_cnt, nl, r_src, r_len, r_tile, state, total;      // offsets of the parts, 256-byte aligned, and the sum
};
inline SqScratchPlan sq_scratch_plan(size_t max_in) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n_tiles = nl_tiles(max_in), max_rec = max_in / 4 + 1, rec_tiles = max_rec / kSqRecTile + 2;
    SqScratchPlan p;
    size_t at = 0;
    p.tile_cnt = at; at += up(n_tiles * 4);
    p.nl = at;       at += up(nl_index_words(max_in) * 4);
    p.r_src = at;    at += up(max_rec * 4);
    p.r_len = at;    at += up(max_rec * 4);
    p.r_tile = at;   at += up(rec_tiles * 4);
    p.state = at;    at += up(sizeof(SqState));
    p.total = at;
    return p;
}

// frames d_in[0, n_in) into d_out (room for n_in bytes); *d_st holds the result when the stream has run.  n_in < 2^32 - 4096.
hipError_t launch_sq_frame(const uint8_t *d_in, size_t n_in, uint8_t *d_out, uint8_t *d_scratch, const SqScratchPlan &plan, hipStream_t s);

// ---- FASTA (sq_core.h, namespace sqfa; the kernels are sq_fasta_kernels.hip) -------------------------------------------------------
struct SqFaState {             // device memory; its first 40 bytes are hast_sq_result
    uint64_t consumed, out_bytes, records, bases;
    uint32_t flags, first_bad;
    uint32_t n_nl, n_lines;    // newlines of the view; its lines (one more with `last` and bytes behind the last newline)
    uint32_t lines_bytes;      // what the lines emit: out_bytes without the closing '\n'
};

constexpr uint32_t kSqFaTile = 256;          // lines per tile of the two prefix sums

// the scratch a view of up to max_in bytes needs in the worst case: a newline at every byte (the most lines), ">\n" repeated (the
// most headers); both stay within one line per byte and one more
struct SqFaScratchPlan {
    size_t tile_cnt, nl, tile_h, tile_e, line_dst, state, total;      // offsets of the parts, 256-byte aligned, and the sum
};
inline SqFaScratchPlan sq_fa_scratch_plan(size_t max_in) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n_tiles = nl_tiles(max_in), max_lines = max_in + 1, line_tiles = max_lines / kSqFaTile + 2;
    SqFaScratchPlan p;
    size_t at = 0;
    p.tile_cnt = at; at += up(n_tiles * 4);
    p.nl = at;       at += up(nl_index_words(max_in) * 4);
    p.tile_h = at;   at += up(line_tiles * 4);
    p.tile_e = at;   at += up(line_tiles * 4);
    p.line_dst = at; at += up((max_lines + 1) * 4);
    p.state = at;    at += up(sizeof(SqFaState));
    p.total = at;
    return p;
}

// frames the view d_in[0, n_in) into d_out (room for n_in + 1 bytes); in_flags: SQ_FA_OPEN | SQ_FA_LAST.  n_in < 2^32 - 4096.
hipError_t launch_sq_fasta_frame(const uint8_t *d_in, size_t n_in, uint8_t *d_out, unsigned in_flags, uint8_t *d_scratch, const SqFaScratchPlan &plan,
                                 hipStream_t s);

}  // namespace hast
