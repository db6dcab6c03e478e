// tx_device.h -- what tx_kernels.hip and tx_api.cpp share: two buffers of raw FASTQ in HBM -> two runs of 10x records in HBM.
//
// ALL OFFSETS ARE 32 BITS.  A step takes at most kTxMaxIn = 128 MB (2^27 bytes) a side.  The shortest record is four bytes (four
// empty lines), so a side holds at most 2^27 / 4 = 2^25 records.  A record grows by at most 106 bytes: read 1's header (one byte at
// least) becomes a name line of at most 24 + 20 + 16 = 60, and 16 + 7 + 23 = 46 bytes (value, ATCGAGN, the quality's head) are put
// in.  So an output run is at most 2^25 * (4 + 106) = 3 690 987 520 bytes < 2^32 = 4 294 967 296, and every offset into an input,
// every running sum of record lengths and both totals fit 32 bits.  N itself is 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nl_index.h"
#include "tx_plan.h"

namespace hast {

constexpr size_t kTxMaxIn = 128u << 20;
constexpr uint32_t kTxTile = 256;        // pairs per tile of the prefix sums

struct TxDevState {            // device memory, copied to the host behind every step
    uint64_t consumed[2], pairs, used, out_bytes[2];
    uint32_t lines[2];
    uint32_t refused, pad;     // refused != 0: an output is larger than its room, nothing was written
};

// the scratch a step over up to max_in bytes a side needs in the worst case, inputs that are all newlines
struct TxScratchPlan {
    size_t tile_cnt[2], nl[2], slot, tile_kept, tile_out[2], state, total;      // offsets of the parts, 256-byte aligned, and the sum
};
inline TxScratchPlan tx_scratch_plan(size_t max_in) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n_tiles = nl_tiles(max_in), max_pairs = max_in / 4 + 1, pair_tiles = max_pairs / kTxTile + 2;
    TxScratchPlan p;
    size_t at = 0;
    for (int s = 0; s < 2; ++s) { p.tile_cnt[s] = at; at += up(n_tiles * 4); }
    for (int s = 0; s < 2; ++s) { p.nl[s] = at; at += up(nl_index_words(max_in) * 4); }
    p.slot = at;      at += up(max_pairs * 4);
    p.tile_kept = at; at += up(pair_tiles * 4);
    for (int s = 0; s < 2; ++s) { p.tile_out[s] = at; at += up(pair_tiles * 4); }
    p.state = at;     at += up(sizeof(TxDevState));
    p.total = at;
    return p;
}

struct TxStepArgs {
    const uint8_t *d_in[2];
    size_t n_in[2];
    uint8_t *d_out[2];
    size_t cap[2];
    uint64_t used;             // N so far
    const tx::TableSlot *d_table;
    uint32_t n_slots;
};

// one step on stream s; the TxDevState at d_scratch + plan.state holds the result when the stream has run.  n_in[] <= kTxMaxIn.
hipError_t launch_tx_step(const TxStepArgs &a, uint8_t *d_scratch, const TxScratchPlan &plan, hipStream_t s);

}  // namespace hast

// what tx_feed.cpp needs of a hast_tx (tx_api.cpp): whose it is, what it was created for, the map for the steps that go to the host
// model, and where a step leaves its TxDevState in device memory
struct hast_tx;
struct hast_tx_map;
struct hast_ctx;
namespace hast {
struct TxParts {
    hast_ctx *ctx;
    int device;
    size_t max_in;
    const hast_tx_map *map;
    const TxDevState *d_state;
};
TxParts tx_parts_of(const hast_tx *t);
}  // namespace hast
