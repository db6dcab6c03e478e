// classify_tile.h -- the LDS TILE of the two classify kernels (k_classify_f in hast_filter.hip, k_classify in hast_kernels.hip): where every
// array of a workgroup's tile lies and how many bytes the tile takes.  Host and device integer code, no HIP include of its own: the kernels
// take their pointers from it, the host plan (classify_plan.h) takes the dynamic LDS size from bytes(), and
// tests/native/test_classify_plan.cpp steps it on its own.  Offsets are in bytes from the start of the dynamic LDS.
//
// A tile holds TR rows (reads, or segments of long reads).  Per row: ws() 64-bit words of packed bases (w64 + one pad word that
// window_bits reads into), the row's votes, offset, length and flag and -- strict rows only -- iw() 32-bit words of invalid-byte masks.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef HAST_HD                 // (hast_common.h's, where that came first: the .hip files include it in front of this header)
#if defined(__HIPCC__)
#define HAST_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HAST_HD inline
#endif
#endif

namespace hast {

// first-level sliding-minimum entries per row of k_classify_f: one per t-mer position and one more, rounded up to the 4 entries a lane
// of phase M stores at once (rows stay 16-byte aligned); a dense filter is probed on a fixed grid and has no first level
HAST_HD constexpr uint32_t l1_stride_for(uint32_t read_len, uint32_t t, bool dense) {
    return dense ? 0u : ((read_len >= t ? read_len - t + 1 : 0u) + 1 + 3) & ~3u;
}

constexpr int kQCap = 128;                                    // k_classify_f's queue entries per wave: < 64 waiting + <= 64 new
constexpr size_t kQueueBytes = (size_t)4 * 3 * kQCap * 4;     // [4 waves][lo, hi, read][kQCap] words

constexpr size_t kTileHeadBytes = 16;      // the workgroup's next tile (8 B); k_classify_f: + the tile's dirty flag; 16 keeps what follows 16-aligned
constexpr size_t kTileTailBytes = 64;      // behind the last array; no kernel reads into it: it is part of the size the LDS budgets were measured with

// ---- k_classify_f -------------------------------------------------------------------------
// 64 words behind the last row of s_l1.  The probe's lanes without a window read l1[p .. p + NT - g] of a clamped row; that stays
// inside the row (p < max_pos), so today these words are slack between s_l1 and s_pack.
constexpr size_t kL1PadWords = 64;

struct FilterTile {
    uint32_t TR, w64, l1_stride;
    bool strict;
    HAST_HD uint32_t ws() const { return w64 + 1; }
    HAST_HD uint32_t iw() const { return 2 * w64 + 1; }
    HAST_HD size_t l1_words() const { return (size_t)TR * l1_stride + kL1PadWords; }
    HAST_HD size_t pack_words() const { return (size_t)TR * ws(); }
    HAST_HD size_t tile_at() const { return 0; }
    HAST_HD size_t dirty_at() const { return 8; }
    HAST_HD size_t l1_at() const { return kTileHeadBytes; }                                               // [TR][l1_stride] u32 (+ kL1PadWords)
    HAST_HD size_t pack_at() const { return l1_at() + l1_words() * 4; }                                   // [TR][ws] u64
    HAST_HD size_t vote_at() const { return pack_at() + pack_words() * 8; }                               // [TR] u64
    HAST_HD size_t off_at() const { return vote_at() + (size_t)TR * 8; }                                  // [TR] u64
    HAST_HD size_t len_at() const { return off_at() + (size_t)TR * 8; }                                   // [TR] u32
    HAST_HD size_t flag_at() const { return len_at() + (size_t)TR * 4; }                                  // [TR] u32
    HAST_HD size_t queue_at() const { return flag_at() + (size_t)TR * 4; }                                // kQueueBytes
    HAST_HD size_t inv_at() const { return queue_at() + kQueueBytes; }                                    // [TR][iw] u32, strict only
    HAST_HD size_t bytes() const { return inv_at() + (strict ? (size_t)TR * iw() * 4 : 0) + kTileTailBytes; }
};

// ---- k_classify ---------------------------------------------------------------------------
// The m-mer hashes s_mh are [TR][mh_stride].  A lane without a window (past the tile's last one, or every lane when rows are shorter
// than K) takes the window minimum of row 0, position 0: W entries from the start of s_mh, which run past TR * mh_stride entries when
// the rows are short.  They land in the 16 words in front of s_inv and, for W > 16, in s_inv (strict) or in the W entries kept behind
// the last array for them: inside the tile either way, and never used.
constexpr size_t kMhGapWords = 16;

struct ExactTile {
    uint32_t TR, w64, mh_stride;
    bool strict;
    HAST_HD uint32_t ws() const { return w64 + 1; }
    HAST_HD uint32_t iw() const { return 2 * w64 + 1; }
    HAST_HD size_t pack_words() const { return (size_t)TR * ws(); }
    HAST_HD size_t mh_words() const { return (size_t)TR * mh_stride + kMhGapWords; }
    HAST_HD size_t tile_at() const { return 0; }
    HAST_HD size_t pack_at() const { return kTileHeadBytes; }                                             // [TR][ws] u64
    HAST_HD size_t vote_at() const { return pack_at() + pack_words() * 8; }                               // [TR] u64
    HAST_HD size_t off_at() const { return vote_at() + (size_t)TR * 8; }                                  // [TR] u64
    HAST_HD size_t len_at() const { return off_at() + (size_t)TR * 8; }                                   // [TR] u32
    HAST_HD size_t flag_at() const { return len_at() + (size_t)TR * 4; }                                  // [TR] u32
    HAST_HD size_t mh_at() const { return flag_at() + (size_t)TR * 4; }                                   // [TR][mh_stride] u32 (+ kMhGapWords)
    HAST_HD size_t inv_at() const { return mh_at() + mh_words() * 4; }                                    // [TR][iw] u32, strict only
    // (W = K - m + 1 m-mers per window is no part of where the arrays lie, only of the room behind them: the W entries above)
    HAST_HD size_t bytes(uint32_t W) const { return inv_at() + (strict ? (size_t)TR * iw() * 4 : 0) + (size_t)W * 4 + kTileTailBytes; }
};

}  // namespace hast
