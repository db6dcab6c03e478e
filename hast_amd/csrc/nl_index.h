// nl_index.h -- the newline index of a byte range in HBM: where every '\n' of [lo, hi) lies, in order.  One implementation for every
// framer: a count per 4-KB tile, an exclusive scan of the counts (scan_device.h), then every tile writes its positions at its scanned
// base.
// The range may start and end at any address.  Tiles are cut at 16-byte boundaries of the ADDRESS; a 16-byte piece that straddles an
// edge of the range is read byte by byte, so nothing outside [lo, hi) is touched.
// A range the HOST knows (rs_, sq_, sq_fasta_, tx_kernels.hip) goes through k_nl_count / k_nl_index (nl_kernels.hip); the scan between
// them is each family's own: it also initialises its state.  k_fq_count / k_fq_index stay apart: their range is decided on the device
// (k_fq_begin, FqState) and they zero the tiles outside it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define NL_HD __host__ __device__ __forceinline__
#else
#define NL_HD inline
#endif

namespace hast {

constexpr uint32_t kNlTile = 4096;               // bytes per tile = 256 lanes x 16 B

// tiles of a range of n bytes that may start at any address (up to 15 bytes into its first tile), with one to spare
constexpr size_t nl_tiles(size_t n) { return (n + 15) / kNlTile + 2; }
// words the index of n bytes needs in the worst case, a range that is all newlines
constexpr size_t nl_index_words(size_t n) { return n + 16; }
// the grid of a kernel whose workgroups loop over tiles of `per` items: the tiles of the worst case, at least 1, at most `cap`
inline uint32_t capped_grid(size_t items, uint32_t per, uint32_t cap = 2048) {
    const size_t t = (items + per - 1) / per;
    return (uint32_t)(t < 1 ? 1 : t < cap ? t : cap);
}

// a range as the index wants it: the 16-byte boundary in front of it and the bytes [lo, hi) behind that, lo in 0..15
struct NlRange {
    const uint8_t *base16;
    uint64_t lo, hi;
    uint32_t tiles() const { return (uint32_t)((hi + kNlTile - 1) / kNlTile); }
    uint32_t grid() const { return tiles() ? tiles() : 1; }
};
inline NlRange nl_range(const uint8_t *p, size_t n) {
    const uint64_t lo = reinterpret_cast<uintptr_t>(p) & 15;
    return NlRange{p - lo, lo, lo + n};
}
struct NlSides {               // one or two ranges a launch, and where each side's tile counts and offsets go
    NlRange r[2];
    uint32_t *tile_cnt[2], *nl[2];
};

// bit i set <=> byte i of w (the byte at the lowest address first) is '\n'
NL_HD uint32_t nl_bits4(uint32_t w) {
    const uint32_t y = w ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;         // 0x80 in every zero byte, exact
    return ((z >> 7) * 0x00204081u) >> 21 & 0xFu;                                         // bits 0,8,16,24 -> 4 adjacent bits
}

}  // namespace hast

#if defined(__HIPCC__) || defined(__CUDACC__)
#include "scan_device.h"

namespace hast {

// bit i set <=> base16[at + i] == '\n', for the 16 bytes at the 16-B aligned base16 + at; only bytes inside [lo, hi) are read
__device__ __forceinline__ uint32_t nl_mask16(const uint8_t *base16, uint64_t at, uint64_t lo, uint64_t hi) {
    if (at + 16 <= lo || at >= hi) return 0;
    if (at >= lo && at + 16 <= hi) {
        const uint4 v = *reinterpret_cast<const uint4 *>(base16 + at);
        return nl_bits4(v.x) | nl_bits4(v.y) << 4 | nl_bits4(v.z) << 8 | nl_bits4(v.w) << 12;
    }
    uint32_t m = 0;
    for (uint32_t i = 0; i < 16; ++i)
        if (at + i >= lo && at + i < hi && base16[at + i] == '\n') m |= 1u << i;
    return m;
}

// Workgroup of 256 = tile `tile` of base16 (bytes [tile * kNlTile, (tile + 1) * kNlTile)): the newlines of the tile inside [lo, hi).
// Returns their number.
__device__ __forceinline__ uint32_t nl_tile_count(const uint8_t *base16, uint64_t tile, uint64_t lo, uint64_t hi) {
    __shared__ uint32_t s_wave[4];
    return block_sum_256(__popc(nl_mask16(base16, tile * kNlTile + threadIdx.x * 16, lo, hi)), s_wave);
}

// The same workgroup once the counts are scanned: nl[tile_base[tile] ...] = position - origin of every newline of the tile, in order.
__device__ __forceinline__ void nl_tile_index(const uint8_t *base16, uint64_t tile, uint64_t lo, uint64_t hi, uint64_t origin, const uint32_t *tile_base,
                                              uint32_t *nl) {
    __shared__ uint32_t s_wave[4];
    const uint64_t at = tile * kNlTile + threadIdx.x * 16;
    uint32_t m = nl_mask16(base16, at, lo, hi);
    uint32_t to = tile_base[tile] + block_exclusive_sum_256(__popc(m), s_wave);
    while (m) {
        const uint32_t b = __ffs(m) - 1;
        nl[to++] = (uint32_t)(at + b - origin);
        m &= m - 1;
    }
}

// (nl_kernels.hip) 1 or 2 ranges in one launch of `grid` tiles each
void launch_nl_count(const NlSides &in, uint32_t sides, uint32_t grid, hipStream_t s);
void launch_nl_index(const NlSides &in, uint32_t sides, uint32_t grid, hipStream_t s);

}  // namespace hast
#endif
