// nl_index.h -- the newline index of a byte range in HBM: where every '\n' of [lo, hi) lies, in order.  One implementation for the
// framers of `classify` (fq_kernels.hip) and of stage 00's device ingest (sq_kernels.hip): a count per 4-KB tile, an exclusive scan of
// the counts (scan_device.h), then every tile writes its positions at its scanned base.
// The range may start and end at any address.  Tiles are cut at 16-byte boundaries of the ADDRESS; a 16-byte piece that straddles an
// edge of the range is read byte by byte, so nothing outside [lo, hi) is touched.
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
// the grid of a kernel whose workgroups loop over tiles of `per` items: the tiles of the worst case, at least 1, at most 2048
inline uint32_t capped_grid(size_t items, uint32_t per) {
    const size_t t = (items + per - 1) / per;
    return (uint32_t)(t < 1 ? 1 : t < 2048 ? t : 2048);
}

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

}  // namespace hast
#endif
