// rows_device.h -- what rows_api.cpp (host) and rows_kernels.hip (device) share: the arrays of the output table's device step as they
// lie in device memory, and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rows_core.h"

namespace hast {
namespace rows {

// rows a workgroup of 256 scans and stages at a time (two per lane): 512 x 61 B of table text at most, 31 KB of LDS
constexpr uint32_t kTile = 512;
inline size_t n_tiles(size_t n) { return (n + kTile - 1) / kTile; }

// what a lane of k_rows_key leaves per id beside the key: the row's length, its list line's length and its list (1..3)
__host__ __device__ inline uint32_t meta_pack(uint32_t row_len, uint32_t line_len, uint32_t list) { return row_len | line_len << 8 | list << 16; }
__host__ __device__ inline uint32_t meta_row_len(uint32_t m) { return m & 0xFF; }
__host__ __device__ inline uint32_t meta_line_len(uint32_t m) { return (m >> 8) & 0xFF; }
__host__ __device__ inline uint32_t meta_list(uint32_t m) { return (m >> 16) & 3; }

// bytes in front of a tile, of the table and of each list; entry n_tiles holds the totals
struct TileBase {
    uint64_t at[4];
};

// a lane per id: key, id, meta, list by id; flags[0] |= any_sep, flags[1] |= past_int (zeroed by the caller)
hipError_t launch_key(const uint8_t *d_text16, const uint64_t *d_counts, size_t n, uint64_t n0, uint64_t n1, double w0, double w1, uint64_t *d_hi, uint64_t *d_lo,
                      uint32_t *d_id, uint32_t *d_meta, uint8_t *d_list, uint32_t *d_flags, hipStream_t s);
// d_out[r] = d_by_id[d_ids[r]]: the high words in the order the first pass left
hipError_t launch_gather(const uint64_t *d_by_id, const uint32_t *d_ids, size_t n, uint64_t *d_out, hipStream_t s);
// one stable pass of the LSD sort: 64-bit keys, ids as payload (the library's radix sort); d_tmp == nullptr asks for *tmp_bytes
hipError_t sort_pass(void *d_tmp, size_t *tmp_bytes, const uint64_t *d_keys_in, uint64_t *d_keys_out, const uint32_t *d_ids_in, uint32_t *d_ids_out, size_t n,
                     hipStream_t s);
// the sums of every tile of the sorted order, then their exclusive 64-bit scan in place: d_base[0 .. n_tiles(n)], the last one the totals
hipError_t launch_scan(const uint32_t *d_order, const uint32_t *d_meta, size_t n, TileBase *d_base, hipStream_t s);
// the rows and (with_lists) the list lines to their offsets.  d_table holds d_base[n_tiles].at[0] bytes, d_list[l] .at[l + 1]
hipError_t launch_write(const uint8_t *d_text16, const uint64_t *d_counts, const uint32_t *d_order, const uint32_t *d_meta, size_t n, const TileBase *d_base,
                        uint8_t *d_table, uint8_t *d_list0, uint8_t *d_list1, uint8_t *d_list2, int with_lists, hipStream_t s);

}  // namespace rows
}  // namespace hast
