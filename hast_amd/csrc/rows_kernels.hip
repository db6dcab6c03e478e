// rows_kernels.hip -- the output table of `classify --rows device` made in HBM (include/hast.h "the output table on the GPU"): a key,
// a call and the lengths per barcode id (k_rows_key), the ids ordered by key (two stable passes of the library's radix sort over the
// key's low and high word, rows_sort.hip, k_rows_gather between them), the offsets of every row and list line (k_rows_tile_sums, k_rows_scan) and
// the text itself (k_rows_write).  Every rule is rows_core.h's; rows_host.h is the same steps on the host.  gfx950, wave64, workgroups
// of 256; no kernel may use scratch memory (the Makefile's rule reads the compiler's resource report).
//
// THE OFFSETS.  A row's place in the table is the sum of the lengths of the rows in front of it in sorted order; a list line's place is
// the sum of the line lengths of the rows in front of it that are on the same list -- the three lists are a stable partition of the
// sorted order.  Four sums, then: a tile of kTile rows sums them (k_rows_tile_sums; a tile's sums fit 16 bits each, two share a word),
// one workgroup scans the tiles' sums 256 at a time with a 64-bit carry from one 256 to the next (k_rows_scan: any number of tiles),
// and k_rows_write scans inside its tile again, in registers, instead of reading 16 bytes of offsets per row that a kernel would have
// had to write first.  Offsets are 64-bit from the tile's base on: nothing assumes that a table stays under 4 GB.
//
// THE STORES.  A lane that wrote its 18..61-byte row to where it belongs would store bytes that 64 lanes scatter over 1..4 KB.  The
// rows of a tile are consecutive in the table, so the tile's text is ONE run of bytes: the lanes put their rows together in LDS
// (byte stores, at the in-tile offsets) and the workgroup stores the run as aligned dwords, lane after lane -- 256 B per wave and
// store.  The lists' lines of a tile are three such runs.  (Splitting by output bytes as span_copy.h does needs the offsets of all
// rows in memory and a binary search per lane; here the producer of the bytes is arithmetic, not a copy, and a lane would have to
// format a row again for every 16-byte piece of it.)
#include <hip/hip_runtime.h>

#include "rows_core.h"
#include "rows_device.h"
#include "scan_device.h"

namespace hast {
namespace rows {
namespace {

constexpr uint32_t kRecWords = 5;      // a record in LDS: 16 bytes at a stride of 20, so that the lanes' byte reads spread over the banks
constexpr uint32_t kGridCap = 2048;    // workgroups of a grid at most; the loops go on from there

// The lane's record into words of LDS that only this lane reads: the rules of rows_core.h index the record byte by byte, which in
// registers would be an array indexed at run time (scratch memory).  One 16-byte load, as the records lie.
__device__ __forceinline__ const uint8_t *stage_rec(uint32_t *slot, const uint8_t *d_rec) {
    const uint4 v = *reinterpret_cast<const uint4 *>(d_rec);
    slot[0] = v.x;
    slot[1] = v.y;
    slot[2] = v.z;
    slot[3] = v.w;
    return reinterpret_cast<const uint8_t *>(slot);
}

// the four lengths a row adds to the sums of its tile, two to a word: a = row | line on list 1, b = line on list 2 | line on list 3
__device__ __forceinline__ void pack_lengths(uint32_t meta, uint32_t *a, uint32_t *b) {
    const uint32_t list = meta_list(meta), line = meta_line_len(meta);
    *a = meta_row_len(meta) | (list == 1 ? line << 16 : 0u);
    *b = (list == 2 ? line : 0u) | (list == 3 ? line << 16 : 0u);
}

__global__ __launch_bounds__(256) void k_rows_key(const uint8_t *__restrict__ text16, const uint64_t *__restrict__ counts, size_t n, uint64_t n0, uint64_t n1,
                                                  double w0, double w1, uint64_t *__restrict__ hi, uint64_t *__restrict__ lo, uint32_t *__restrict__ id,
                                                  uint32_t *__restrict__ meta, uint8_t *__restrict__ list_of, uint32_t *flags) {
    __shared__ uint32_t s_rec[256 * kRecWords];
    uint32_t sep = 0, past = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint8_t *rec = stage_rec(s_rec + threadIdx.x * kRecWords, text16 + 16 * i);
        const ulonglong2 c = *reinterpret_cast<const ulonglong2 *>(counts + 4 * i);
        const Key k = row_key(rec);
        const int hap = row_hap(rec, c.x, c.y, n0, n1, w0, w1);
        const uint32_t list = row_list(hap);
        hi[i] = k.hi;
        lo[i] = k.lo;
        id[i] = (uint32_t)i;
        meta[i] = meta_pack(row_len(rec, hap, c.x, c.y), line_len(rec), list);
        list_of[i] = (uint8_t)list;
        sep |= has_sep(rec) ? 1u : 0u;
        past |= past_int(c.x, c.y) ? 1u : 0u;
    }
    const bool any_sep = __ballot(sep != 0) != 0, any_past = __ballot(past != 0) != 0;
    if ((threadIdx.x & 63) == 0) {
        if (any_sep) atomicOr(&flags[0], 1u);
        if (any_past) atomicOr(&flags[1], 1u);
    }
}

__global__ __launch_bounds__(256) void k_rows_gather(const uint64_t *__restrict__ by_id, const uint32_t *__restrict__ ids, size_t n, uint64_t *__restrict__ out) {
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (size_t)gridDim.x * 256) out[r] = by_id[ids[r]];
}

__global__ __launch_bounds__(256) void k_rows_tile_sums(const uint32_t *__restrict__ order, const uint32_t *__restrict__ meta, size_t n, TileBase *__restrict__ base) {
    __shared__ uint32_t s_sum[8];
    const size_t nt = (n + kTile - 1) / kTile;
    for (size_t t = blockIdx.x; t < nt; t += gridDim.x) {
        uint32_t a = 0, b = 0;
        for (uint32_t j = 0; j < 2; ++j) {
            const size_t r = t * kTile + 2 * threadIdx.x + j;
            if (r < n) {
                uint32_t ra, rb;
                pack_lengths(meta[order[r]], &ra, &rb);
                a += ra;
                b += rb;
            }
        }
        a = block_sum_256(a, s_sum);
        b = block_sum_256(b, s_sum + 4);
        if (threadIdx.x == 0) base[t] = TileBase{{a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16}};
        __syncthreads();
    }
}

// one workgroup: base[t] = the sums of the tiles in front of t, base[nt] = the totals
__global__ __launch_bounds__(256) void k_rows_scan(TileBase *base, size_t nt) {
    __shared__ uint32_t s_ex[16], s_tot[16];
    uint64_t carry0 = 0, carry1 = 0, carry2 = 0, carry3 = 0;
    for (size_t t0 = 0; t0 < nt; t0 += 256) {
        const size_t t = t0 + threadIdx.x;
        TileBase v = TileBase{{0, 0, 0, 0}};
        if (t < nt) v = base[t];
        // (a tile's sums are below 2^16 and 256 of them below 2^24: 32-bit scans inside the 256, the carry in 64)
        const uint32_t v0 = (uint32_t)v.at[0], v1 = (uint32_t)v.at[1], v2 = (uint32_t)v.at[2], v3 = (uint32_t)v.at[3];
        const uint32_t e0 = block_exclusive_sum_256(v0, s_ex), e1 = block_exclusive_sum_256(v1, s_ex + 4);
        const uint32_t e2 = block_exclusive_sum_256(v2, s_ex + 8), e3 = block_exclusive_sum_256(v3, s_ex + 12);
        const uint32_t t0s = block_sum_256(v0, s_tot), t1s = block_sum_256(v1, s_tot + 4), t2s = block_sum_256(v2, s_tot + 8), t3s = block_sum_256(v3, s_tot + 12);
        if (t < nt) base[t] = TileBase{{carry0 + e0, carry1 + e1, carry2 + e2, carry3 + e3}};
        carry0 += t0s;
        carry1 += t1s;
        carry2 += t2s;
        carry3 += t3s;
        __syncthreads();
    }
    if (threadIdx.x == 0) base[nt] = TileBase{{carry0, carry1, carry2, carry3}};
}

// n bytes of LDS to out + g0, by the whole workgroup: bytes up to the first 4-byte boundary of the destination, dwords, bytes
__device__ __forceinline__ void tile_store(uint8_t *out, uint64_t g0, const uint8_t *s, uint32_t n) {
    uint8_t *dst = out + g0;
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    if (head > n) head = n;
    if (threadIdx.x < head) dst[threadIdx.x] = s[threadIdx.x];
    const uint32_t nw = (n - head) >> 2;
    for (uint32_t w = threadIdx.x; w < nw; w += 256) {
        const uint32_t k = head + 4 * w;
        *reinterpret_cast<uint32_t *>(dst + k) = (uint32_t)s[k] | (uint32_t)s[k + 1] << 8 | (uint32_t)s[k + 2] << 16 | (uint32_t)s[k + 3] << 24;
    }
    const uint32_t tail = head + 4 * nw;
    if (threadIdx.x < n - tail) dst[tail + threadIdx.x] = s[tail + threadIdx.x];
}

__global__ __launch_bounds__(256) void k_rows_write(const uint8_t *__restrict__ text16, const uint64_t *__restrict__ counts, const uint32_t *__restrict__ order,
                                                    const uint32_t *__restrict__ meta, size_t n, const TileBase *__restrict__ base, uint8_t *table, uint8_t *list0,
                                                    uint8_t *list1, uint8_t *list2, int with_lists) {
    __shared__ uint32_t s_rec[256 * kRecWords];
    __shared__ uint32_t s_table_w[kTile * kMaxRow / 4];
    __shared__ uint32_t s_list_w[kTile * kMaxLine / 4];
    __shared__ uint32_t s_scan[8];
    uint8_t *s_table = reinterpret_cast<uint8_t *>(s_table_w), *s_list = reinterpret_cast<uint8_t *>(s_list_w);
    const size_t nt = (n + kTile - 1) / kTile;
    for (size_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const TileBase b0 = base[t], b1 = base[t + 1];
        const uint32_t n_table = (uint32_t)(b1.at[0] - b0.at[0]);
        const uint32_t n_l0 = (uint32_t)(b1.at[1] - b0.at[1]), n_l1 = (uint32_t)(b1.at[2] - b0.at[2]), n_l2 = (uint32_t)(b1.at[3] - b0.at[3]);
        uint32_t row_id[2] = {0, 0}, row_meta[2] = {0, 0}, a[2] = {0, 0}, b[2] = {0, 0};
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j) {
            const size_t r = t * kTile + 2 * threadIdx.x + j;
            if (r < n) {
                row_id[j] = order[r];
                row_meta[j] = meta[row_id[j]];
                pack_lengths(row_meta[j], &a[j], &b[j]);
            }
        }
        const uint32_t ea = block_exclusive_sum_256(a[0] + a[1], s_scan), eb = block_exclusive_sum_256(b[0] + b[1], s_scan + 4);
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j) {
            const size_t r = t * kTile + 2 * threadIdx.x + j;
            if (r >= n) continue;
            const uint32_t fa = ea + (j ? a[0] : 0u), fb = eb + (j ? b[0] : 0u);        // the lengths in front of this row in its tile
            const uint32_t list = meta_list(row_meta[j]);
            const uint8_t *rec = stage_rec(s_rec + threadIdx.x * kRecWords, text16 + 16 * (size_t)row_id[j]);
            const ulonglong2 c = *reinterpret_cast<const ulonglong2 *>(counts + 4 * (size_t)row_id[j]);
            put_row(s_table + (fa & 0xFFFF), rec, list == 1 ? 0 : list == 2 ? 1 : -1, c.x, c.y);
            if (with_lists) {
                const uint32_t at = list == 1 ? fa >> 16 : list == 2 ? n_l0 + (fb & 0xFFFF) : n_l0 + n_l1 + (fb >> 16);
                put_line(s_list + at, rec);
            }
        }
        __syncthreads();
        tile_store(table, b0.at[0], s_table, n_table);
        if (with_lists) {
            tile_store(list0, b0.at[1], s_list, n_l0);
            tile_store(list1, b0.at[2], s_list + n_l0, n_l1);
            tile_store(list2, b0.at[3], s_list + n_l0 + n_l1, n_l2);
        }
        __syncthreads();
    }
}

inline uint32_t grid_for(size_t items) { return (uint32_t)(items < kGridCap ? (items ? items : 1) : kGridCap); }

}  // namespace

hipError_t launch_key(const uint8_t *d_text16, const uint64_t *d_counts, size_t n, uint64_t n0, uint64_t n1, double w0, double w1, uint64_t *d_hi, uint64_t *d_lo,
                      uint32_t *d_id, uint32_t *d_meta, uint8_t *d_list, uint32_t *d_flags, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rows_key, dim3(grid_for((n + 255) / 256)), dim3(256), 0, s, d_text16, d_counts, n, n0, n1, w0, w1, d_hi, d_lo, d_id, d_meta, d_list, d_flags);
    return hipGetLastError();
}

hipError_t launch_gather(const uint64_t *d_by_id, const uint32_t *d_ids, size_t n, uint64_t *d_out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rows_gather, dim3(grid_for((n + 255) / 256)), dim3(256), 0, s, d_by_id, d_ids, n, d_out);
    return hipGetLastError();
}

hipError_t launch_scan(const uint32_t *d_order, const uint32_t *d_meta, size_t n, TileBase *d_base, hipStream_t s) {
    const size_t nt = n_tiles(n);
    if (nt) hipLaunchKernelGGL(k_rows_tile_sums, dim3(grid_for(nt)), dim3(256), 0, s, d_order, d_meta, n, d_base);
    hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(256), 0, s, d_base, nt);
    return hipGetLastError();
}

hipError_t launch_write(const uint8_t *d_text16, const uint64_t *d_counts, const uint32_t *d_order, const uint32_t *d_meta, size_t n, const TileBase *d_base,
                        uint8_t *d_table, uint8_t *d_list0, uint8_t *d_list1, uint8_t *d_list2, int with_lists, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rows_write, dim3(grid_for(n_tiles(n))), dim3(256), 0, s, d_text16, d_counts, d_order, d_meta, n, d_base, d_table, d_list0, d_list1, d_list2,
                       with_lists);
    return hipGetLastError();
}

}  // namespace rows
}  // namespace hast
