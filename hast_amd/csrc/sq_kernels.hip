// sq_kernels.hip -- gfx950 device code: a block of raw four-line FASTQ in HBM becomes the base stream hast_kc_count_device eats
// (stage 00 ingest on the device).  The rules are sq_core.h's; the steps, all on one stream:
//   k_sq_count      newlines per 4-KB tile of the block (16 bytes per lane)
//   k_sq_scan       exclusive scan of the tile counts; the block's newline and record counts
//   k_sq_index      offsets of all newlines, in order
//   k_sq_records    a lane per record: the four extents, the rules, the record's output length and where its sequence lies
//   k_sq_scan_out   exclusive scan of the output lengths per tile of 256 records; the block's verdict
//   k_sq_copy       every wave copies its 64 records one after the other, 64 bytes a step, and ends each with '\n'
// A block that breaks a rule is not copied at all: k_sq_copy reads the verdict on the device.
// The block may start at any address: the tiles are cut at 16-byte boundaries of the ADDRESS, and the 16-byte pieces that reach
// outside the block are read byte by byte, so nothing outside [d_in, d_in + n_in) is touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nl_index.h"
#include "sq_device.h"

namespace hast {

// The newline index is nl_index.h's, shared with the framer of `classify` (fq_kernels.hip); here its offsets count from the block's
// first byte, base + lo.
__global__ void __launch_bounds__(256) k_sq_count(const uint8_t *base, uint64_t lo, uint64_t hi, uint32_t *tile_cnt) {
    const uint32_t c = nl_tile_count(base, blockIdx.x, lo, hi);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = c;
}

__global__ void __launch_bounds__(1024) k_sq_scan(uint32_t *tile_cnt, uint32_t n, SqState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_nl = block_exclusive_scan_1024(tile_cnt, n, s_part);
    if (threadIdx.x == 0) {
        st->consumed = st->out_bytes = st->records = st->bases = 0;
        st->n_nl = n_nl;
        st->n_rec = n_nl / 4;
        st->flags = n_nl < 4 ? SQ_NO_RECORD : 0u;
        st->first_bad = sq::kNoBad;
    }
}

// nl[j] = offset of the j-th newline from the block's first byte (base + lo)
__global__ void __launch_bounds__(256) k_sq_index(const uint8_t *base, uint64_t lo, uint64_t hi, const uint32_t *tile_base, uint32_t *nl) {
    nl_tile_index(base, blockIdx.x, lo, hi, lo, tile_base, nl);
}

__global__ void __launch_bounds__(kSqRecTile) k_sq_records(const uint8_t *in, SqState *st, const uint32_t *nl, uint32_t *r_src, uint32_t *r_len, uint32_t *tile_sum) {
    __shared__ uint32_t s[4];
    const uint32_t n_rec = st->n_rec, n_tiles = (n_rec + kSqRecTile - 1) / kSqRecTile;
    unsigned long long bases = 0;                                // lane 0 of the workgroup: over all its tiles
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * kSqRecTile + threadIdx.x;
        uint32_t len = 0;
        if (i < n_rec) {
            uint32_t seq_at, ls;
            if (!sq::record_at(in, nl, i, &seq_at, &ls)) atomicMin(&st->first_bad, i);
            r_src[i] = seq_at;
            r_len[i] = len = ls + 1;
            if (i == n_rec - 1) st->consumed = (uint64_t)nl[4 * (uint64_t)i + 3] + 1;
        }
        __syncthreads();                                         // (s of the tile before has been read)
        const uint32_t sum = block_sum_256(len, s);
        if (threadIdx.x == 0) {
            const uint32_t in_tile = n_rec - tile * kSqRecTile < kSqRecTile ? n_rec - tile * kSqRecTile : kSqRecTile;
            tile_sum[tile] = sum;
            bases += sum - in_tile;
        }
    }
    if (threadIdx.x == 0 && bases) atomicAdd(reinterpret_cast<unsigned long long *>(&st->bases), bases);
}

__global__ void __launch_bounds__(1024) k_sq_scan_out(uint32_t *tile_sum, SqState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_rec = st->n_rec;
    const uint32_t total = block_exclusive_scan_1024(tile_sum, (n_rec + kSqRecTile - 1) / kSqRecTile, s_part);
    if (threadIdx.x == 0) {
        if (st->first_bad != sq::kNoBad) {                       // refused as a whole
            st->flags |= SQ_NOT_FOUR_LINE;
            st->consumed = st->bases = 0;
        } else {
            st->out_bytes = total;
            st->records = n_rec;
        }
    }
}

__global__ void __launch_bounds__(kSqRecTile) k_sq_copy(const uint8_t *in, const SqState *st, const uint32_t *r_src, const uint32_t *r_len, const uint32_t *tile_base,
                                                        uint8_t *out) {
    __shared__ uint32_t s_src[kSqRecTile], s_dst[kSqRecTile], s_n[kSqRecTile];
    __shared__ uint32_t s_wave[4];
    if (st->flags) return;
    const uint32_t n_rec = st->n_rec, n_tiles = (n_rec + kSqRecTile - 1) / kSqRecTile;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * kSqRecTile + threadIdx.x;
        const uint32_t len = i < n_rec ? r_len[i] : 0;
        s_src[threadIdx.x] = i < n_rec ? r_src[i] : 0;
        s_dst[threadIdx.x] = tile_base[tile] + block_exclusive_sum_256(len, s_wave);
        s_n[threadIdx.x] = len;
        __syncthreads();
        for (uint32_t r = 0; r < 64; ++r) {
            const uint32_t j = wave * 64 + r;
            const uint32_t n = s_n[j];                           // sequence + '\n'; 0 behind the last record
            if (n == 0) break;
            const uint8_t *src = in + s_src[j];
            uint8_t *d = out + s_dst[j];
            for (uint32_t b = lane; b + 1 < n; b += 64) d[b] = src[b];
            if (lane == ((n - 1) & 63)) d[n - 1] = '\n';
        }
        __syncthreads();
    }
}

hipError_t launch_sq_frame(const uint8_t *d_in, size_t n_in, uint8_t *d_out, uint8_t *d_scratch, const SqScratchPlan &p, hipStream_t s) {
    const uint64_t lo = reinterpret_cast<uintptr_t>(d_in) & 15, hi = lo + n_in;
    const uint8_t *base = d_in - lo;
    const uint32_t n_tiles = (uint32_t)((hi + kNlTile - 1) / kNlTile), grid = n_tiles ? n_tiles : 1;
    uint32_t *tile_cnt = reinterpret_cast<uint32_t *>(d_scratch + p.tile_cnt), *nl = reinterpret_cast<uint32_t *>(d_scratch + p.nl);
    uint32_t *r_src = reinterpret_cast<uint32_t *>(d_scratch + p.r_src), *r_len = reinterpret_cast<uint32_t *>(d_scratch + p.r_len);
    uint32_t *r_tile = reinterpret_cast<uint32_t *>(d_scratch + p.r_tile);
    SqState *st = reinterpret_cast<SqState *>(d_scratch + p.state);
    const uint32_t rec_grid = capped_grid(n_in / 4, kSqRecTile);
    hipLaunchKernelGGL(k_sq_count, dim3(grid), dim3(256), 0, s, base, lo, hi, tile_cnt);
    hipLaunchKernelGGL(k_sq_scan, dim3(1), dim3(1024), 0, s, tile_cnt, grid, st);
    hipLaunchKernelGGL(k_sq_index, dim3(grid), dim3(256), 0, s, base, lo, hi, tile_cnt, nl);
    hipLaunchKernelGGL(k_sq_records, dim3(rec_grid), dim3(kSqRecTile), 0, s, d_in, st, nl, r_src, r_len, r_tile);
    hipLaunchKernelGGL(k_sq_scan_out, dim3(1), dim3(1024), 0, s, r_tile, st);
    hipLaunchKernelGGL(k_sq_copy, dim3(rec_grid), dim3(kSqRecTile), 0, s, d_in, st, r_src, r_len, r_tile, d_out);
    return hipGetLastError();
}

}  // namespace hast
