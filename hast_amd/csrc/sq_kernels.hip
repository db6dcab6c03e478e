// sq_kernels.hip -- gfx950 device code: a block of raw four-line FASTQ in HBM becomes the base stream hast_kc_count_device eats
// (stage 00 ingest on the device).  The rules are sq_core.h's; the steps, all on one stream:
//   k_nl_count      newlines per 4-KB tile of the block (nl_kernels.hip)
//   k_sq_scan       exclusive scan of the tile counts; the block's newline and record counts
//   k_nl_index      offsets of all newlines, in order (nl_kernels.hip)
//   k_sq_records    a lane per record: the four extents, the rules, the record's output length and where its sequence lies
//   k_sq_scan_out   exclusive scan of the output lengths per tile of 256 records; the block's verdict
//   k_sq_copy       the sequences gathered back to back, each ended with '\n' (record_gather.h)
// A block that breaks a rule is not copied at all: k_sq_copy reads the verdict on the device.
// The block may start at any address (nl_index.h): nothing outside [d_in, d_in + n_in) is touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nl_index.h"
#include "record_gather.h"
#include "sq_device.h"

namespace hast {

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
    __shared__ uint32_t s_wave[4];
    if (st->flags) return;
    const uint32_t n_rec = st->n_rec, n_tiles = (n_rec + kSqRecTile - 1) / kSqRecTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * kSqRecTile + threadIdx.x;
        const uint32_t len = i < n_rec ? r_len[i] : 0;           // sequence + '\n'
        const uint32_t dst = tile_base[tile] + block_exclusive_sum_256(len, s_wave);
        record_gather_256<GatherLines>(in, out, i < n_rec ? r_src[i] : 0, dst, len, n_rec - tile * kSqRecTile);
    }
}

hipError_t launch_sq_frame(const uint8_t *d_in, size_t n_in, uint8_t *d_out, uint8_t *d_scratch, const SqScratchPlan &p, hipStream_t s) {
    uint32_t *tile_cnt = reinterpret_cast<uint32_t *>(d_scratch + p.tile_cnt), *nl = reinterpret_cast<uint32_t *>(d_scratch + p.nl);
    uint32_t *r_src = reinterpret_cast<uint32_t *>(d_scratch + p.r_src), *r_len = reinterpret_cast<uint32_t *>(d_scratch + p.r_len);
    uint32_t *r_tile = reinterpret_cast<uint32_t *>(d_scratch + p.r_tile);
    SqState *st = reinterpret_cast<SqState *>(d_scratch + p.state);
    const uint32_t rec_grid = capped_grid(n_in / 4, kSqRecTile);
    const NlSides block{{nl_range(d_in, n_in)}, {tile_cnt}, {nl}};
    const uint32_t grid = block.r[0].grid();
    launch_nl_count(block, 1, grid, s);
    hipLaunchKernelGGL(k_sq_scan, dim3(1), dim3(1024), 0, s, tile_cnt, grid, st);
    launch_nl_index(block, 1, grid, s);
    hipLaunchKernelGGL(k_sq_records, dim3(rec_grid), dim3(kSqRecTile), 0, s, d_in, st, nl, r_src, r_len, r_tile);
    hipLaunchKernelGGL(k_sq_scan_out, dim3(1), dim3(1024), 0, s, r_tile, st);
    hipLaunchKernelGGL(k_sq_copy, dim3(rec_grid), dim3(kSqRecTile), 0, s, d_in, st, r_src, r_len, r_tile, d_out);
    return hipGetLastError();
}

}  // namespace hast
