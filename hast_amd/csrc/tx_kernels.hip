// tx_kernels.hip -- gfx950 device code: two buffers of raw four-line FASTQ in HBM (stLFR read 1 and read 2) become two runs of 10x
// records (stage 02's fake_10x.pl; hast_tx_pair_device).  The rules are tx_core.h's, what is decided per record tx_plan.h's; the
// steps, all on one stream, shaped as sq_kernels.hip's:
//   k_nl_count      newlines per 4-KB tile of both inputs (nl_kernels.hip)
//   k_tx_scan       exclusive scan of both sides' tile counts; lines[], the pairs m of the step
//   k_nl_index      offsets of all newlines of both sides, in order (nl_kernels.hip)
//   k_tx_keys       a lane per pair: the key of the read-1 header, its slot in the map's table (kNoSlot: dropped); kept pairs per tile
//   k_tx_scan_kept  exclusive scan of the kept pairs per tile; used
//   k_tx_sizes      a lane per pair: its rank among the kept, N, the plan; both records' lengths summed per tile
//   k_tx_scan_out   exclusive scan of both sides' tile sizes; out_bytes[], and the verdict: does every run fit its room?
//   k_tx_copy       every wave emits its 64 pairs one after the other, 64 bytes a step, both sides, through rec1_byte / rec2_byte
// A step whose outputs do not fit is not copied at all: k_tx_copy reads the verdict on the device.
// The inputs may start at any address (nl_index.h); nothing outside [d_in, d_in + n_in) is read, nothing outside
// [d_out, d_out + out_bytes) written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nl_index.h"
#include "tx_device.h"

namespace hast {

__global__ void __launch_bounds__(1024) k_tx_scan(uint32_t *tile_cnt0, uint32_t *tile_cnt1, uint32_t n, TxDevState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_nl0 = block_exclusive_scan_1024(tile_cnt0, n, s_part);
    __syncthreads();                                             // (every thread has read the first total)
    const uint32_t n_nl1 = block_exclusive_scan_1024(tile_cnt1, n, s_part);
    if (threadIdx.x == 0) {
        st->consumed[0] = st->consumed[1] = st->used = st->out_bytes[0] = st->out_bytes[1] = 0;
        st->pairs = tx::pairs_of(n_nl0, n_nl1);
        st->lines[0] = n_nl0;
        st->lines[1] = n_nl1;
        st->refused = st->pad = 0;
    }
}

__global__ void __launch_bounds__(kTxTile) k_tx_keys(const uint8_t *r1, TxDevState *st, const uint32_t *nl1, const uint32_t *nl2, const tx::TableSlot *table,
                                                     uint32_t n_slots, uint32_t *slot, uint32_t *tile_kept) {
    __shared__ uint32_t s[4];
    const uint32_t m = (uint32_t)st->pairs, n_tiles = (m + kTxTile - 1) / kTxTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * kTxTile + threadIdx.x;
        uint32_t found = tx::kNoSlot;
        if (i < m) {
            uint64_t lo, hi;
            uint32_t key[4];
            tx::header_of(nl1, i, &lo, &hi);
            if (tx::key_record(r1, lo, hi, key)) found = tx::table_find(table, n_slots, key);
            slot[i] = found;
            if (i == m - 1) {
                st->consumed[0] = tx::consumed_of(nl1, m);
                st->consumed[1] = tx::consumed_of(nl2, m);
            }
        }
        __syncthreads();                                         // (s of the tile before has been read)
        const uint32_t kept = block_sum_256(found != tx::kNoSlot ? 1u : 0u, s);
        if (threadIdx.x == 0) tile_kept[tile] = kept;
    }
}

__global__ void __launch_bounds__(1024) k_tx_scan_kept(uint32_t *tile_kept, TxDevState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t m = (uint32_t)st->pairs;
    const uint32_t total = block_exclusive_scan_1024(tile_kept, (m + kTxTile - 1) / kTxTile, s_part);
    if (threadIdx.x == 0) st->used = total;
}

// what a lane knows of pair i once the kept pairs are scanned
struct TxPair {
    uint32_t slot;             // kNoSlot: dropped, or behind the last pair
    uint32_t v;                // bytes of its value
    uint64_t n;                // its N
    tx::Plan plan;
};
// every thread of the workgroup calls it (one barrier inside, on s_wave)
__device__ __forceinline__ TxPair tx_pair_of(uint32_t tile, uint32_t m, const uint32_t *nl1, const uint32_t *nl2, const uint32_t *slot, const uint32_t *tile_rank,
                                             const tx::TableSlot *table, uint64_t used, uint32_t *s_wave) {
    const uint32_t i = tile * kTxTile + threadIdx.x;
    TxPair p;
    p.slot = i < m ? slot[i] : tx::kNoSlot;
    const bool kept = p.slot != tx::kNoSlot;
    const uint32_t rank = tile_rank[tile] + block_exclusive_sum_256(kept ? 1u : 0u, s_wave);
    p.n = used + 1 + rank;
    p.v = kept ? table[p.slot].v : 0;
    if (kept) p.plan = tx::plan_pair(nl1, nl2, i, true, p.n, p.v);
    else p.plan = tx::Plan{};
    return p;
}

__global__ void __launch_bounds__(kTxTile) k_tx_sizes(const TxDevState *st, const uint32_t *nl1, const uint32_t *nl2, const uint32_t *slot, const uint32_t *tile_rank,
                                                      const tx::TableSlot *table, uint64_t used, uint32_t *tile_out0, uint32_t *tile_out1) {
    __shared__ uint32_t s_rank[4], s0[4], s1[4];
    const uint32_t m = (uint32_t)st->pairs, n_tiles = (m + kTxTile - 1) / kTxTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();                                         // (the LDS words of the tile before have been read)
        const TxPair p = tx_pair_of(tile, m, nl1, nl2, slot, tile_rank, table, used, s_rank);
        const uint32_t sum0 = block_sum_256(p.plan.rec1_len, s0), sum1 = block_sum_256(p.plan.rec2_len, s1);
        if (threadIdx.x == 0) {
            tile_out0[tile] = sum0;
            tile_out1[tile] = sum1;
        }
    }
}

__global__ void __launch_bounds__(1024) k_tx_scan_out(uint32_t *tile_out0, uint32_t *tile_out1, TxDevState *st, uint64_t cap0, uint64_t cap1) {
    __shared__ uint32_t s_part[1024];
    const uint32_t m = (uint32_t)st->pairs, n_tiles = (m + kTxTile - 1) / kTxTile;
    const uint32_t total0 = block_exclusive_scan_1024(tile_out0, n_tiles, s_part);
    __syncthreads();
    const uint32_t total1 = block_exclusive_scan_1024(tile_out1, n_tiles, s_part);
    if (threadIdx.x == 0) {
        st->out_bytes[0] = total0;
        st->out_bytes[1] = total1;
        st->refused = total0 > cap0 || total1 > cap1 ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(kTxTile) k_tx_copy(const uint8_t *r1, const uint8_t *r2, const TxDevState *st, const uint32_t *nl1, const uint32_t *nl2,
                                                     const uint32_t *slot, const uint32_t *tile_rank, const tx::TableSlot *table, uint64_t used,
                                                     const uint32_t *tile_base0, const uint32_t *tile_base1, uint8_t *out1, uint8_t *out2) {
    __shared__ tx::Plan s_plan[kTxTile];
    __shared__ uint32_t s_slot[kTxTile], s_rank_of[kTxTile], s_dst1[kTxTile], s_dst2[kTxTile];
    __shared__ uint32_t s_rank[4], s0[4], s1[4];
    if (st->refused) return;
    const uint32_t m = (uint32_t)st->pairs, n_tiles = (m + kTxTile - 1) / kTxTile;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const TxPair p = tx_pair_of(tile, m, nl1, nl2, slot, tile_rank, table, used, s_rank);
        s_plan[threadIdx.x] = p.plan;
        s_slot[threadIdx.x] = p.slot;
        s_rank_of[threadIdx.x] = (uint32_t)(p.n - used - 1);
        s_dst1[threadIdx.x] = tile_base0[tile] + block_exclusive_sum_256(p.plan.rec1_len, s0);
        s_dst2[threadIdx.x] = tile_base1[tile] + block_exclusive_sum_256(p.plan.rec2_len, s1);
        __syncthreads();
        for (uint32_t r = 0; r < 64; ++r) {
            const uint32_t j = wave * 64 + r;
            const uint32_t at = s_slot[j];
            if (at == tx::kNoSlot) continue;                     // dropped, or behind the last pair: nothing is written
            const tx::Plan pl = s_plan[j];
            const uint64_t n = used + 1 + s_rank_of[j];
            const uint8_t *value = table[at].value;
            const uint32_t v = table[at].v;
            uint8_t *d1 = out1 + s_dst1[j], *d2 = out2 + s_dst2[j];
            for (uint32_t b = lane; b < pl.rec1_len; b += 64) d1[b] = tx::rec1_byte(pl, r1, n, value, v, b);
            for (uint32_t b = lane; b < pl.rec2_len; b += 64) d2[b] = tx::rec2_byte(pl, r2, n, b);
        }
        __syncthreads();                                         // (the tile's LDS has been read before the next one writes it)
    }
}

hipError_t launch_tx_step(const TxStepArgs &a, uint8_t *d_scratch, const TxScratchPlan &p, hipStream_t s) {
    auto words = [&](size_t at) { return reinterpret_cast<uint32_t *>(d_scratch + at); };
    uint32_t *cnt0 = words(p.tile_cnt[0]), *cnt1 = words(p.tile_cnt[1]), *nl0 = words(p.nl[0]), *nl1 = words(p.nl[1]);
    uint32_t *slot = words(p.slot), *tile_kept = words(p.tile_kept), *out0 = words(p.tile_out[0]), *out1 = words(p.tile_out[1]);
    TxDevState *st = reinterpret_cast<TxDevState *>(d_scratch + p.state);
    const NlSides in{{nl_range(a.d_in[0], a.n_in[0]), nl_range(a.d_in[1], a.n_in[1])}, {cnt0, cnt1}, {nl0, nl1}};
    const uint32_t n_tiles = in.r[0].grid() > in.r[1].grid() ? in.r[0].grid() : in.r[1].grid();
    const size_t least = a.n_in[0] < a.n_in[1] ? a.n_in[0] : a.n_in[1];
    const uint32_t grid = capped_grid(least / 4, kTxTile);
    launch_nl_count(in, 2, n_tiles, s);
    hipLaunchKernelGGL(k_tx_scan, dim3(1), dim3(1024), 0, s, cnt0, cnt1, n_tiles, st);
    launch_nl_index(in, 2, n_tiles, s);
    hipLaunchKernelGGL(k_tx_keys, dim3(grid), dim3(kTxTile), 0, s, a.d_in[0], st, nl0, nl1, a.d_table, a.n_slots, slot, tile_kept);
    hipLaunchKernelGGL(k_tx_scan_kept, dim3(1), dim3(1024), 0, s, tile_kept, st);
    hipLaunchKernelGGL(k_tx_sizes, dim3(grid), dim3(kTxTile), 0, s, st, nl0, nl1, slot, tile_kept, a.d_table, a.used, out0, out1);
    hipLaunchKernelGGL(k_tx_scan_out, dim3(1), dim3(1024), 0, s, out0, out1, st, (uint64_t)a.cap[0], (uint64_t)a.cap[1]);
    hipLaunchKernelGGL(k_tx_copy, dim3(grid), dim3(kTxTile), 0, s, a.d_in[0], a.d_in[1], st, nl0, nl1, slot, tile_kept, a.d_table, a.used, out0, out1,
                       a.d_out[0], a.d_out[1]);
    return hipGetLastError();
}

}  // namespace hast
