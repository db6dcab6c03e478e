// rr_kernels.hip -- gfx950 device code: the rows of stage 03's reads made where their names and votes lie (`classify_read --rows device`).
// The rule is rr_core.h's; the input is what k_rs_names and the per-read classifier leave in HBM.  The steps, all on one stream:
//   k_rr_sums    a lane per read: class and q, the length of its row; per tile of 256 reads the bytes of its rows (64 bits: the sizes
//                of a view's rows may pass 2^32 before anybody knows that they do not fit) and its reads per class
//   k_rr_scan    exclusive scan of the tile sums (a workgroup of 1024, every thread a run of tiles: any number of tiles), the total, the
//                counts, and the word on whether the rows fit
//   k_rr_write   a lane per read: its row starts at the tile's offset plus the lengths in front of it; the names go in a wave per read,
//                64 bytes a step (record_gather.h: a name is a few bytes or a FASTA header line of kilobytes, and no lane walks one
//                alone), then every lane stores the at most 31 bytes behind its name.  Nothing is written when the rows do not fit.
// No kernel here may use scratch memory (Makefile): put_tail stores its bytes as it makes them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "record_gather.h"
#include "rr_core.h"
#include "rs_device.h"
#include "scan_device.h"

namespace hast {

struct RrRow {
    uint32_t cls, name_len, len;
    uint64_t q;
};
__device__ __forceinline__ RrRow rr_row(const uint32_t *name_off, const uint32_t *votes, uint32_t t0, uint32_t t1, uint32_t r) {
    RrRow x;
    rr::row_of(votes[2 * (size_t)r], votes[2 * (size_t)r + 1], t0, t1, &x.cls, &x.q);
    x.name_len = name_off[r + 1] - name_off[r];
    x.len = x.name_len + rr::tail_bytes(x.cls, x.q);        // (below 2^32: the names of a view are)
    return x;
}

__global__ void __launch_bounds__(kRsTile) k_rr_sums(const uint32_t *name_off, const uint32_t *votes, uint32_t n_rec, uint32_t t0, uint32_t t1,
                                                     uint64_t *tile_bytes, uint32_t *tile_cnt) {
    __shared__ uint32_t s_b[4], s_c[rb::kClasses][4];
    const uint32_t n_tiles = (n_rec + kRsTile - 1) / kRsTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r = tile * kRsTile + threadIdx.x;
        uint32_t cls = rb::kClasses, len = 0;
        if (r < n_rec) {
            const RrRow x = rr_row(name_off, votes, t0, t1, r);
            cls = x.cls;
            len = x.len;
        }
        __syncthreads();                                         // (the sums of the tile before have been read)
        // a tile's names are a piece of one buffer of under 2^32 bytes and its tails 256 x 31 at most, but their sum may wrap: two halves
        const uint32_t lo = block_sum_256(len & 0xffffu, s_b);
        __syncthreads();
        const uint32_t hi = block_sum_256(len >> 16, s_b);
        if (threadIdx.x == 0) tile_bytes[tile] = ((uint64_t)hi << 16) + lo;
        for (uint32_t c = 0; c < rb::kClasses; ++c) {
            const uint32_t sum_c = block_sum_256(cls == c, s_c[c]);
            if (threadIdx.x == 0) tile_cnt[c * n_tiles + tile] = sum_c;
        }
    }
}

// Workgroup of 1024: exclusive scan of v[0, n) in place, every thread a run of the values; returns the total, to every thread.
// s_part: 1024 words of LDS.  (scan_device.h's block_exclusive_scan_1024, on 64-bit values)
__device__ __forceinline__ uint64_t rr_exclusive_scan_1024(uint64_t *v, uint32_t n, uint64_t *s_part) {
    const uint32_t per = (n + 1023) / 1024;
    const uint64_t first = (uint64_t)threadIdx.x * per;
    const uint32_t lo = first < n ? (uint32_t)first : n, hi = n - lo > per ? lo + per : n;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += v[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {                    // Hillis-Steele inclusive scan
        const uint64_t x = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0;
        __syncthreads();
        s_part[threadIdx.x] += x;
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? s_part[threadIdx.x - 1] : 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t c = v[i];
        v[i] = run;
        run += c;
    }
    return s_part[1023];
}

__global__ void __launch_bounds__(1024) k_rr_scan(uint32_t n_rec, uint64_t cap, uint64_t *tile_bytes, uint32_t *tile_cnt, RrState *st) {
    __shared__ uint64_t s_part[1024];
    const uint32_t n_tiles = (n_rec + kRsTile - 1) / kRsTile;
    const uint64_t total = rr_exclusive_scan_1024(tile_bytes, n_tiles, s_part);
    // the counts: the sums of three runs of tiles (3 n_tiles may pass 2^32 / 256 only with n_rec near 2^32, and the sums stay below n_rec)
    for (uint32_t c = 0; c < rb::kClasses; ++c) {
        __syncthreads();                                         // (s_part is written again)
        uint64_t sum = 0;
        for (uint32_t i = threadIdx.x; i < n_tiles; i += 1024) sum += tile_cnt[(size_t)c * n_tiles + i];
        s_part[threadIdx.x] = sum;
        __syncthreads();
        for (uint32_t d = 512; d; d >>= 1) {
            if (threadIdx.x < d) s_part[threadIdx.x] += s_part[threadIdx.x + d];
            __syncthreads();
        }
        if (threadIdx.x == 0) st->count[c] = s_part[0];
    }
    if (threadIdx.x == 0) {
        st->total = total;
        st->written = total <= cap && total < (1ull << 32);
        st->pad = 0;
    }
}

__global__ void __launch_bounds__(kRsTile) k_rr_write(const uint8_t *names, const uint32_t *name_off, const uint32_t *votes, uint32_t n_rec, uint32_t t0,
                                                      uint32_t t1, const uint64_t *tile_bytes, const RrState *st, uint8_t *out) {
    __shared__ uint32_t s_wave[4];
    if (!st->written) return;
    const uint32_t n_tiles = (n_rec + kRsTile - 1) / kRsTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r = tile * kRsTile + threadIdx.x;
        RrRow x;
        x.cls = rb::kClasses, x.name_len = 0, x.len = 0, x.q = 0;
        if (r < n_rec) x = rr_row(name_off, votes, t0, t1, r);
        const uint32_t dst = (uint32_t)tile_bytes[tile] + block_exclusive_sum_256(x.len, s_wave);      // (total < 2^32)
        record_gather_256<GatherBytes>(names, out, r < n_rec ? name_off[r] : 0, dst, x.name_len, n_rec - tile * kRsTile);
        if (r < n_rec) rr::put_tail(out + dst + x.name_len, x.cls, x.q);
    }
}

hipError_t launch_rr_rows(const uint8_t *d_names, const uint32_t *d_name_off, const uint32_t *d_votes, size_t n, uint32_t t0, uint32_t t1, uint8_t *d_rr,
                          const RrScratchPlan &p, uint8_t *d_out, uint64_t cap, hipStream_t s) {
    uint64_t *tile_bytes = reinterpret_cast<uint64_t *>(d_rr + p.tile_bytes);
    uint32_t *tile_cnt = reinterpret_cast<uint32_t *>(d_rr + p.tile_cnt);
    RrState *st = reinterpret_cast<RrState *>(d_rr + p.state);
    const uint32_t n_rec = (uint32_t)n, grid = capped_grid(n, kRsTile);
    hipLaunchKernelGGL(k_rr_sums, dim3(grid), dim3(kRsTile), 0, s, d_name_off, d_votes, n_rec, t0, t1, tile_bytes, tile_cnt);
    hipLaunchKernelGGL(k_rr_scan, dim3(1), dim3(1024), 0, s, n_rec, cap, tile_bytes, tile_cnt, st);
    hipLaunchKernelGGL(k_rr_write, dim3(grid), dim3(kRsTile), 0, s, d_names, d_name_off, d_votes, n_rec, t0, t1, (const uint64_t *)tile_bytes,
                       (const RrState *)st, d_out);
    return hipGetLastError();
}

}  // namespace hast
