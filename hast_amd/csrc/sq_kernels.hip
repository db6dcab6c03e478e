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

#include "sq_device.h"

namespace hast {

// bit i set <=> base[at + i] == '\n', for the 16 bytes at the 16-B aligned base + at; only bytes inside [lo, hi) are read
__device__ __forceinline__ uint32_t sq_nl_mask16(const uint8_t *base, uint64_t at, uint64_t lo, uint64_t hi) {
    if (at + 16 <= lo || at >= hi) return 0;
    uint32_t m = 0;
    if (at >= lo && at + 16 <= hi) {
        const uint4 v = *reinterpret_cast<const uint4 *>(base + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t y = w[i] ^ 0x0A0A0A0Au;
            const uint32_t z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;     // 0x80 in every zero byte, exact
            m |= (((z >> 7) * 0x00204081u) >> 21 & 0xFu) << (4 * i);                          // bits 0,8,16,24 -> 4 adjacent bits
        }
        return m;
    }
    for (uint32_t i = 0; i < 16; ++i)
        if (at + i >= lo && at + i < hi && base[at + i] == '\n') m |= 1u << i;
    return m;
}

__global__ void __launch_bounds__(256) k_sq_count(const uint8_t *base, uint64_t lo, uint64_t hi, uint32_t *tile_cnt) {
    const uint64_t at = (uint64_t)blockIdx.x * kSqTile + threadIdx.x * 16;
    uint32_t c = __popc(sq_nl_mask16(base, at, lo, hi));
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    __shared__ uint32_t s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// exclusive scan of n values in place, by one workgroup of 1024; returns the total (to every lane)
__device__ __forceinline__ uint32_t sq_scan_1024(uint32_t *v, uint32_t n, uint32_t *s_part) {
    const uint32_t per = (n + 1023) / 1024, lo = threadIdx.x * per < n ? threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += v[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {                 // Hillis-Steele inclusive scan
        const uint32_t x = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0;
        __syncthreads();
        s_part[threadIdx.x] += x;
        __syncthreads();
    }
    uint32_t run = threadIdx.x ? s_part[threadIdx.x - 1] : 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = v[i];
        v[i] = run;
        run += c;
    }
    return s_part[1023];
}

__global__ void __launch_bounds__(1024) k_sq_scan(uint32_t *tile_cnt, uint32_t n, SqState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_nl = sq_scan_1024(tile_cnt, n, s_part);
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
    const uint64_t at = (uint64_t)blockIdx.x * kSqTile + threadIdx.x * 16;
    uint32_t m = sq_nl_mask16(base, at, lo, hi);
    const uint32_t c = __popc(m);
    uint32_t incl = c;
    const uint32_t lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += v;
    }
    __shared__ uint32_t s[4];
    if (lane == 63) s[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t to = tile_base[blockIdx.x] + incl - c;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) to += s[w];
    while (m) {
        const uint32_t b = __ffs(m) - 1;
        nl[to++] = (uint32_t)(at + b - lo);
        m &= m - 1;
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
        uint32_t c = len;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        __syncthreads();                                         // (s of the tile before has been read)
        if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t sum = s[0] + s[1] + s[2] + s[3], in_tile = n_rec - tile * kSqRecTile < kSqRecTile ? n_rec - tile * kSqRecTile : kSqRecTile;
            tile_sum[tile] = sum;
            bases += sum - in_tile;
        }
    }
    if (threadIdx.x == 0 && bases) atomicAdd(reinterpret_cast<unsigned long long *>(&st->bases), bases);
}

__global__ void __launch_bounds__(1024) k_sq_scan_out(uint32_t *tile_sum, SqState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_rec = st->n_rec;
    const uint32_t total = sq_scan_1024(tile_sum, (n_rec + kSqRecTile - 1) / kSqRecTile, s_part);
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
        uint32_t incl = len;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(incl, off, 64);
            if (lane >= (uint32_t)off) incl += u;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t dst = tile_base[tile] + incl - len;
        for (uint32_t w = 0; w < wave; ++w) dst += s_wave[w];
        s_src[threadIdx.x] = i < n_rec ? r_src[i] : 0;
        s_dst[threadIdx.x] = dst;
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
    const uint32_t n_tiles = (uint32_t)((hi + kSqTile - 1) / kSqTile), grid = n_tiles ? n_tiles : 1;
    uint32_t *tile_cnt = reinterpret_cast<uint32_t *>(d_scratch + p.tile_cnt), *nl = reinterpret_cast<uint32_t *>(d_scratch + p.nl);
    uint32_t *r_src = reinterpret_cast<uint32_t *>(d_scratch + p.r_src), *r_len = reinterpret_cast<uint32_t *>(d_scratch + p.r_len);
    uint32_t *r_tile = reinterpret_cast<uint32_t *>(d_scratch + p.r_tile);
    SqState *st = reinterpret_cast<SqState *>(d_scratch + p.state);
    const uint32_t max_rec_tiles = (uint32_t)((n_in / 4 + kSqRecTile - 1) / kSqRecTile), rec_grid = max_rec_tiles < 1 ? 1 : max_rec_tiles < 2048 ? max_rec_tiles : 2048;
    hipLaunchKernelGGL(k_sq_count, dim3(grid), dim3(256), 0, s, base, lo, hi, tile_cnt);
    hipLaunchKernelGGL(k_sq_scan, dim3(1), dim3(1024), 0, s, tile_cnt, grid, st);
    hipLaunchKernelGGL(k_sq_index, dim3(grid), dim3(256), 0, s, base, lo, hi, tile_cnt, nl);
    hipLaunchKernelGGL(k_sq_records, dim3(rec_grid), dim3(kSqRecTile), 0, s, d_in, st, nl, r_src, r_len, r_tile);
    hipLaunchKernelGGL(k_sq_scan_out, dim3(1), dim3(1024), 0, s, r_tile, st);
    hipLaunchKernelGGL(k_sq_copy, dim3(rec_grid), dim3(kSqRecTile), 0, s, d_in, st, r_src, r_len, r_tile, d_out);
    return hipGetLastError();
}

}  // namespace hast
