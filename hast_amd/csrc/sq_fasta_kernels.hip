// sq_fasta_kernels.hip -- gfx950 device code: a view of raw FASTA in HBM becomes the base stream hast_kc_count_device eats (stage 00
// ingest on the device, `unshared_kmers --device-fasta`).  The rules are sq_core.h's (namespace sqfa); the steps, all on one stream:
//   k_nl_count / k_sqfa_scan / k_nl_index   the newline index (nl_kernels.hip)
//   k_sqfa_lines       a lane per line: stripped length, class, emitted bytes; per tile of 256 lines the headers and the emitted bytes
//   k_sqfa_scan_lines  one workgroup scans both tile sums; the view's results
//   k_sqfa_line_dst    a lane per line: line_dst[j] = where in the output line j's bytes start
//   k_sqfa_copy        the lines compacted into the stream (span_copy.h)
// A line is anything from a 7-column test file's through an assembler's 60 columns and a 150-base read to a chromosome on one line.
// The view and the output may start at any address (nl_index.h, span_copy.h): nothing outside [d_in, d_in + n_in) is read and
// nothing at or behind d_out + out_bytes is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nl_index.h"
#include "sq_device.h"
#include "span_copy.h"

namespace hast {

__global__ void __launch_bounds__(1024) k_sqfa_scan(uint32_t *tile_cnt, uint32_t n, SqFaState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_nl = block_exclusive_scan_1024(tile_cnt, n, s_part);
    if (threadIdx.x == 0) {
        st->consumed = st->out_bytes = st->records = st->bases = 0;
        st->flags = 0;
        st->first_bad = sq::kNoBad;
        st->n_nl = n_nl;
        st->n_lines = st->lines_bytes = 0;
    }
}

struct SqFaLine {
    uint32_t h, e;             // a header; sqfa::raw_emit
};
__device__ __forceinline__ SqFaLine sqfa_line(const uint8_t *in, const uint32_t *nl, uint32_t n_nl, uint64_t n_in, uint32_t j) {
    uint32_t len;
    const uint32_t cls = sqfa::line_class(in, sqfa::line_lo(nl, j), sqfa::line_hi(nl, n_nl, n_in, j), &len);
    SqFaLine x;
    x.h = cls == sqfa::kHeader;
    x.e = sqfa::raw_emit(cls, len);
    return x;
}

__global__ void __launch_bounds__(kSqFaTile) k_sqfa_lines(const uint8_t *in, uint64_t n_in, int last, SqFaState *st, const uint32_t *nl, uint32_t *tile_h,
                                                          uint32_t *tile_e) {
    __shared__ uint32_t s_h[4], s_e[4];
    const uint32_t n_nl = st->n_nl, n_lines = sqfa::n_lines(nl, n_nl, n_in, last != 0), n_tiles = (n_lines + kSqFaTile - 1) / kSqFaTile;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->n_lines = n_lines;
        st->consumed = sqfa::consumed(nl, n_nl, n_in, last != 0);
    }
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t j = tile * kSqFaTile + threadIdx.x;
        SqFaLine x;
        x.h = x.e = 0;
        if (j < n_lines) x = sqfa_line(in, nl, n_nl, n_in, j);
        __syncthreads();                                         // (the sums of the tile before have been read)
        const uint32_t sum_h = block_sum_256(x.h, s_h), sum_e = block_sum_256(x.e, s_e);
        if (threadIdx.x == 0) {
            tile_h[tile] = sum_h;
            tile_e[tile] = sum_e;
        }
    }
}

__global__ void __launch_bounds__(1024) k_sqfa_scan_lines(uint32_t *tile_h, uint32_t *tile_e, SqFaState *st, int open_in, int last) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_tiles = (st->n_lines + kSqFaTile - 1) / kSqFaTile;
    const uint32_t m = block_exclusive_scan_1024(tile_h, n_tiles, s_part);
    __syncthreads();                                             // (s_part is written again)
    const uint32_t raw = block_exclusive_scan_1024(tile_e, n_tiles, s_part);
    if (threadIdx.x == 0) {
        const uint32_t lines_bytes = sqfa::line_dst(raw, m, open_in != 0);
        st->records = m;
        st->bases = sqfa::bases(raw, m);
        st->lines_bytes = lines_bytes;
        st->out_bytes = (uint64_t)lines_bytes + sqfa::closing(m, open_in != 0, last != 0);
    }
}

__global__ void __launch_bounds__(kSqFaTile) k_sqfa_line_dst(const uint8_t *in, uint64_t n_in, const SqFaState *st, const uint32_t *nl, const uint32_t *tile_h,
                                                             const uint32_t *tile_e, int open_in, uint32_t *line_dst) {
    __shared__ uint32_t s_wh[4], s_we[4];
    const uint32_t n_nl = st->n_nl, n_lines = st->n_lines, n_tiles = (n_lines + kSqFaTile - 1) / kSqFaTile;
    if (blockIdx.x == 0 && threadIdx.x == 0) line_dst[n_lines] = st->lines_bytes;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t j = tile * kSqFaTile + threadIdx.x;
        SqFaLine x;
        x.h = x.e = 0;
        if (j < n_lines) x = sqfa_line(in, nl, n_nl, n_in, j);
        const uint32_t eh = tile_h[tile] + block_exclusive_sum_256(x.h, s_wh);
        const uint32_t ee = tile_e[tile] + block_exclusive_sum_256(x.e, s_we);
        if (j < n_lines) line_dst[j] = sqfa::line_dst(ee, eh, open_in != 0);
        __syncthreads();                                         // (s_wh, s_we are written again)
    }
}

// out[0, lines_bytes) = what the lines emit, back to back (span_copy.h), and the closing '\n' behind it.  out = out16 + olo with out16
// 16-byte aligned.  A line that emits and starts with '>' is a header: its one byte is '\n'.  An empty line, the header that opens the
// input: nothing of them is output.
struct SqFaLineSrc {
    static constexpr bool kFills = true;
    const uint8_t *in;
    const uint32_t *nl;
    __device__ __forceinline__ const uint8_t *at(uint32_t j) const { return in + sqfa::line_lo(nl, j); }
    __device__ __forceinline__ bool fill(const uint8_t *line) const { return line[0] == '>'; }
};
__global__ void __launch_bounds__(256) k_sqfa_copy(const uint8_t *in, const SqFaState *st, const uint32_t *nl, const uint32_t *line_dst,
                                                   uint8_t *out16, uint32_t olo) {
    const uint32_t total = st->lines_bytes, n_lines = st->n_lines;
    if (blockIdx.x == 0 && threadIdx.x == 0 && st->out_bytes > total) out16[olo + total] = '\n';
    if (!total) return;
    span_copy(line_dst, 0, n_lines - 1, 0, total, out16, olo, SqFaLineSrc{in, nl});
}

hipError_t launch_sq_fasta_frame(const uint8_t *d_in, size_t n_in, uint8_t *d_out, unsigned in_flags, uint8_t *d_scratch, const SqFaScratchPlan &p,
                                 hipStream_t s) {
    const uint32_t olo = (uint32_t)(reinterpret_cast<uintptr_t>(d_out) & 15);
    const int open_in = (in_flags & SQ_FA_OPEN) != 0, last = (in_flags & SQ_FA_LAST) != 0;
    auto words = [&](size_t at) { return reinterpret_cast<uint32_t *>(d_scratch + at); };
    uint32_t *tile_cnt = words(p.tile_cnt), *nl = words(p.nl), *tile_h = words(p.tile_h), *tile_e = words(p.tile_e), *line_dst = words(p.line_dst);
    SqFaState *st = reinterpret_cast<SqFaState *>(d_scratch + p.state);
    const uint32_t line_grid = capped_grid(n_in + 1, kSqFaTile), copy_grid = capped_grid(n_in + 16, kSpanCopyTile);
    const NlSides view{{nl_range(d_in, n_in)}, {tile_cnt}, {nl}};
    const uint32_t grid = view.r[0].grid();
    launch_nl_count(view, 1, grid, s);
    hipLaunchKernelGGL(k_sqfa_scan, dim3(1), dim3(1024), 0, s, tile_cnt, grid, st);
    launch_nl_index(view, 1, grid, s);
    hipLaunchKernelGGL(k_sqfa_lines, dim3(line_grid), dim3(kSqFaTile), 0, s, d_in, (uint64_t)n_in, last, st, (const uint32_t *)nl, tile_h, tile_e);
    hipLaunchKernelGGL(k_sqfa_scan_lines, dim3(1), dim3(1024), 0, s, tile_h, tile_e, st, open_in, last);
    hipLaunchKernelGGL(k_sqfa_line_dst, dim3(line_grid), dim3(kSqFaTile), 0, s, d_in, (uint64_t)n_in, (const SqFaState *)st, (const uint32_t *)nl,
                       (const uint32_t *)tile_h, (const uint32_t *)tile_e, open_in, line_dst);
    hipLaunchKernelGGL(k_sqfa_copy, dim3(copy_grid), dim3(256), 0, s, d_in, (const SqFaState *)st, (const uint32_t *)nl, (const uint32_t *)line_dst,
                       d_out - olo, olo);
    return hipGetLastError();
}

}  // namespace hast
