// rs_kernels.hip -- gfx950 device code: a view of raw FASTA or four-line FASTQ in HBM becomes the reads of stage 03's per-read
// classifier (`classify_read --ingest device`).  The rules are rs_core.h's; the steps, all on one stream:
//   k_nl_count / k_rs_scan / k_nl_index   the newline index (nl_kernels.hip)
//   k_rs_lines       FASTA, a lane per line: its class and length; per tile of 256 lines the headers and the sequence bytes
//   k_rs_scan_lines  FASTA: exclusive scans of the two tile sums
//   k_rs_line_dst    FASTA, a lane per line: line_dst[j] = sequence bytes in front of line j, hdr_line[r] = the line of header r
//   k_rs_records     a lane per record: name extent, start and length of the read, the format error; consumed and the counts
//   k_rs_scan_names  exclusive scan of the name lengths per tile of 256 records
//   k_rs_names       names gathered back to back (record_gather.h)
//   k_rs_copy        FASTA: the sequence lines compacted into one base buffer (span_copy.h)
//   k_rb_*           `--bin-reads` (rb_core.h), behind the classification: the records routed to three runs by their votes; see below
// FASTQ reads are classified where they lie in the view; a FASTA read is spread over lines, and a k-mer straddles the line breaks,
// so its lines are moved together.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nl_index.h"
#include "rb_core.h"
#include "record_gather.h"
#include "rs_device.h"
#include "span_copy.h"

namespace hast {

__global__ void __launch_bounds__(1024) k_rs_scan(uint32_t *tile_cnt, uint32_t n, RsState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_nl = block_exclusive_scan_1024(tile_cnt, n, s_part);
    if (threadIdx.x == 0) {
        st->consumed = st->records = st->bases = st->name_bytes = 0;
        st->flags = 0;
        st->n_nl = n_nl;
        st->n_hdr = st->seq_total = 0;
    }
}

__global__ void __launch_bounds__(kRsTile) k_rs_lines(const uint8_t *in, RsState *st, const uint32_t *nl, uint32_t *tile_h, uint32_t *tile_s) {
    __shared__ uint32_t s_h[4], s_s[4];
    const uint32_t n_lines = st->n_nl, n_tiles = (n_lines + kRsTile - 1) / kRsTile;
    bool bad = false;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t j = tile * kRsTile + threadIdx.x;
        uint32_t h = 0, s = 0;
        if (j < n_lines) {
            const uint32_t lo = rs::line_lo(nl, j), hi = nl[j], cls = rs::fa_class(in, lo, hi);
            h = cls == rs::kHeader;
            s = rs::fa_seq_len(cls, lo, hi);
            bad |= cls == rs::kBad;
        }
        __syncthreads();                                         // (the sums of the tile before have been read)
        const uint32_t sum_h = block_sum_256(h, s_h), sum_s = block_sum_256(s, s_s);
        if (threadIdx.x == 0) {
            tile_h[tile] = sum_h;
            tile_s[tile] = sum_s;
        }
    }
    if (bad) atomicOr(&st->flags, RS_FORMAT_ERROR);
}

__global__ void __launch_bounds__(1024) k_rs_scan_lines(uint32_t *tile_h, uint32_t *tile_s, RsState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_tiles = (st->n_nl + kRsTile - 1) / kRsTile;
    const uint32_t m = block_exclusive_scan_1024(tile_h, n_tiles, s_part);
    __syncthreads();                                             // (s_part is written again)
    const uint32_t total = block_exclusive_scan_1024(tile_s, n_tiles, s_part);
    if (threadIdx.x == 0) {
        st->n_hdr = m;
        st->seq_total = total;
    }
}

__global__ void __launch_bounds__(kRsTile) k_rs_line_dst(const uint8_t *in, const RsState *st, const uint32_t *nl, const uint32_t *tile_h, const uint32_t *tile_s,
                                                         uint32_t *line_dst, uint32_t *hdr_line) {
    __shared__ uint32_t s_wh[4], s_ws[4];
    const uint32_t n_lines = st->n_nl, n_tiles = (n_lines + kRsTile - 1) / kRsTile;
    if (n_lines == 0 && blockIdx.x == 0 && threadIdx.x == 0) line_dst[0] = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t j = tile * kRsTile + threadIdx.x;
        uint32_t h = 0, s = 0;
        if (j < n_lines) {
            const uint32_t lo = rs::line_lo(nl, j), hi = nl[j], cls = rs::fa_class(in, lo, hi);
            h = cls == rs::kHeader;
            s = rs::fa_seq_len(cls, lo, hi);
        }
        const uint32_t eh = tile_h[tile] + block_exclusive_sum_256(h, s_wh);
        const uint32_t es = tile_s[tile] + block_exclusive_sum_256(s, s_ws);
        if (j < n_lines) {
            line_dst[j] = es;
            if (h) hdr_line[eh] = j;
            if (j == n_lines - 1) line_dst[n_lines] = es + s;
        }
        __syncthreads();                                         // (s_wh, s_ws are written again)
    }
}

__global__ void __launch_bounds__(kRsTile) k_rs_records(int format, const uint8_t *in, uint64_t n, uint64_t origin, int last, int seen_header, RsState *st,
                                                        const uint32_t *nl, const uint32_t *line_dst, const uint32_t *hdr_line, uint32_t *name_pos,
                                                        uint32_t *name_len, uint32_t *name_tile, uint64_t *r_off, uint32_t *r_len) {
    __shared__ uint32_t s_n[4], s_b[4];
    const uint32_t n_nl = st->n_nl, m = st->n_hdr, total = st->seq_total;
    const bool fastq = format == RS_FASTQ;
    const uint32_t n_rec = fastq ? rs::fq_records(n_nl) : rs::fa_records(m, last != 0);
    const uint32_t n_tiles = (n_rec + kRsTile - 1) / kRsTile;
    const uint32_t junk = !fastq && m ? line_dst[hdr_line[0]] : 0;      // sequence bytes in front of the view's first header: no record's
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->records = n_rec;
        st->consumed = fastq ? rs::fq_consumed(nl, n_nl) : rs::fa_consumed(nl, n_nl, n, m, m ? hdr_line[m - 1] : 0, last != 0, seen_header != 0);
    }
    unsigned long long bases = 0;                                // lane 0 of the workgroup: over all its tiles
    bool bad = false;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r = tile * kRsTile + threadIdx.x;
        uint32_t nlen = 0, len = 0;
        if (r < n_rec) {
            const uint32_t hl = fastq ? 4 * r : hdr_line[r];
            const uint32_t lo = rs::line_lo(nl, hl), hi = nl[hl];
            uint32_t npos;
            rs::name_of(lo, hi, &npos, &nlen);
            uint64_t off;
            if (fastq) {
                bad |= rs::fq_bad_header(in, lo, hi);
                off = origin + hi + 1;
                len = nl[hl + 1] - (hi + 1);
            } else {
                const uint32_t a = line_dst[hl], b = r + 1 < m ? line_dst[hdr_line[r + 1]] : total;
                off = a - junk;
                len = b - a;
            }
            name_pos[r] = npos;
            name_len[r] = nlen;
            r_off[r] = off;
            r_len[r] = len;
        }
        __syncthreads();                                         // (the sums of the tile before have been read)
        const uint32_t sum_n = block_sum_256(nlen, s_n), sum_b = block_sum_256(len, s_b);
        if (threadIdx.x == 0) {
            name_tile[tile] = sum_n;
            bases += sum_b;
        }
    }
    if (threadIdx.x == 0 && bases) atomicAdd(reinterpret_cast<unsigned long long *>(&st->bases), bases);
    if (bad) atomicOr(&st->flags, RS_FORMAT_ERROR);
}

__global__ void __launch_bounds__(1024) k_rs_scan_names(uint32_t *name_tile, RsState *st) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_rec = (uint32_t)st->records;
    const uint32_t total = block_exclusive_scan_1024(name_tile, (n_rec + kRsTile - 1) / kRsTile, s_part);
    if (threadIdx.x == 0) st->name_bytes = total;
}

__global__ void __launch_bounds__(kRsTile) k_rs_names(const uint8_t *in, const RsState *st, const uint32_t *name_pos, const uint32_t *name_len,
                                                      const uint32_t *name_tile, uint32_t *name_off, uint8_t *names) {
    __shared__ uint32_t s_wave[4];
    const uint32_t n_rec = (uint32_t)st->records, n_tiles = (n_rec + kRsTile - 1) / kRsTile;
    if (blockIdx.x == 0 && threadIdx.x == 0) name_off[n_rec] = (uint32_t)st->name_bytes;
    if (st->flags) return;                                       // the format error: nobody reads the names
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r = tile * kRsTile + threadIdx.x;
        const uint32_t len = r < n_rec ? name_len[r] : 0;
        const uint32_t dst = name_tile[tile] + block_exclusive_sum_256(len, s_wave);
        if (r < n_rec) name_off[r] = dst;
        record_gather_256<GatherBytes>(in, names, r < n_rec ? name_pos[r] : 0, dst, len, n_rec - tile * kRsTile);
    }
}

// out[0, bases) = the sequence lines of the complete records, back to back (span_copy.h).  Byte p of the output is byte p + junk of the
// sequence bytes of ALL lines in view order (line_dst counts those); a header or an empty line emits nothing, and the lines behind the
// last complete record lie behind the output.
struct RsLineSrc {
    static constexpr bool kFills = false;
    const uint8_t *in;
    const uint32_t *nl;
    __device__ __forceinline__ const uint8_t *at(uint32_t j) const { return in + rs::line_lo(nl, j); }
};
__global__ void __launch_bounds__(256) k_rs_copy(const uint8_t *in, const RsState *st, const uint32_t *nl, const uint32_t *line_dst, const uint32_t *hdr_line,
                                                 uint8_t *out) {
    const uint32_t m = st->n_hdr, bases = (uint32_t)st->bases, n_lines = st->n_nl;
    if (!m || !bases || st->flags) return;
    const uint32_t h0 = hdr_line[0], junk = line_dst[h0];
    span_copy(line_dst, h0, n_lines - 1, junk, bases, out, 0, RsLineSrc{in, nl});
}

hipError_t launch_rs_frame(int format, const uint8_t *d_base, size_t origin, size_t n, bool last, bool seen_header, uint8_t *d_seq, uint8_t *d_names,
                           uint8_t *d_scratch, const RsScratchPlan &p, hipStream_t s) {
    const uint8_t *in = d_base + origin;
    auto words = [&](size_t at) { return reinterpret_cast<uint32_t *>(d_scratch + at); };
    uint32_t *tile_cnt = words(p.tile_cnt), *nl = words(p.nl), *tile_h = words(p.line_tile_h), *tile_s = words(p.line_tile_s), *line_dst = words(p.line_dst);
    uint32_t *hdr_line = words(p.hdr_line), *name_pos = words(p.name_pos), *name_len = words(p.name_len), *name_tile = words(p.name_tile);
    uint32_t *name_off = words(p.name_off), *r_len = words(p.len);
    uint64_t *r_off = reinterpret_cast<uint64_t *>(d_scratch + p.off);
    RsState *st = reinterpret_cast<RsState *>(d_scratch + p.state);
    const bool fasta = format == RS_FASTA;
    const uint32_t line_grid = capped_grid(n, kRsTile), rec_grid = capped_grid(fasta ? n / 2 + 1 : n / 4 + 1, kRsTile), copy_grid = capped_grid(n, kSpanCopyTile);
    const NlSides view{{nl_range(in, n)}, {tile_cnt}, {nl}};
    const uint32_t grid = view.r[0].grid();
    launch_nl_count(view, 1, grid, s);
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, tile_cnt, grid, st);
    launch_nl_index(view, 1, grid, s);
    if (fasta) {
        hipLaunchKernelGGL(k_rs_lines, dim3(line_grid), dim3(kRsTile), 0, s, in, st, nl, tile_h, tile_s);
        hipLaunchKernelGGL(k_rs_scan_lines, dim3(1), dim3(1024), 0, s, tile_h, tile_s, st);
        hipLaunchKernelGGL(k_rs_line_dst, dim3(line_grid), dim3(kRsTile), 0, s, in, st, nl, tile_h, tile_s, line_dst, hdr_line);
    }
    hipLaunchKernelGGL(k_rs_records, dim3(rec_grid), dim3(kRsTile), 0, s, format, in, (uint64_t)n, (uint64_t)origin, (int)last, (int)seen_header, st, nl, line_dst,
                       hdr_line, name_pos, name_len, name_tile, r_off, r_len);
    hipLaunchKernelGGL(k_rs_scan_names, dim3(1), dim3(1024), 0, s, name_tile, st);
    hipLaunchKernelGGL(k_rs_names, dim3(rec_grid), dim3(kRsTile), 0, s, in, st, name_pos, name_len, name_tile, name_off, d_names);
    if (fasta) hipLaunchKernelGGL(k_rs_copy, dim3(copy_grid), dim3(256), 0, s, in, st, nl, line_dst, hdr_line, d_seq);
    return hipGetLastError();
}

// ---- the read bins (rb_core.h): every record, as it lies in the view, to the run of its class ------------------------------------
//   k_rb_sums    a lane per record: class and extent; per tile of 256 records the records and the bytes of each class
//   k_rb_scan    exclusive scans of the two tile sums, laid out class by class: a tile's entry is where its class-c records start
//   k_rb_place   the stable partition: order[j] = the record at place j, dst[j] = its offset in the output (monotone: class 0's
//                records in input order, then class 1's, then class 2's)
//   k_rb_copy    the records compacted into the output in that order (span_copy.h): a record is anything from ">\n" to one line of
//                10^8 bases
struct RbRecord {
    uint32_t cls, lo, len;
};
__device__ __forceinline__ RbRecord rb_record(bool fastq, const uint32_t *nl, uint32_t n_nl, const uint32_t *hdr_line, uint32_t m, const uint32_t *votes,
                                              uint32_t total0, uint32_t total1, uint32_t r) {
    uint32_t lo, hi;
    if (fastq) rb::fq_extent(nl, r, &lo, &hi);
    else rb::fa_extent(nl, n_nl, hdr_line, m, r, &lo, &hi);
    RbRecord x;
    x.cls = rb::read_class(votes[2 * (size_t)r], votes[2 * (size_t)r + 1], total0, total1);
    x.lo = lo;
    x.len = hi - lo;
    return x;
}

__global__ void __launch_bounds__(kRsTile) k_rb_sums(int format, const RsState *st, const uint32_t *nl, const uint32_t *hdr_line, const uint32_t *votes,
                                                     uint32_t total0, uint32_t total1, uint32_t *tile_cnt, uint32_t *tile_bytes) {
    __shared__ uint32_t s_c[rb::kClasses][4], s_b[rb::kClasses][4];
    const uint32_t n_rec = (uint32_t)st->records, n_tiles = (n_rec + kRsTile - 1) / kRsTile, n_nl = st->n_nl, m = st->n_hdr;
    const bool fastq = format == RS_FASTQ;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r = tile * kRsTile + threadIdx.x;
        uint32_t cls = rb::kClasses, len = 0;
        if (r < n_rec) {
            const RbRecord x = rb_record(fastq, nl, n_nl, hdr_line, m, votes, total0, total1, r);
            cls = x.cls;
            len = x.len;
        }
        __syncthreads();                                         // (the sums of the tile before have been read)
        for (uint32_t c = 0; c < rb::kClasses; ++c) {
            const uint32_t sum_c = block_sum_256(cls == c, s_c[c]), sum_b = block_sum_256(cls == c ? len : 0, s_b[c]);
            if (threadIdx.x == 0) {
                tile_cnt[c * n_tiles + tile] = sum_c;
                tile_bytes[c * n_tiles + tile] = sum_b;
            }
        }
    }
}

__global__ void __launch_bounds__(1024) k_rb_scan(const RsState *st, uint32_t *tile_cnt, uint32_t *tile_bytes, RbState *rb) {
    __shared__ uint32_t s_part[1024];
    const uint32_t n_rec = (uint32_t)st->records, n_tiles = (n_rec + kRsTile - 1) / kRsTile;
    const uint32_t records = block_exclusive_scan_1024(tile_cnt, 3 * n_tiles, s_part);
    __syncthreads();                                             // (s_part is written again)
    const uint32_t bytes = block_exclusive_scan_1024(tile_bytes, 3 * n_tiles, s_part);
    __syncthreads();                                             // (the scanned sums of the other threads are read)
    if (threadIdx.x < 3) {
        const uint32_t c = threadIdx.x;
        const uint32_t c_lo = n_tiles ? tile_cnt[c * n_tiles] : 0, c_hi = n_tiles && c < 2 ? tile_cnt[(c + 1) * n_tiles] : records;
        const uint32_t b_lo = n_tiles ? tile_bytes[c * n_tiles] : 0, b_hi = n_tiles && c < 2 ? tile_bytes[(c + 1) * n_tiles] : bytes;
        rb->count[c] = c_hi - c_lo;
        rb->raw_bytes[c] = b_hi - b_lo;
        if (c == 0) rb->total = bytes;
    }
}

__global__ void __launch_bounds__(kRsTile) k_rb_place(int format, const RsState *st, const uint32_t *nl, const uint32_t *hdr_line, const uint32_t *votes,
                                                      uint32_t total0, uint32_t total1, const uint32_t *tile_cnt, const uint32_t *tile_bytes, const RbState *rb,
                                                      uint32_t *order, uint32_t *dst) {
    __shared__ uint32_t s_wc[4], s_wb[4];
    const uint32_t n_rec = (uint32_t)st->records, n_tiles = (n_rec + kRsTile - 1) / kRsTile, n_nl = st->n_nl, m = st->n_hdr;
    const bool fastq = format == RS_FASTQ;
    if (blockIdx.x == 0 && threadIdx.x == 0) dst[n_rec] = (uint32_t)rb->total;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r = tile * kRsTile + threadIdx.x;
        RbRecord x;
        x.cls = rb::kClasses, x.lo = 0, x.len = 0;
        if (r < n_rec) x = rb_record(fastq, nl, n_nl, hdr_line, m, votes, total0, total1, r);
        uint32_t place = 0, at = 0;
        for (uint32_t c = 0; c < rb::kClasses; ++c) {
            const uint32_t ec = block_exclusive_sum_256(x.cls == c, s_wc), eb = block_exclusive_sum_256(x.cls == c ? x.len : 0, s_wb);
            if (x.cls == c) {
                place = tile_cnt[c * n_tiles + tile] + ec;
                at = tile_bytes[c * n_tiles + tile] + eb;
            }
            __syncthreads();                                     // (s_wc, s_wb are written again)
        }
        if (r < n_rec) {
            order[place] = r;
            dst[place] = at;
        }
    }
}

// out[0, total) = the three runs (span_copy.h): item j is the record at place j, and its source lies wherever order[j] says.
struct RbRecordSrc {
    static constexpr bool kFills = false;
    const uint8_t *in;
    const uint32_t *nl, *hdr_line, *order;
    bool fastq;
    __device__ __forceinline__ const uint8_t *at(uint32_t j) const {
        const uint32_t r = order[j];
        return in + rs::line_lo(nl, fastq ? 4 * r : hdr_line[r]);
    }
};
__global__ void __launch_bounds__(256) k_rb_copy(int format, const uint8_t *in, const RsState *st, const uint32_t *nl, const uint32_t *hdr_line, const RbState *rb,
                                                 const uint32_t *order, const uint32_t *dst, uint8_t *out) {
    const uint32_t n_rec = (uint32_t)st->records, total = (uint32_t)rb->total;
    if (!n_rec || !total) return;
    span_copy(dst, 0, n_rec - 1, 0, total, out, 0, RbRecordSrc{in, nl, hdr_line, order, format == RS_FASTQ});
}

hipError_t launch_rb_bin(int format, const uint8_t *d_base, size_t origin, size_t n, uint32_t total0, uint32_t total1, const uint8_t *d_scratch,
                         const RsScratchPlan &p, uint8_t *d_rb, const RbScratchPlan &q, uint8_t *d_out, hipStream_t s) {
    const uint8_t *in = d_base + origin;
    auto words = [&](size_t at) { return reinterpret_cast<const uint32_t *>(d_scratch + at); };
    auto own = [&](size_t at) { return reinterpret_cast<uint32_t *>(d_rb + at); };
    const uint32_t *nl = words(p.nl), *hdr_line = words(p.hdr_line), *votes = words(p.votes);
    const RsState *st = reinterpret_cast<const RsState *>(d_scratch + p.state);
    RbState *rb = reinterpret_cast<RbState *>(d_rb + q.state);
    uint32_t *order = own(q.order), *dst = own(q.dst), *tile_cnt = own(q.tile_cnt), *tile_bytes = own(q.tile_bytes);
    const uint32_t rec_grid = capped_grid(format == RS_FASTA ? n / 2 + 1 : n / 4 + 1, kRsTile), copy_grid = capped_grid(n, kSpanCopyTile);
    hipLaunchKernelGGL(k_rb_sums, dim3(rec_grid), dim3(kRsTile), 0, s, format, st, nl, hdr_line, votes, total0, total1, tile_cnt, tile_bytes);
    hipLaunchKernelGGL(k_rb_scan, dim3(1), dim3(1024), 0, s, st, tile_cnt, tile_bytes, rb);
    hipLaunchKernelGGL(k_rb_place, dim3(rec_grid), dim3(kRsTile), 0, s, format, st, nl, hdr_line, votes, total0, total1, (const uint32_t *)tile_cnt,
                       (const uint32_t *)tile_bytes, (const RbState *)rb, order, dst);
    hipLaunchKernelGGL(k_rb_copy, dim3(copy_grid), dim3(256), 0, s, format, in, st, nl, hdr_line, (const RbState *)rb, (const uint32_t *)order,
                       (const uint32_t *)dst, d_out);
    return hipGetLastError();
}

}  // namespace hast
