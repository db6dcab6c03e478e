// rs_api.cpp -- the part of the C ABI behind `classify_read --ingest device` (include/hast.h "stage 03 ingest on the device"): raw
// FASTA / FASTQ bytes in HBM are framed into reads (rs_kernels.hip, rules: rs_core.h) and classified per read where they lie; with
// the rows switched on (`--rows device`; rr_kernels.hip, rules: rr_core.h) their rows are made there too and only text comes back.
#include <hip/hip_runtime.h>

#include <new>

#include "carry_feed.h"
#include "dz_device.h"
#include "hast_internal.h"
#include "rs_device.h"

using namespace hast;

static_assert(HAST_RS_FASTA == RS_FASTA && HAST_RS_FASTQ == RS_FASTQ, "hast.h and rs_core.h name the same formats");
static_assert(HAST_RS_FORMAT_ERROR == RS_FORMAT_ERROR && HAST_RS_RECORD_TOO_LONG == RS_RECORD_TOO_LONG, "hast.h and rs_core.h name the same flags");

// over a carried-block feed (carry_plan.h, carry_feed.h) on the context's stream
struct hast_rs {
    hast_ctx *ctx = nullptr;
    int format = 0;
    CarryFeed in;
    RsScratchPlan plan;
    uint8_t *d_seq = nullptr, *d_names = nullptr, *d_scratch = nullptr;
    RsState *h_st = nullptr;                                 // pinned
    uint32_t *h_votes = nullptr, *h_name_off = nullptr;      // pinned, grown to the largest block so far
    uint8_t *h_names = nullptr;
    size_t cap_rec = 0, cap_names = 0;
    bool is_last[2] = {false, false};
    bool seen_header = false;                                // FASTA: a header line has been framed in this file
    bool file_done = false;                                  // FASTQ: the tail is a finished file's (hast_rs_take_tail)
    uint32_t given_up = 0;                                   // the flags that ended this file: its other blocks are not looked at
    // the read bins (hast_rs_set_bins): nothing of this is allocated before they are first switched on
    int bin_mode = 0;                                        // 0 off, 1 plain, 2 gzip
    uint32_t bin_total[2] = {0, 0};
    RbScratchPlan rb_plan{};
    uint8_t *d_rb = nullptr, *d_out = nullptr, *h_out = nullptr;       // per-record arrays; the three runs of a view, device and pinned
    RbState *h_rb = nullptr;                                 // pinned
    uint8_t *d_gz = nullptr, *h_gz = nullptr;                // gzip: the members, device and pinned
    dz::EncoderSlot enc;
    dz::Result *h_dzres = nullptr;                           // pinned
    size_t gz_cap = 0;
    // the rows (hast_rs_set_rows): nothing of this is allocated before they are first switched on
    int row_mode = 0;
    uint32_t row_total[2] = {0, 0};
    RrScratchPlan rr_plan{};
    uint8_t *d_rr = nullptr, *d_rows = nullptr, *h_rows = nullptr;     // tile sums and state; the text of a view, device and pinned
    RrState *h_rr = nullptr;                                 // pinned
    size_t rows_cap = 0;
};

// The room for a view's rows, device and pinned: block_bytes, half of what a view can hold.  Reads as sequencers name them need about
// 0.15 x their bytes, long reads next to nothing; only records of a few bytes each need more than half (">\n" makes a row of 15), and
// such a view goes to the host.
static size_t rows_room(size_t block_bytes) { return block_bytes; }

extern "C" {

hast_status hast_rs_create(hast_ctx *ctx, int format, size_t block_bytes, hast_rs **out) {
    if (!ctx || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (format != HAST_RS_FASTA && format != HAST_RS_FASTQ) return set_error(HAST_ERR_INVALID, "hast_rs_create: format %d", format);
    if (block_bytes < 64 || block_bytes > (1ull << 30)) return set_error(HAST_ERR_INVALID, "hast_rs_create: blocks of %zu bytes (64 .. 2^30)", block_bytes);
    hast_rs *f = new (std::nothrow) hast_rs;
    if (!f) return set_error(HAST_ERR_OOM, "hast_rs_create");
    f->ctx = ctx;
    f->format = format;
    f->plan = rs_scratch_plan(format, 2 * block_bytes);
    hipError_t e = f->in.create("hast_rs", ctx_device_of(ctx), ctx_stream_of(ctx), block_bytes);
    if (e == hipSuccess) e = dev_malloc(&f->d_scratch, f->plan.total);
    if (e == hipSuccess) e = dev_malloc(&f->d_names, carry::room_of(block_bytes));
    if (e == hipSuccess && format == HAST_RS_FASTA) e = dev_malloc(&f->d_seq, carry::room_of(block_bytes));
    if (e == hipSuccess) e = pinned_malloc(&f->h_st, sizeof(RsState));
    if (e != hipSuccess) {
        const size_t total = f->plan.total;
        hast_rs_destroy(f);
        return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_rs_create: blocks of %zu bytes, %zu of scratch: %s", block_bytes, total,
                         hipGetErrorString(e));
    }
    *out = f;
    return HAST_OK;
}

hast_status hast_rs_host_block(hast_rs *f, uint8_t **h_buf) { return f ? f->in.block(1, h_buf) : set_error(HAST_ERR_INVALID, "null feed"); }

hast_status hast_rs_device_block(hast_rs *f, uint8_t **d_buf, hast_stream *fill) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (hast_status st = f->in.block(2, d_buf)) return st;
    if (fill) *fill = f->in.stream;
    return HAST_OK;
}

hast_status hast_rs_submit(hast_rs *f, size_t n_bytes, int last) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    const int slot = f->in.plan.submit_slot();
    if (hast_status st = f->in.submit(n_bytes, last != 0)) return st;        // (a file's last block may be empty)
    f->is_last[slot] = last != 0;
    return HAST_OK;
}

static hast_status rs_grow(hast_rs *f, size_t records, size_t name_bytes) {
    if (records + 1 > f->cap_rec) {
        const size_t cap = records + records / 2 + 1024;
        park_pinned(f->h_votes, f->cap_rec * 8, 3);
        park_pinned(f->h_name_off, f->cap_rec * 4, 3);
        f->h_votes = f->h_name_off = nullptr;
        f->cap_rec = 0;
        HAST_HIP_TRY(pinned_malloc(&f->h_votes, cap * 8));
        HAST_HIP_TRY(pinned_malloc(&f->h_name_off, cap * 4));
        f->cap_rec = cap;
    }
    if (name_bytes > f->cap_names) {
        const size_t cap = name_bytes + name_bytes / 2 + 4096;
        park_pinned(f->h_names, f->cap_names, 3);
        f->h_names = nullptr;
        f->cap_names = 0;
        HAST_HIP_TRY(pinned_malloc(&f->h_names, cap));
        f->cap_names = cap;
    }
    return HAST_OK;
}

// the buffers of the bins, at the first switch-on of a mode that needs them
static hast_status rb_alloc(hast_rs *f, int mode) {
    const size_t view = 2 * f->in.plan.block;
    if (!f->d_rb) {
        f->rb_plan = rb_scratch_plan(f->plan);
        HAST_HIP_TRY(dev_malloc(&f->d_rb, f->rb_plan.total));
        HAST_HIP_TRY(dev_malloc(&f->d_out, view + 64));
        HAST_HIP_TRY(pinned_malloc(&f->h_rb, sizeof(RbState)));
    }
    if (mode == 1 && !f->h_out) HAST_HIP_TRY(pinned_malloc(&f->h_out, view));
    if (mode == 2 && !f->d_gz) {
        f->gz_cap = (size_t)dz::max_out_bytes(view);
        HAST_HIP_TRY(dz::slot_alloc(&f->enc, dz::max_pieces(view)));
        HAST_HIP_TRY(pinned_malloc(&f->h_gz, f->gz_cap));
        HAST_HIP_TRY(pinned_malloc(&f->h_dzres, sizeof(dz::Result)));
        HAST_HIP_TRY(dev_malloc(&f->d_gz, f->gz_cap));
    }
    return HAST_OK;
}

hast_status hast_rs_set_bins(hast_rs *f, int mode, uint32_t total0, uint32_t total1) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (mode < 0 || mode > 2) return set_error(HAST_ERR_INVALID, "hast_rs_set_bins: mode %d", mode);
    if (f->in.plan.waiting()) return set_error(HAST_ERR_INVALID, "hast_rs_set_bins: a submitted block waits for hast_rs_next");
    HAST_HIP_TRY(hipSetDevice(f->in.device));
    if (mode)
        if (hast_status st = rb_alloc(f, mode)) return st;
    f->bin_mode = mode;
    f->bin_total[0] = total0;
    f->bin_total[1] = total1;
    return HAST_OK;
}

hast_status hast_rs_set_rows(hast_rs *f, int mode, uint32_t total0, uint32_t total1) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (mode < 0 || mode > 1) return set_error(HAST_ERR_INVALID, "hast_rs_set_rows: mode %d", mode);
    if (f->in.plan.waiting()) return set_error(HAST_ERR_INVALID, "hast_rs_set_rows: a submitted block waits for hast_rs_next");
    if (mode && (!total0 || !total1)) return set_error(HAST_ERR_INVALID, "hast_rs_set_rows: a set size of 0 (the rows of an empty set are the host's)");
    if (mode && f->bin_mode && (f->bin_total[0] != total0 || f->bin_total[1] != total1))
        return set_error(HAST_ERR_INVALID, "hast_rs_set_rows: set sizes %u, %u, the bins have %u, %u", total0, total1, f->bin_total[0], f->bin_total[1]);
    HAST_HIP_TRY(hipSetDevice(f->in.device));
    if (mode && !f->d_rr) {                          // the buffers of the rows, at the first switch-on
        f->rr_plan = rr_scratch_plan(f->plan.max_rec);
        f->rows_cap = rows_room(f->in.plan.block);
        HAST_HIP_TRY(dev_malloc(&f->d_rr, f->rr_plan.total));
        HAST_HIP_TRY(dev_malloc(&f->d_rows, f->rows_cap));
        HAST_HIP_TRY(pinned_malloc(&f->h_rows, f->rows_cap));
        HAST_HIP_TRY(pinned_malloc(&f->h_rr, sizeof(RrState)));
    }
    f->row_mode = mode;
    f->row_total[0] = total0;
    f->row_total[1] = total1;
    return HAST_OK;
}

static hast_status rs_next(hast_rs *f, hast_rs_block *out, hast_rs_binned *bins, hast_rs_rows *rows);

hast_status hast_rs_next(hast_rs *f, hast_rs_block *out) { return rs_next(f, out, nullptr, nullptr); }

hast_status hast_rs_next_binned(hast_rs *f, hast_rs_block *out, hast_rs_binned *bins) {
    if (!bins) return set_error(HAST_ERR_INVALID, "null argument");
    *bins = hast_rs_binned{};
    return rs_next(f, out, bins, nullptr);
}

hast_status hast_rs_next_rows(hast_rs *f, hast_rs_block *out, hast_rs_binned *bins, hast_rs_rows *rows) {
    if (!rows) return set_error(HAST_ERR_INVALID, "null argument");
    *rows = hast_rs_rows{};
    if (bins) *bins = hast_rs_binned{};
    return rs_next(f, out, bins, rows);
}

hast_status hast_rs_rows_device(hast_ctx *ctx, const uint8_t *d_names, const uint32_t *d_name_off, const uint32_t *d_votes, size_t n, uint32_t total0,
                                uint32_t total1, uint8_t *d_out, size_t cap, uint64_t *bytes, uint64_t count[3]) {
    if (!ctx || !bytes || !count) return set_error(HAST_ERR_INVALID, "null argument");
    *bytes = 0;
    count[0] = count[1] = count[2] = 0;
    if (!total0 || !total1) return set_error(HAST_ERR_INVALID, "hast_rs_rows_device: a set size of 0");
    if (n >= (1ull << 32) - 1) return set_error(HAST_ERR_INVALID, "hast_rs_rows_device: %zu reads", n);
    if (!n) return HAST_OK;
    if (!d_names || !d_name_off || !d_votes || (cap && !d_out)) return set_error(HAST_ERR_INVALID, "null argument");
    HAST_HIP_TRY(hipSetDevice(ctx_device_of(ctx)));
    hipStream_t stream = ctx_stream_of(ctx);
    const RrScratchPlan plan = rr_scratch_plan(n);
    uint8_t *d_rr = nullptr;
    HAST_HIP_TRY(dev_malloc(&d_rr, plan.total));
    RrState st{};
    hipError_t e = launch_rr_rows(d_names, d_name_off, d_votes, n, total0, total1, d_rr, plan, d_out, cap, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&st, d_rr + plan.state, sizeof(RrState), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    park_device(d_rr, plan.total, 3);
    HAST_HIP_TRY(e);
    *bytes = st.total;
    if (!st.written) return set_error(HAST_ERR_UNSUPPORTED, "hast_rs_rows_device: the rows need %llu bytes, the output has room for %zu", (unsigned long long)st.total, cap);
    for (int c = 0; c < 3; ++c) count[c] = st.count[c];
    return HAST_OK;
}

static hast_status rs_next(hast_rs *f, hast_rs_block *out, hast_rs_binned *bins, hast_rs_rows *rows) {
    if (!f || !out) return set_error(HAST_ERR_INVALID, "null argument");
    if (hast_status st = f->in.wait_step()) return st;
    carry::Plan &p = f->in.plan;
    hipStream_t stream = f->in.stream;
    const bool last = f->is_last[p.step_slot()], fastq = f->format == HAST_RS_FASTQ;
    if (f->given_up) {                               // a block of this file was refused: up to its last block nothing is framed
        *out = hast_rs_block{};
        out->flags = f->given_up;
        p.done();
        if (last) f->given_up = 0;
        return HAST_OK;
    }
    if (f->file_done) {                              // the tail of the file before was not asked for
        p.drop_tail();
        f->file_done = false;
    }
    const carry::View v = p.view();
    const uint8_t *d_in = f->in.d_in[v.slot];
    HAST_HIP_TRY(launch_rs_frame(f->format, d_in, v.off, v.bytes, last, f->seen_header, f->d_seq, f->d_names, f->d_scratch, f->plan, stream));
    HAST_HIP_TRY(hipMemcpyAsync(f->h_st, f->d_scratch + f->plan.state, sizeof(RsState), hipMemcpyDeviceToHost, stream));
    HAST_HIP_TRY(hipStreamSynchronize(stream));
    const RsState s = *f->h_st;
    *out = hast_rs_block{};
    out->consumed = s.consumed;
    out->flags = s.flags;
    p.done();
    f->seen_header = !last && (f->seen_header || s.n_hdr > 0);
    const size_t left = v.bytes - (size_t)s.consumed;
    if (!(s.flags & RS_FORMAT_ERROR) && !p.fits(left)) out->flags |= HAST_RS_RECORD_TOO_LONG;
    if (out->flags) {                                // nothing classified, nothing carried: the caller gives this file up
        p.drop_tail();
        f->seen_header = false;
        if (!last) f->given_up = out->flags;
        return HAST_OK;
    }
    const size_t n_rec = (size_t)s.records;
    if (n_rec > f->plan.max_rec) return set_error(HAST_ERR_INVALID,"hast_rs_next: %zu records, scratch for %zu", n_rec, f->plan.max_rec);
    if (hast_status st = rs_grow(f, n_rec, (size_t)s.name_bytes)) return st;
    uint32_t *d_votes = reinterpret_cast<uint32_t *>(f->d_scratch + f->plan.votes);
    const uint32_t *d_name_off = reinterpret_cast<const uint32_t *>(f->d_scratch + f->plan.name_off);
    const bool rowed = rows && f->row_mode;          // names and votes stay where they are, unless the rows turn out not to fit
    auto download_block = [&]() -> hast_status {
        if (n_rec) {
            HAST_HIP_TRY(hipMemcpyAsync(f->h_votes, d_votes, n_rec * 8, hipMemcpyDeviceToHost, stream));
            if (s.name_bytes) HAST_HIP_TRY(hipMemcpyAsync(f->h_names, f->d_names, (size_t)s.name_bytes, hipMemcpyDeviceToHost, stream));
        }
        HAST_HIP_TRY(hipMemcpyAsync(f->h_name_off, d_name_off, (n_rec + 1) * 4, hipMemcpyDeviceToHost, stream));
        return HAST_OK;
    };
    if (n_rec) {
        const uint64_t *d_off = reinterpret_cast<const uint64_t *>(f->d_scratch + f->plan.off);
        const uint32_t *d_len = reinterpret_cast<const uint32_t *>(f->d_scratch + f->plan.len);
        const uint8_t *d_buf = fastq ? d_in : f->d_seq;
        const size_t buf_bytes = fastq ? v.off + v.bytes : (size_t)s.bases;
        if (hast_status st = classify_framed_perread(f->ctx, d_buf, buf_bytes, d_off, d_len, d_votes, n_rec, stream)) return st;
    }
    if (!rowed)
        if (hast_status st = download_block()) return st;
    if (hast_status st = f->in.carry(v, left, (size_t)s.consumed)) return st;
    if (rowed) {                                     // behind the classification: names and votes are read where they lie
        HAST_HIP_TRY(launch_rr_rows(f->d_names, d_name_off, d_votes, n_rec, f->row_total[0], f->row_total[1], f->d_rr, f->rr_plan, f->d_rows, f->rows_cap, stream));
        HAST_HIP_TRY(hipMemcpyAsync(f->h_rr, f->d_rr + f->rr_plan.state, sizeof(RrState), hipMemcpyDeviceToHost, stream));
    }
    const bool binned = bins && f->bin_mode && n_rec;
    if (binned) {                                    // behind the classification: the votes are read where they lie
        HAST_HIP_TRY(launch_rb_bin(f->format, d_in, v.off, v.bytes, f->bin_total[0], f->bin_total[1], f->d_scratch, f->plan, f->d_rb, f->rb_plan, f->d_out, stream));
        const RbState *d_state = reinterpret_cast<const RbState *>(f->d_rb + f->rb_plan.state);
        HAST_HIP_TRY(hipMemcpyAsync(f->h_rb, d_state, sizeof(RbState), hipMemcpyDeviceToHost, stream));
        if (f->bin_mode == 2) {
            HAST_HIP_TRY(dz::launch_job_from_bins(f->enc.job(), d_state->raw_bytes, stream));
            HAST_HIP_TRY(dz::launch_compress(f->enc.job(), f->d_out, f->enc.max_pieces, f->enc.d_work, f->d_gz, f->gz_cap, f->enc.res(), 0, stream));
            HAST_HIP_TRY(hipMemcpyAsync(f->h_dzres, f->enc.res(), sizeof(dz::Result), hipMemcpyDeviceToHost, stream));
        }
    }
    if (hast_status st = framed_err(f->ctx, stream)) return st;              // (waits for the stream)
    bool rows_on_host = false;
    if (rowed) {                                     // the size is known now: the text comes down, or, if it did not fit, names and votes as ever
        const RrState r = *f->h_rr;
        if (r.count[0] + r.count[1] + r.count[2] != n_rec || (r.written && r.total > f->rows_cap)) return set_error(HAST_ERR_INVALID, "hast_rs_next_rows: the rows do not add up");
        rows_on_host = !r.written;
        if (rows_on_host) {
            if (hast_status st = download_block()) return st;
        } else if (r.total) {
            HAST_HIP_TRY(hipMemcpyAsync(f->h_rows, f->d_rows, (size_t)r.total, hipMemcpyDeviceToHost, stream));
        }
        rows->on_host = rows_on_host;
        rows->text = rows_on_host ? nullptr : f->h_rows;
        rows->bytes = rows_on_host ? 0 : r.total;
        for (int c = 0; c < 3; ++c) rows->count[c] = r.count[c];
        if (!binned) HAST_HIP_TRY(hipStreamSynchronize(stream));
    }
    if (binned) {                                    // the sizes are known now: the runs (or their members) come down, and are waited for
        const RbState b = *f->h_rb;
        if (b.total > v.bytes || b.count[0] + b.count[1] + b.count[2] != n_rec) return set_error(HAST_ERR_INVALID, "hast_rs_next_binned: the runs do not add up");
        if (f->bin_mode == 1) {
            uint64_t at = 0;
            if (b.total) HAST_HIP_TRY(hipMemcpyAsync(f->h_out, f->d_out, (size_t)b.total, hipMemcpyDeviceToHost, stream));
            for (int c = 0; c < 3; ++c) {
                bins->run[c] = f->h_out + at;
                bins->run_bytes[c] = b.raw_bytes[c];
                at += b.raw_bytes[c];
            }
        } else {
            const dz::Result zr = *f->h_dzres;
            uint64_t total = 0, off[dz::kMaxRuns];
            if (zr.flags) return set_error(HAST_ERR_INVALID, "hast_rs_next_binned: the compressed runs do not fit (flags %u)", zr.flags);
            if (dz::member_layout(zr, 3, f->gz_cap, off, &total)) return set_error(HAST_ERR_INVALID, "the compressed runs are not where they should be");
            for (int c = 0; c < 3; ++c) {
                bins->run[c] = f->h_gz + off[c];             // (an empty run's too)
                bins->run_bytes[c] = zr.out_bytes[c];
            }
            if (total) HAST_HIP_TRY(hipMemcpyAsync(f->h_gz, f->d_gz, (size_t)total, hipMemcpyDeviceToHost, stream));
        }
        for (int c = 0; c < 3; ++c) {
            bins->raw_bytes[c] = b.raw_bytes[c];
            bins->count[c] = b.count[c];
        }
        HAST_HIP_TRY(hipStreamSynchronize(stream));
    }
    f->file_done = last && left;                     // FASTQ only: a FASTA file's last view consumes everything
    out->records = n_rec;
    out->bases = s.bases;
    out->name_bytes = s.name_bytes;
    if (!rowed || rows_on_host) {
        out->votes = f->h_votes;
        out->name_off = f->h_name_off;
        out->names = f->h_names;
    }
    return HAST_OK;
}

hast_status hast_rs_take_tail(hast_rs *f, uint8_t *dst, size_t *n_bytes) {
    if (!f) return set_error(HAST_ERR_INVALID, "null argument");
    if (hast_status st = f->in.take_tail(dst, n_bytes)) return st;
    f->file_done = false;
    f->seen_header = false;
    return HAST_OK;
}

void hast_rs_destroy(hast_rs *f) {
    if (!f) return;
    // (parked, not freed: a free stops every stream of the device, hast_internal.h; hast_ctx_destroy frees what is parked)
    f->in.release(true);
    const size_t block = f->in.plan.block;
    for (uint8_t *d : {f->d_seq, f->d_names, f->d_out}) park_device(d, carry::room_of(block), 3);
    park_device(f->d_scratch, f->plan.total, 3);
    park_pinned(f->h_st, sizeof(RsState), 3);
    park_pinned(f->h_votes, f->cap_rec * 8, 3);
    park_pinned(f->h_name_off, f->cap_rec * 4, 3);
    park_pinned(f->h_names, f->cap_names, 3);
    park_device(f->d_rb, f->rb_plan.total, 3);
    park_pinned(f->h_out, 2 * block, 3);
    park_pinned(f->h_rb, sizeof(RbState), 3);
    park_device(f->d_gz, f->gz_cap, 3);
    park_pinned(f->h_gz, f->gz_cap, 3);
    dz::slot_release(&f->enc, true);
    park_pinned(f->h_dzres, sizeof(dz::Result), 3);
    park_device(f->d_rr, f->rr_plan.total, 3);
    park_device(f->d_rows, f->rows_cap, 3);
    park_pinned(f->h_rows, f->rows_cap, 3);
    park_pinned(f->h_rr, sizeof(RrState), 3);
    delete f;
}

}  // extern "C"
