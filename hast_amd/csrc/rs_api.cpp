// rs_api.cpp -- the part of the C ABI behind `classify_read --ingest device` (include/hast.h "stage 03 ingest on the device"): raw
// FASTA / FASTQ bytes in HBM are framed into reads (rs_kernels.hip, rules: rs_core.h) and classified per read where they lie.
#include <hip/hip_runtime.h>

#include <new>

#include "dz_device.h"
#include "hast_internal.h"
#include "rs_device.h"

using namespace hast;

static_assert(HAST_RS_FASTA == RS_FASTA && HAST_RS_FASTQ == RS_FASTQ, "hast.h and rs_core.h name the same formats");
static_assert(HAST_RS_FORMAT_ERROR == RS_FORMAT_ERROR && HAST_RS_RECORD_TOO_LONG == RS_RECORD_TOO_LONG, "hast.h and rs_core.h name the same flags");

// Block n lies in d_in[n & 1] as [carried bytes | new bytes], the new bytes always at offset `block`, what block n-1 left unframed
// right in front of them (the layout of hast_sq_feed): the upload of block n+1 does not have to know how much block n leaves.
struct hast_rs {
    hast_ctx *ctx = nullptr;
    int device = 0, format = 0;
    size_t block = 0;
    hipStream_t stream = nullptr, up_stream = nullptr;       // the context's: framing and classification; ours: uploads
    RsScratchPlan plan;
    uint8_t *d_in[2] = {nullptr, nullptr}, *h_in[2] = {nullptr, nullptr};
    uint8_t *d_seq = nullptr, *d_names = nullptr, *d_scratch = nullptr;
    RsState *h_st = nullptr;                                 // pinned
    uint32_t *h_votes = nullptr, *h_name_off = nullptr;      // pinned, grown to the largest block so far
    uint8_t *h_names = nullptr;
    size_t cap_rec = 0, cap_names = 0;
    hipEvent_t up_ev[2] = {nullptr, nullptr};
    bool up_pending[2] = {false, false}, on_device[2] = {false, false}, is_last[2] = {false, false};
    size_t n_new[2] = {0, 0};
    int handed = 0;                                          // what the caller holds: 0 nothing, 1 a host block, 2 a device block
    uint64_t n_submitted = 0, n_done = 0;
    size_t tail = 0;                                         // bytes carried in front of block n_done's new bytes
    bool seen_header = false;                                // FASTA: a header line has been framed in this file
    bool file_done = false;                                  // FASTQ: the tail is a finished file's (hast_rs_take_tail)
    uint32_t given_up = 0;                                   // the flags that ended this file: its other blocks are not looked at
    // the read bins (hast_rs_set_bins): nothing of this is allocated before they are first switched on
    int bin_mode = 0;                                        // 0 off, 1 plain, 2 gzip
    uint32_t bin_total[2] = {0, 0};
    RbScratchPlan rb_plan{};
    uint8_t *d_rb = nullptr, *d_out = nullptr, *h_out = nullptr;       // per-record arrays; the three runs of a view, device and pinned
    RbState *h_rb = nullptr;                                 // pinned
    uint8_t *d_gz = nullptr, *h_gz = nullptr, *d_dzwork = nullptr;     // gzip: the members, device and pinned; the encoder's workspace, job and result
    dz::Job *d_dzjob = nullptr;
    dz::Result *d_dzres = nullptr, *h_dzres = nullptr;
    size_t gz_cap = 0, dzwork_bytes = 0;
    uint32_t dz_pieces = 0;
};

extern "C" {

hast_status hast_rs_create(hast_ctx *ctx, int format, size_t block_bytes, hast_rs **out) {
    if (!ctx || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (format != HAST_RS_FASTA && format != HAST_RS_FASTQ) return set_error(HAST_ERR_INVALID, "hast_rs_create: format %d", format);
    if (block_bytes < 64 || block_bytes > (1ull << 30)) return set_error(HAST_ERR_INVALID, "hast_rs_create: blocks of %zu bytes (64 .. 2^30)", block_bytes);
    hast_rs *f = new (std::nothrow) hast_rs;
    if (!f) return set_error(HAST_ERR_OOM, "hast_rs_create");
    f->ctx = ctx;
    f->device = ctx_device_of(ctx);
    f->format = format;
    f->block = block_bytes;
    f->stream = ctx_stream_of(ctx);
    f->plan = rs_scratch_plan(format, 2 * block_bytes);
    hipError_t e = hipSetDevice(f->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->up_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = dev_malloc(&f->d_scratch, f->plan.total);
    if (e == hipSuccess) e = dev_malloc(&f->d_names, 2 * block_bytes + 64);
    if (e == hipSuccess && format == HAST_RS_FASTA) e = dev_malloc(&f->d_seq, 2 * block_bytes + 64);
    if (e == hipSuccess) e = pinned_malloc(&f->h_st, sizeof(RsState));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = dev_malloc(&f->d_in[i], 2 * block_bytes + 64);                      // (the classifier may read a few bytes behind a read: the pad)
        if (e == hipSuccess) e = pinned_malloc(&f->h_in[i], block_bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->up_ev[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        const size_t total = f->plan.total;
        hast_rs_destroy(f);
        return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_rs_create: blocks of %zu bytes, %zu of scratch: %s", block_bytes, total,
                         hipGetErrorString(e));
    }
    *out = f;
    return HAST_OK;
}

static hast_status rs_slot(hast_rs *f, int *slot) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (f->n_submitted - f->n_done >= 2) return set_error(HAST_ERR_INVALID, "hast_rs: two blocks are waiting for hast_rs_next");
    *slot = (int)(f->n_submitted & 1);
    HAST_HIP_TRY(hipSetDevice(f->device));
    return HAST_OK;
}

hast_status hast_rs_host_block(hast_rs *f, uint8_t **h_buf) {
    int slot;
    if (hast_status st = rs_slot(f, &slot)) return st;
    if (!h_buf) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->up_pending[slot]) {                       // the upload out of this staging block, two blocks ago
        HAST_HIP_TRY(hipEventSynchronize(f->up_ev[slot]));
        f->up_pending[slot] = false;
    }
    f->handed = 1;
    *h_buf = f->h_in[slot];
    return HAST_OK;
}

hast_status hast_rs_device_block(hast_rs *f, uint8_t **d_buf, hast_stream *fill) {
    int slot;
    if (hast_status st = rs_slot(f, &slot)) return st;
    if (!d_buf) return set_error(HAST_ERR_INVALID, "null argument");
    f->handed = 2;
    *d_buf = f->d_in[slot] + f->block;               // (written on the context's stream: behind everything that still reads this buffer)
    if (fill) *fill = f->stream;
    return HAST_OK;
}

hast_status hast_rs_submit(hast_rs *f, size_t n_bytes, int last) {
    int slot;
    if (hast_status st = rs_slot(f, &slot)) return st;
    if (!f->handed || n_bytes > f->block || (n_bytes < 1 && !last))
        return set_error(HAST_ERR_INVALID, "hast_rs_submit: %zu bytes of a block of %zu", n_bytes, f->block);
    f->on_device[slot] = f->handed == 2 || n_bytes == 0;
    if (!f->on_device[slot]) {
        // (this buffer held block n-2, framed, classified and waited for by its hast_rs_next)
        HAST_HIP_TRY(hipMemcpyAsync(f->d_in[slot] + f->block, f->h_in[slot], n_bytes, hipMemcpyHostToDevice, f->up_stream));
        HAST_HIP_TRY(hipEventRecord(f->up_ev[slot], f->up_stream));
        f->up_pending[slot] = true;
    }
    f->n_new[slot] = n_bytes;
    f->is_last[slot] = last != 0;
    f->handed = 0;
    ++f->n_submitted;
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
    const size_t view = 2 * f->block;
    if (!f->d_rb) {
        f->rb_plan = rb_scratch_plan(f->plan);
        HAST_HIP_TRY(dev_malloc(&f->d_rb, f->rb_plan.total));
        HAST_HIP_TRY(dev_malloc(&f->d_out, view + 64));
        HAST_HIP_TRY(pinned_malloc(&f->h_rb, sizeof(RbState)));
    }
    if (mode == 1 && !f->h_out) HAST_HIP_TRY(pinned_malloc(&f->h_out, view));
    if (mode == 2 && !f->d_gz) {
        f->dz_pieces = dz::max_pieces(view);
        f->gz_cap = (size_t)dz::max_out_bytes(view);
        const size_t work = (dz::workspace_bytes(f->dz_pieces) + 63) & ~(size_t)63;
        f->dzwork_bytes = work + sizeof(dz::Job) + sizeof(dz::Result);
        HAST_HIP_TRY(dev_malloc(&f->d_dzwork, f->dzwork_bytes));
        f->d_dzjob = reinterpret_cast<dz::Job *>(f->d_dzwork + work);
        f->d_dzres = reinterpret_cast<dz::Result *>(f->d_dzjob + 1);
        HAST_HIP_TRY(pinned_malloc(&f->h_gz, f->gz_cap));
        HAST_HIP_TRY(pinned_malloc(&f->h_dzres, sizeof(dz::Result)));
        HAST_HIP_TRY(dev_malloc(&f->d_gz, f->gz_cap));
    }
    return HAST_OK;
}

hast_status hast_rs_set_bins(hast_rs *f, int mode, uint32_t total0, uint32_t total1) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (mode < 0 || mode > 2) return set_error(HAST_ERR_INVALID, "hast_rs_set_bins: mode %d", mode);
    if (f->n_submitted != f->n_done) return set_error(HAST_ERR_INVALID, "hast_rs_set_bins: a submitted block waits for hast_rs_next");
    HAST_HIP_TRY(hipSetDevice(f->device));
    if (mode)
        if (hast_status st = rb_alloc(f, mode)) return st;
    f->bin_mode = mode;
    f->bin_total[0] = total0;
    f->bin_total[1] = total1;
    return HAST_OK;
}

static hast_status rs_next(hast_rs *f, hast_rs_block *out, hast_rs_binned *bins);

hast_status hast_rs_next(hast_rs *f, hast_rs_block *out) { return rs_next(f, out, nullptr); }

hast_status hast_rs_next_binned(hast_rs *f, hast_rs_block *out, hast_rs_binned *bins) {
    if (!bins) return set_error(HAST_ERR_INVALID, "null argument");
    *bins = hast_rs_binned{};
    return rs_next(f, out, bins);
}

static hast_status rs_next(hast_rs *f, hast_rs_block *out, hast_rs_binned *bins) {
    if (!f || !out) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->n_done == f->n_submitted) return set_error(HAST_ERR_INVALID, "hast_rs_next: no block submitted");
    const int slot = (int)(f->n_done & 1);
    const bool last = f->is_last[slot], fastq = f->format == HAST_RS_FASTQ;
    HAST_HIP_TRY(hipSetDevice(f->device));
    if (!f->on_device[slot]) HAST_HIP_TRY(hipStreamWaitEvent(f->stream, f->up_ev[slot], 0));
    if (f->given_up) {                               // a block of this file was refused: up to its last block nothing is framed
        *out = hast_rs_block{};
        out->flags = f->given_up;
        ++f->n_done;
        if (last) f->given_up = 0;
        return HAST_OK;
    }
    if (f->file_done) {                              // the tail of the file before was not asked for
        f->tail = 0;
        f->file_done = false;
    }
    const size_t origin = f->block - f->tail, n = f->tail + f->n_new[slot];
    HAST_HIP_TRY(launch_rs_frame(f->format, f->d_in[slot], origin, n, last, f->seen_header, f->d_seq, f->d_names, f->d_scratch, f->plan, f->stream));
    HAST_HIP_TRY(hipMemcpyAsync(f->h_st, f->d_scratch + f->plan.state, sizeof(RsState), hipMemcpyDeviceToHost, f->stream));
    HAST_HIP_TRY(hipStreamSynchronize(f->stream));
    const RsState s = *f->h_st;
    *out = hast_rs_block{};
    out->consumed = s.consumed;
    out->flags = s.flags;
    ++f->n_done;
    f->seen_header = !last && (f->seen_header || s.n_hdr > 0);
    const size_t left = n - (size_t)s.consumed;
    if (!(s.flags & RS_FORMAT_ERROR) && left > f->block) out->flags |= HAST_RS_RECORD_TOO_LONG;
    if (out->flags) {                                // nothing classified, nothing carried: the caller gives this file up
        f->tail = 0;
        f->seen_header = false;
        if (!last) f->given_up = out->flags;
        return HAST_OK;
    }
    const size_t n_rec = (size_t)s.records;
    if (n_rec > f->plan.max_rec) return set_error(HAST_ERR_INVALID,"hast_rs_next: %zu records, scratch for %zu", n_rec, f->plan.max_rec);
    if (hast_status st = rs_grow(f, n_rec, (size_t)s.name_bytes)) return st;
    uint32_t *d_votes = reinterpret_cast<uint32_t *>(f->d_scratch + f->plan.votes);
    if (n_rec) {
        const uint64_t *d_off = reinterpret_cast<const uint64_t *>(f->d_scratch + f->plan.off);
        const uint32_t *d_len = reinterpret_cast<const uint32_t *>(f->d_scratch + f->plan.len);
        const uint8_t *d_buf = fastq ? f->d_in[slot] : f->d_seq;
        const size_t buf_bytes = fastq ? f->block + f->n_new[slot] : (size_t)s.bases;
        if (hast_status st = classify_framed_perread(f->ctx, d_buf, buf_bytes, d_off, d_len, d_votes, n_rec, f->stream)) return st;
        HAST_HIP_TRY(hipMemcpyAsync(f->h_votes, d_votes, n_rec * 8, hipMemcpyDeviceToHost, f->stream));
        if (s.name_bytes) HAST_HIP_TRY(hipMemcpyAsync(f->h_names, f->d_names, (size_t)s.name_bytes, hipMemcpyDeviceToHost, f->stream));
    }
    HAST_HIP_TRY(hipMemcpyAsync(f->h_name_off, f->d_scratch + f->plan.name_off, (n_rec + 1) * 4, hipMemcpyDeviceToHost, f->stream));
    if (left) HAST_HIP_TRY(hipMemcpyAsync(f->d_in[slot ^ 1] + f->block - left, f->d_in[slot] + origin + s.consumed, left, hipMemcpyDeviceToDevice, f->stream));
    const bool binned = bins && f->bin_mode && n_rec;
    if (binned) {                                    // behind the classification: the votes are read where they lie
        HAST_HIP_TRY(launch_rb_bin(f->format, f->d_in[slot], origin, n, f->bin_total[0], f->bin_total[1], f->d_scratch, f->plan, f->d_rb, f->rb_plan, f->d_out,
                                   f->stream));
        const RbState *d_state = reinterpret_cast<const RbState *>(f->d_rb + f->rb_plan.state);
        HAST_HIP_TRY(hipMemcpyAsync(f->h_rb, d_state, sizeof(RbState), hipMemcpyDeviceToHost, f->stream));
        if (f->bin_mode == 2) {
            HAST_HIP_TRY(dz::launch_job_from_bins(f->d_dzjob, d_state->raw_bytes, f->stream));
            HAST_HIP_TRY(dz::launch_compress(f->d_dzjob, f->d_out, f->dz_pieces, f->d_dzwork, f->d_gz, f->gz_cap, f->d_dzres, 0, f->stream));
            HAST_HIP_TRY(hipMemcpyAsync(f->h_dzres, f->d_dzres, sizeof(dz::Result), hipMemcpyDeviceToHost, f->stream));
        }
    }
    if (hast_status st = framed_err(f->ctx, f->stream)) return st;           // (waits for the stream)
    if (binned) {                                    // the sizes are known now: the runs (or their members) come down, and are waited for
        const RbState b = *f->h_rb;
        if (b.total > n || b.count[0] + b.count[1] + b.count[2] != n_rec) return set_error(HAST_ERR_INVALID, "hast_rs_next_binned: the runs do not add up");
        uint64_t at = 0;
        if (f->bin_mode == 1) {
            if (b.total) HAST_HIP_TRY(hipMemcpyAsync(f->h_out, f->d_out, (size_t)b.total, hipMemcpyDeviceToHost, f->stream));
            for (int c = 0; c < 3; ++c) {
                bins->run[c] = f->h_out + at;
                bins->run_bytes[c] = b.raw_bytes[c];
                at += b.raw_bytes[c];
            }
        } else {
            const dz::Result zr = *f->h_dzres;
            if (zr.flags) return set_error(HAST_ERR_INVALID, "hast_rs_next_binned: the compressed runs do not fit (flags %u)", zr.flags);
            for (int c = 0; c < 3; ++c) {
                if (!zr.out_bytes[c]) {
                    bins->run[c] = f->h_gz + at;
                    continue;
                }
                if (zr.member_off[c] != at || at + zr.out_bytes[c] > f->gz_cap) return set_error(HAST_ERR_INVALID, "the compressed runs are not where they should be");
                bins->run[c] = f->h_gz + at;
                bins->run_bytes[c] = zr.out_bytes[c];
                at += zr.out_bytes[c];
            }
            if (at) HAST_HIP_TRY(hipMemcpyAsync(f->h_gz, f->d_gz, (size_t)at, hipMemcpyDeviceToHost, f->stream));
        }
        for (int c = 0; c < 3; ++c) {
            bins->raw_bytes[c] = b.raw_bytes[c];
            bins->count[c] = b.count[c];
        }
        HAST_HIP_TRY(hipStreamSynchronize(f->stream));
    }
    f->tail = left;
    f->file_done = last && left;                     // FASTQ only: a FASTA file's last view consumes everything
    out->records = n_rec;
    out->bases = s.bases;
    out->name_bytes = s.name_bytes;
    out->votes = f->h_votes;
    out->name_off = f->h_name_off;
    out->names = f->h_names;
    return HAST_OK;
}

hast_status hast_rs_take_tail(hast_rs *f, uint8_t *dst, size_t *n_bytes) {
    if (!f || !dst || !n_bytes) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->n_done != f->n_submitted) return set_error(HAST_ERR_INVALID, "hast_rs_take_tail: a submitted block has not been framed");
    HAST_HIP_TRY(hipSetDevice(f->device));
    *n_bytes = f->tail;
    if (f->tail) {
        HAST_HIP_TRY(hipMemcpyAsync(dst, f->d_in[f->n_done & 1] + f->block - f->tail, f->tail, hipMemcpyDeviceToHost, f->stream));
        HAST_HIP_TRY(hipStreamSynchronize(f->stream));
    }
    f->tail = 0;
    f->file_done = false;
    f->seen_header = false;
    return HAST_OK;
}

void hast_rs_destroy(hast_rs *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->up_stream) (void)hipStreamSynchronize(f->up_stream);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    // (parked, not freed: a free stops every stream of the device, hast_internal.h; hast_ctx_destroy frees what is parked)
    for (int i = 0; i < 2; ++i) {
        park_device(f->d_in[i], 2 * f->block + 64, 3);
        park_pinned(f->h_in[i], f->block, 3);
        if (f->up_ev[i]) (void)hipEventDestroy(f->up_ev[i]);
    }
    park_device(f->d_seq, 2 * f->block + 64, 3);
    park_device(f->d_names, 2 * f->block + 64, 3);
    park_device(f->d_scratch, f->plan.total, 3);
    park_pinned(f->h_st, sizeof(RsState), 3);
    park_pinned(f->h_votes, f->cap_rec * 8, 3);
    park_pinned(f->h_name_off, f->cap_rec * 4, 3);
    park_pinned(f->h_names, f->cap_names, 3);
    park_device(f->d_rb, f->rb_plan.total, 3);
    park_device(f->d_out, 2 * f->block + 64, 3);
    park_pinned(f->h_out, 2 * f->block, 3);
    park_pinned(f->h_rb, sizeof(RbState), 3);
    park_device(f->d_gz, f->gz_cap, 3);
    park_pinned(f->h_gz, f->gz_cap, 3);
    park_device(f->d_dzwork, f->dzwork_bytes, 3);
    park_pinned(f->h_dzres, sizeof(dz::Result), 3);
    if (f->up_stream) (void)hipStreamDestroy(f->up_stream);
    delete f;
}

}  // extern "C"
