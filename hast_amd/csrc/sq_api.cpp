// sq_api.cpp -- the part of the C ABI that frames raw four-line FASTQ, or FASTA, in device memory into the k-mer counter's base stream
// (include/hast.h "stage 00 ingest on the device"; the kernels are sq_kernels.hip and sq_fasta_kernels.hip, the rules sq_core.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "hast_internal.h"
#include "sq_device.h"

using namespace hast;

static_assert(HAST_SQ_NOT_FOUR_LINE == SQ_NOT_FOUR_LINE && HAST_SQ_NO_RECORD == SQ_NO_RECORD, "hast.h and sq_core.h name the same flags");
static_assert(sizeof(hast_sq_result) == 40 && sizeof(hast_sq_result) <= sizeof(SqState), "hast_sq_result is the head of SqState");
static_assert(HAST_SQ_FA_OPEN == SQ_FA_OPEN && HAST_SQ_FA_LAST == SQ_FA_LAST, "hast.h and sq_core.h name the same flags");
static_assert(sizeof(hast_sq_result) <= sizeof(SqFaState), "hast_sq_result is the head of SqFaState");

struct hast_sq {
    int device = 0;
    hipStream_t stream = nullptr;            // the count table's: a framed block is counted behind its framing without an event
    size_t max_in = 0;
    SqScratchPlan plan;
    uint8_t *d_scratch = nullptr;
    SqState *h_st = nullptr;                 // pinned
    // FASTA: allocated at the first FASTA frame, so a framer that sees only FASTQ holds what it always held
    SqFaScratchPlan fa_plan;
    uint8_t *d_fa_scratch = nullptr;
    SqFaState *h_fa_st = nullptr;            // pinned
};

constexpr size_t kSqKeepPad = 64;            // room in front of a FASTA view's output for the kept bytes (K - 1 <= 31 of them)


// one input stream of `unshared_kmers --ingest device` (include/hast.h): block n lies in d_in[n & 1] as [kept bytes | new bytes], the
// new bytes always at offset `block`, what block n-1 left unframed right in front of them -- so the upload of block n+1 does not
// have to know how much block n leaves
struct hast_sq_feed {
    hast_kc *kc = nullptr;
    hast_sq *sq = nullptr;
    int device = 0;
    size_t block = 0;
    hipStream_t table_stream = nullptr, up_stream = nullptr;
    uint8_t *d_in[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr}, *h_in[2] = {nullptr, nullptr};
    hipEvent_t up_ev[2] = {nullptr, nullptr}, tail_ev = nullptr;
    bool up_pending[2] = {false, false}, tail_pending = false;
    size_t n_new[2] = {0, 0};
    bool on_device[2] = {false, false};
    int handed = 0;                          // what the caller holds: 0 nothing, 1 a host block, 2 a device block
    uint64_t n_submitted = 0, n_done = 0;
    size_t tail = 0;                         // bytes carried in front of block n_done's new bytes
    // FASTA (hast_sq_feed_set_formats): what the current input is, whether one of its headers has been seen, and how many of its last
    // emitted bytes lie in front of the next view's output, at d_out[n_done & 1] + kSqKeepPad - kept
    unsigned formats = HAST_SQ_TAKE_FASTQ;
    int format = 0;                          // 0 undecided, 1 FASTQ, 2 FASTA
    bool fa_open = false;
    size_t kept = 0, keep = 0;               // keep = K - 1
};

extern "C" {

hast_status hast_sq_create(hast_kc *kc, size_t max_in_bytes, hast_sq **out) {
    if (!kc || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (max_in_bytes < 1 || max_in_bytes >= (1ull << 32) - 2 * kNlTile)
        return set_error(HAST_ERR_INVALID, "hast_sq_create: %zu bytes a block; offsets inside a block are 32 bits wide", max_in_bytes);
    hast_sq *q = new (std::nothrow) hast_sq;
    if (!q) return set_error(HAST_ERR_OOM, "hast_sq_create");
    q->device = kc_device_of(kc);
    q->stream = static_cast<hipStream_t>(hast_kc_stream(kc));
    q->max_in = max_in_bytes;
    q->plan = sq_scratch_plan(max_in_bytes);
    hipError_t e = hipSetDevice(q->device);
    if (e == hipSuccess) e = dev_malloc(&q->d_scratch, q->plan.total);
    if (e == hipSuccess) e = pinned_malloc(&q->h_st, sizeof(SqState));
    if (e != hipSuccess) {
        const size_t total = q->plan.total;
        hast_sq_destroy(q);
        return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_sq_create: %zu bytes of scratch: %s", total, hipGetErrorString(e));
    }
    *out = q;
    return HAST_OK;
}

hast_status hast_sq_frame_device(hast_sq *q, const uint8_t *d_in, size_t n_in, uint8_t *d_out, size_t cap_out, hast_sq_result *res) {
    if (!q || !res || (n_in && (!d_in || !d_out))) return set_error(HAST_ERR_INVALID, "null argument");
    if (n_in > q->max_in) return set_error(HAST_ERR_INVALID, "hast_sq_frame_device: %zu bytes, the framer was created for %zu", n_in, q->max_in);
    if (cap_out < n_in) return set_error(HAST_ERR_INVALID, "hast_sq_frame_device: %zu bytes of room for a block of %zu", cap_out, n_in);
    HAST_HIP_TRY(hipSetDevice(q->device));
    HAST_HIP_TRY(launch_sq_frame(d_in, n_in, d_out, q->d_scratch, q->plan, q->stream));
    HAST_HIP_TRY(hipMemcpyAsync(q->h_st, q->d_scratch + q->plan.state, sizeof(SqState), hipMemcpyDeviceToHost, q->stream));
    HAST_HIP_TRY(hipStreamSynchronize(q->stream));
    const SqState &s = *q->h_st;
    res->consumed = s.consumed;
    res->out_bytes = s.out_bytes;
    res->records = s.records;
    res->bases = s.bases;
    res->flags = s.flags;
    res->first_bad = s.first_bad;
    return HAST_OK;
}

hast_status hast_sq_frame_fasta_device(hast_sq *q, const uint8_t *d_in, size_t n_in, uint8_t *d_out, size_t cap_out, unsigned in_flags, hast_sq_result *res) {
    if (!q || !res || (n_in && !d_in) || !d_out) return set_error(HAST_ERR_INVALID, "null argument");
    if (in_flags & ~(HAST_SQ_FA_OPEN | HAST_SQ_FA_LAST)) return set_error(HAST_ERR_INVALID, "hast_sq_frame_fasta_device: flags %#x", in_flags);
    if (n_in > q->max_in) return set_error(HAST_ERR_INVALID, "hast_sq_frame_fasta_device: %zu bytes, the framer was created for %zu", n_in, q->max_in);
    if (cap_out < n_in + 1) return set_error(HAST_ERR_INVALID, "hast_sq_frame_fasta_device: %zu bytes of room for a view of %zu and the closing byte", cap_out, n_in);
    HAST_HIP_TRY(hipSetDevice(q->device));
    if (!q->d_fa_scratch) {
        q->fa_plan = sq_fa_scratch_plan(q->max_in);
        hipError_t e = dev_malloc(&q->d_fa_scratch, q->fa_plan.total);
        if (e == hipSuccess && !q->h_fa_st) e = pinned_malloc(&q->h_fa_st, sizeof(SqFaState));
        if (e != hipSuccess) {
            if (q->d_fa_scratch) (void)hipFree(q->d_fa_scratch);
            q->d_fa_scratch = nullptr;
            return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_sq_frame_fasta_device: %zu bytes of scratch: %s", q->fa_plan.total,
                             hipGetErrorString(e));
        }
    }
    if (n_in == 0) {                         // no line: at most the closing byte
        *res = hast_sq_result{0, sqfa::closing(0, (in_flags & SQ_FA_OPEN) != 0, (in_flags & SQ_FA_LAST) != 0), 0, 0, 0, sq::kNoBad};
        if (res->out_bytes) HAST_HIP_TRY(hipMemsetAsync(d_out, '\n', 1, q->stream));
        HAST_HIP_TRY(hipStreamSynchronize(q->stream));
        return HAST_OK;
    }
    HAST_HIP_TRY(launch_sq_fasta_frame(d_in, n_in, d_out, in_flags, q->d_fa_scratch, q->fa_plan, q->stream));
    HAST_HIP_TRY(hipMemcpyAsync(q->h_fa_st, q->d_fa_scratch + q->fa_plan.state, sizeof(SqFaState), hipMemcpyDeviceToHost, q->stream));
    HAST_HIP_TRY(hipStreamSynchronize(q->stream));
    const SqFaState &s = *q->h_fa_st;
    res->consumed = s.consumed;
    res->out_bytes = s.out_bytes;
    res->records = s.records;
    res->bases = s.bases;
    res->flags = s.flags;
    res->first_bad = s.first_bad;
    return HAST_OK;
}

void hast_sq_destroy(hast_sq *q) {
    if (!q) return;
    (void)hipSetDevice(q->device);
    if (q->stream) (void)hipStreamSynchronize(q->stream);
    if (q->d_scratch) (void)hipFree(q->d_scratch);
    if (q->h_st) (void)hipHostFree(q->h_st);
    if (q->d_fa_scratch) (void)hipFree(q->d_fa_scratch);
    if (q->h_fa_st) (void)hipHostFree(q->h_fa_st);
    delete q;
}

hast_status hast_sq_feed_create(hast_kc *kc, size_t block_bytes, hast_sq_feed **out) {
    if (!kc || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (block_bytes < 64 || block_bytes > (1ull << 30)) return set_error(HAST_ERR_INVALID, "hast_sq_feed_create: blocks of %zu bytes (64 .. 2^30)", block_bytes);
    hast_sq_feed *f = new (std::nothrow) hast_sq_feed;
    if (!f) return set_error(HAST_ERR_OOM, "hast_sq_feed_create");
    f->kc = kc;
    f->device = kc_device_of(kc);
    f->block = block_bytes;
    f->keep = (size_t)kc_k_of(kc) - 1;
    f->table_stream = static_cast<hipStream_t>(hast_kc_stream(kc));
    hast_status st = hast_sq_create(kc, 2 * block_bytes, &f->sq);
    hipError_t e = hipSuccess;
    if (st == HAST_OK) {
        e = hipSetDevice(f->device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->up_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->tail_ev, hipEventDisableTiming);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            e = dev_malloc(&f->d_in[i], 2 * block_bytes + 64);
            if (e == hipSuccess) e = dev_malloc(&f->d_out[i], 2 * block_bytes + 64);      // (the counter reads nothing behind n_bytes; the pad is slack)
            if (e == hipSuccess) e = pinned_malloc(&f->h_in[i], block_bytes);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&f->up_ev[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) st = set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_sq_feed_create: %s", hipGetErrorString(e));
    }
    if (st != HAST_OK) {
        hast_sq_feed_destroy(f);
        return st;
    }
    *out = f;
    return HAST_OK;
}

static hast_status feed_slot(hast_sq_feed *f, int *slot) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (f->n_submitted - f->n_done >= 2) return set_error(HAST_ERR_INVALID, "hast_sq_feed: two blocks are waiting for hast_sq_feed_next");
    *slot = (int)(f->n_submitted & 1);
    HAST_HIP_TRY(hipSetDevice(f->device));
    return HAST_OK;
}

hast_status hast_sq_feed_host_block(hast_sq_feed *f, uint8_t **h_buf) {
    int slot;
    if (hast_status st = feed_slot(f, &slot)) return st;
    if (!h_buf) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->up_pending[slot]) {                       // the upload out of this staging block, two blocks ago
        HAST_HIP_TRY(hipEventSynchronize(f->up_ev[slot]));
        f->up_pending[slot] = false;
    }
    f->handed = 1;
    *h_buf = f->h_in[slot];
    return HAST_OK;
}

hast_status hast_sq_feed_device_block(hast_sq_feed *f, uint8_t **d_buf) {
    int slot;
    if (hast_status st = feed_slot(f, &slot)) return st;
    if (!d_buf) return set_error(HAST_ERR_INVALID, "null argument");
    f->handed = 2;
    *d_buf = f->d_in[slot] + f->block;               // (written on the table's stream: behind everything that still reads this buffer)
    return HAST_OK;
}

hast_status hast_sq_feed_submit(hast_sq_feed *f, size_t n_bytes) {
    int slot;
    if (hast_status st = feed_slot(f, &slot)) return st;
    if (!f->handed || n_bytes < 1 || n_bytes > f->block) return set_error(HAST_ERR_INVALID, "hast_sq_feed_submit: %zu bytes of a block of %zu", n_bytes, f->block);
    f->on_device[slot] = f->handed == 2;
    if (f->handed == 1) {
        // this buffer held block n-2: its framing has been waited for, the copy of what it left to block n-1 may still run
        if (f->tail_pending) HAST_HIP_TRY(hipStreamWaitEvent(f->up_stream, f->tail_ev, 0));
        HAST_HIP_TRY(hipMemcpyAsync(f->d_in[slot] + f->block, f->h_in[slot], n_bytes, hipMemcpyHostToDevice, f->up_stream));
        HAST_HIP_TRY(hipEventRecord(f->up_ev[slot], f->up_stream));
        f->up_pending[slot] = true;
    }
    f->n_new[slot] = n_bytes;
    f->handed = 0;
    ++f->n_submitted;
    return HAST_OK;
}

// One view of a FASTA input: framed behind the kept bytes, counted with them in front (K - 1 bytes hold no window, so no window is
// counted twice and none across the cut is lost: ChunkSink's rule), its last K - 1 emitted bytes put in front of the next view's output
// and [consumed, n) in front of the next view's input.
static hast_status feed_fasta_view(hast_sq_feed *f, int slot, int parent, const uint8_t *d_view, size_t n, bool last, hast_sq_result *res) {
    uint8_t *out = f->d_out[slot] + kSqKeepPad;
    const unsigned in_flags = (f->fa_open ? HAST_SQ_FA_OPEN : 0u) | (last ? HAST_SQ_FA_LAST : 0u);
    if (hast_status st = hast_sq_frame_fasta_device(f->sq, d_view, n, out, 2 * f->block + 64, in_flags, res)) return st;
    const size_t left = n - (size_t)res->consumed;
    if (left > f->block) {
        res->flags |= HAST_SQ_TAIL_TOO_LONG;
        return HAST_OK;
    }
    const size_t have = f->kept + (size_t)res->out_bytes;
    if (res->out_bytes && have > f->keep)
        if (hast_status st = hast_kc_count_device(f->kc, parent, out - f->kept, have)) return st;
    const size_t kept = std::min(f->keep, have);
    if (kept && !last)
        HAST_HIP_TRY(hipMemcpyAsync(f->d_out[slot ^ 1] + kSqKeepPad - kept, out + res->out_bytes - kept, kept, hipMemcpyDeviceToDevice, f->table_stream));
    if (left) HAST_HIP_TRY(hipMemcpyAsync(f->d_in[slot ^ 1] + f->block - left, d_view + res->consumed, left, hipMemcpyDeviceToDevice, f->table_stream));
    HAST_HIP_TRY(hipEventRecord(f->tail_ev, f->table_stream));
    f->tail_pending = true;
    f->tail = left;
    f->kept = kept;
    if (res->records) f->fa_open = true;
    return HAST_OK;
}

hast_status hast_sq_feed_set_formats(hast_sq_feed *f, unsigned mask) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (!(mask & HAST_SQ_TAKE_FASTQ) || (mask & ~(HAST_SQ_TAKE_FASTQ | HAST_SQ_TAKE_FASTA)))
        return set_error(HAST_ERR_INVALID, "hast_sq_feed_set_formats: mask %#x (FASTQ, or FASTQ and FASTA)", mask);
    if (f->n_submitted != f->n_done || f->handed || f->tail || f->format)
        return set_error(HAST_ERR_INVALID, "hast_sq_feed_set_formats: an input is on its way through the feed");
    if ((mask & HAST_SQ_TAKE_FASTA) && !(f->formats & HAST_SQ_TAKE_FASTA)) {
        // a FASTA view's output lies behind the kept bytes and may end with the closing byte: larger output buffers
        HAST_HIP_TRY(hipSetDevice(f->device));
        HAST_HIP_TRY(hipStreamSynchronize(f->table_stream));
        for (int i = 0; i < 2; ++i) {
            uint8_t *d = nullptr;
            const hipError_t e = dev_malloc(&d, 2 * f->block + 64 + 2 * kSqKeepPad);
            if (e != hipSuccess) return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_sq_feed_set_formats: %s", hipGetErrorString(e));
            (void)hipFree(f->d_out[i]);
            f->d_out[i] = d;
        }
    }
    f->formats = mask;
    return HAST_OK;
}

int hast_sq_feed_format(hast_sq_feed *f) { return f ? f->format : 0; }

hast_status hast_sq_feed_next(hast_sq_feed *f, int parent, hast_sq_result *res) {
    if (!f || !res) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->n_done == f->n_submitted) return set_error(HAST_ERR_INVALID, "hast_sq_feed_next: no block submitted");
    const int slot = (int)(f->n_done & 1);
    HAST_HIP_TRY(hipSetDevice(f->device));
    if (!f->on_device[slot]) HAST_HIP_TRY(hipStreamWaitEvent(f->table_stream, f->up_ev[slot], 0));
    const uint8_t *d_view = f->d_in[slot] + f->block - f->tail;
    const size_t n = f->tail + f->n_new[slot];
    if (f->format == 0) {                            // the first view of an input: its first byte decides, as it does for SeqParser
        f->format = 1;
        if (f->formats & HAST_SQ_TAKE_FASTA) {
            uint8_t first = 0;
            if (!f->on_device[slot]) first = f->h_in[slot][0];       // (still there: the block is not handed out again before it is framed)
            else {
                HAST_HIP_TRY(hipMemcpyAsync(&first, d_view, 1, hipMemcpyDeviceToHost, f->table_stream));
                HAST_HIP_TRY(hipStreamSynchronize(f->table_stream));
            }
            if (first == '>') f->format = 2;
        }
    }
    if (f->format == 2) {
        if (hast_status st = feed_fasta_view(f, slot, parent, d_view, n, false, res)) return st;
        if (!(res->flags & HAST_SQ_TAIL_TOO_LONG)) ++f->n_done;
        return HAST_OK;
    }
    if (hast_status st = hast_sq_frame_device(f->sq, d_view, n, f->d_out[slot], 2 * f->block + 64, res)) return st;
    if (res->flags & HAST_SQ_NOT_FOUR_LINE) return HAST_OK;
    const size_t left = n - (size_t)res->consumed;
    if (left > f->block) {
        res->flags |= HAST_SQ_TAIL_TOO_LONG;
        return HAST_OK;
    }
    if (res->out_bytes)
        if (hast_status st = hast_kc_count_device(f->kc, parent, f->d_out[slot], (size_t)res->out_bytes)) return st;
    if (left) HAST_HIP_TRY(hipMemcpyAsync(f->d_in[slot ^ 1] + f->block - left, d_view + res->consumed, left, hipMemcpyDeviceToDevice, f->table_stream));
    HAST_HIP_TRY(hipEventRecord(f->tail_ev, f->table_stream));
    f->tail_pending = true;
    f->tail = left;
    ++f->n_done;
    return HAST_OK;
}

hast_status hast_sq_feed_take_tail(hast_sq_feed *f, uint8_t *dst, size_t *n_bytes) {
    if (!f || !dst || !n_bytes) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->n_done != f->n_submitted) return set_error(HAST_ERR_INVALID, "hast_sq_feed_take_tail: a submitted block has not been framed");
    HAST_HIP_TRY(hipSetDevice(f->device));
    *n_bytes = f->tail;
    if (f->tail) {
        HAST_HIP_TRY(hipMemcpyAsync(dst, f->d_in[f->n_done & 1] + f->block - f->tail, f->tail, hipMemcpyDeviceToHost, f->table_stream));
        HAST_HIP_TRY(hipStreamSynchronize(f->table_stream));
    }
    f->tail = 0;
    f->format = 0;                                   // the input has ended
    f->fa_open = false;
    f->kept = 0;
    return HAST_OK;
}

hast_status hast_sq_feed_finish(hast_sq_feed *f, int parent, hast_sq_result *res) {
    if (!f || !res) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->n_done != f->n_submitted) return set_error(HAST_ERR_INVALID, "hast_sq_feed_finish: a submitted block has not been framed");
    if (f->format != 2) return set_error(HAST_ERR_INVALID, "hast_sq_feed_finish: the input is not FASTA; its end goes through hast_sq_feed_take_tail");
    HAST_HIP_TRY(hipSetDevice(f->device));
    const int slot = (int)(f->n_done & 1);
    if (hast_status st = feed_fasta_view(f, slot, parent, f->d_in[slot] + f->block - f->tail, f->tail, true, res)) return st;
    f->tail = f->kept = 0;
    f->format = 0;
    f->fa_open = false;
    return HAST_OK;
}

void hast_sq_feed_destroy(hast_sq_feed *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->up_stream) (void)hipStreamSynchronize(f->up_stream);
    if (f->table_stream) (void)hipStreamSynchronize(f->table_stream);
    hast_sq_destroy(f->sq);
    for (int i = 0; i < 2; ++i) {
        if (f->d_in[i]) (void)hipFree(f->d_in[i]);
        if (f->d_out[i]) (void)hipFree(f->d_out[i]);
        if (f->h_in[i]) (void)hipHostFree(f->h_in[i]);
        if (f->up_ev[i]) (void)hipEventDestroy(f->up_ev[i]);
    }
    if (f->tail_ev) (void)hipEventDestroy(f->tail_ev);
    if (f->up_stream) (void)hipStreamDestroy(f->up_stream);
    delete f;
}

}  // extern "C"
