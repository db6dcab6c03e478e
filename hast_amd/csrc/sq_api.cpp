// sq_api.cpp -- the part of the C ABI that frames raw four-line FASTQ, or FASTA, in device memory into the k-mer counter's base stream
// (include/hast.h "stage 00 ingest on the device"; the kernels are sq_kernels.hip and sq_fasta_kernels.hip, the rules sq_core.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "carry_feed.h"
#include "hast_internal.h"
#include "sq_device.h"

using namespace hast;

static_assert(HAST_SQ_NOT_FOUR_LINE == SQ_NOT_FOUR_LINE && HAST_SQ_NO_RECORD == SQ_NO_RECORD, "hast.h and sq_core.h name the same flags");
static_assert(sizeof(hast_sq_result) == 40 && offsetof(hast_sq_result, first_bad) == offsetof(SqState, first_bad), "hast_sq_result is the head of SqState");
static_assert(HAST_SQ_FA_OPEN == SQ_FA_OPEN && HAST_SQ_FA_LAST == SQ_FA_LAST, "hast.h and sq_core.h name the same flags");
static_assert(offsetof(hast_sq_result, first_bad) == offsetof(SqFaState, first_bad), "hast_sq_result is the head of SqFaState");

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

// one input stream of `unshared_kmers --ingest device` over a carried-block feed (carry_plan.h, carry_feed.h)
struct hast_sq_feed {
    hast_kc *kc = nullptr;
    hast_sq *sq = nullptr;
    CarryFeed in;                            // on the table's stream
    uint8_t *d_out[2] = {nullptr, nullptr};
    // FASTA (hast_sq_feed_set_formats): what the current input is, whether one of its headers has been seen, and how many of its last
    // emitted bytes lie in front of the next view's output, at d_out[slot] + kSqKeepPad - kept
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
    memcpy(res, q->h_st, sizeof *res);               // (the head of the state: the asserts above)
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
    memcpy(res, q->h_fa_st, sizeof *res);
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
    f->keep = (size_t)kc_k_of(kc) - 1;
    hipError_t e = f->in.create("hast_sq_feed", kc_device_of(kc), static_cast<hipStream_t>(hast_kc_stream(kc)), block_bytes);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = dev_malloc(&f->d_out[i], carry::room_of(block_bytes));
    hast_status st = e == hipSuccess ? hast_sq_create(kc, 2 * block_bytes, &f->sq)
                                     : set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_sq_feed_create: %s", hipGetErrorString(e));
    if (st != HAST_OK) {
        hast_sq_feed_destroy(f);
        return st;
    }
    *out = f;
    return HAST_OK;
}

hast_status hast_sq_feed_host_block(hast_sq_feed *f, uint8_t **h_buf) { return f ? f->in.block(1, h_buf) : set_error(HAST_ERR_INVALID, "null feed"); }
hast_status hast_sq_feed_device_block(hast_sq_feed *f, uint8_t **d_buf) { return f ? f->in.block(2, d_buf) : set_error(HAST_ERR_INVALID, "null feed"); }
hast_status hast_sq_feed_submit(hast_sq_feed *f, size_t n_bytes) { return f ? f->in.submit(n_bytes, false) : set_error(HAST_ERR_INVALID, "null feed"); }

// One view of a FASTA input: framed behind the kept bytes, counted with them in front (K - 1 bytes hold no window, so no window is
// counted twice and none across the cut is lost: ChunkSink's rule), its last K - 1 emitted bytes put in front of the next view's output
// and what it left in front of the next view's input.
static hast_status feed_fasta_view(hast_sq_feed *f, int parent, const carry::View &v, bool last, hast_sq_result *res) {
    uint8_t *out = f->d_out[v.slot] + kSqKeepPad;
    const unsigned in_flags = (f->fa_open ? HAST_SQ_FA_OPEN : 0u) | (last ? HAST_SQ_FA_LAST : 0u);
    if (hast_status st = hast_sq_frame_fasta_device(f->sq, f->in.at(v), v.bytes, out, carry::room_of(f->in.plan.block), in_flags, res)) return st;
    const size_t left = v.bytes - (size_t)res->consumed;
    if (!f->in.plan.fits(left)) {
        res->flags |= HAST_SQ_TAIL_TOO_LONG;
        return HAST_OK;
    }
    const size_t have = f->kept + (size_t)res->out_bytes;
    if (res->out_bytes && have > f->keep)
        if (hast_status st = hast_kc_count_device(f->kc, parent, out - f->kept, have)) return st;
    const size_t kept = std::min(f->keep, have);
    if (kept && !last)
        HAST_HIP_TRY(hipMemcpyAsync(f->d_out[v.slot ^ 1] + kSqKeepPad - kept, out + res->out_bytes - kept, kept, hipMemcpyDeviceToDevice, f->in.stream));
    if (hast_status st = f->in.carry(v, left, (size_t)res->consumed)) return st;
    f->kept = kept;
    if (res->records) f->fa_open = true;
    return HAST_OK;
}

hast_status hast_sq_feed_set_formats(hast_sq_feed *f, unsigned mask) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (!(mask & HAST_SQ_TAKE_FASTQ) || (mask & ~(HAST_SQ_TAKE_FASTQ | HAST_SQ_TAKE_FASTA)))
        return set_error(HAST_ERR_INVALID, "hast_sq_feed_set_formats: mask %#x (FASTQ, or FASTQ and FASTA)", mask);
    if (!f->in.plan.at_rest() || f->format)
        return set_error(HAST_ERR_INVALID, "hast_sq_feed_set_formats: an input is on its way through the feed");
    if ((mask & HAST_SQ_TAKE_FASTA) && !(f->formats & HAST_SQ_TAKE_FASTA)) {
        // a FASTA view's output lies behind the kept bytes and may end with the closing byte: larger output buffers
        HAST_HIP_TRY(hipSetDevice(f->in.device));
        HAST_HIP_TRY(hipStreamSynchronize(f->in.stream));
        for (int i = 0; i < 2; ++i) {
            uint8_t *d = nullptr;
            const hipError_t e = dev_malloc(&d, carry::room_of(f->in.plan.block) + 2 * kSqKeepPad);
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
    if (hast_status st = f->in.wait_step()) return st;
    const carry::View v = f->in.plan.view();
    const uint8_t *d_view = f->in.at(v);
    if (f->format == 0) {                            // the first view of an input: its first byte decides, as it does for SeqParser
        f->format = 1;
        if (f->formats & HAST_SQ_TAKE_FASTA) {
            uint8_t first = 0;
            if (!f->in.plan.on_device[v.slot]) first = f->in.h_in[v.slot][0];    // (still there: the block is not given out again before it is framed)
            else {
                HAST_HIP_TRY(hipMemcpyAsync(&first, d_view, 1, hipMemcpyDeviceToHost, f->in.stream));
                HAST_HIP_TRY(hipStreamSynchronize(f->in.stream));
            }
            if (first == '>') f->format = 2;
        }
    }
    if (f->format == 2) {
        if (hast_status st = feed_fasta_view(f, parent, v, false, res)) return st;
        if (!(res->flags & HAST_SQ_TAIL_TOO_LONG)) f->in.plan.done();
        return HAST_OK;
    }
    if (hast_status st = hast_sq_frame_device(f->sq, d_view, v.bytes, f->d_out[v.slot], carry::room_of(f->in.plan.block), res)) return st;
    if (res->flags & HAST_SQ_NOT_FOUR_LINE) return HAST_OK;
    const size_t left = v.bytes - (size_t)res->consumed;
    if (!f->in.plan.fits(left)) {
        res->flags |= HAST_SQ_TAIL_TOO_LONG;
        return HAST_OK;
    }
    if (res->out_bytes)
        if (hast_status st = hast_kc_count_device(f->kc, parent, f->d_out[v.slot], (size_t)res->out_bytes)) return st;
    if (hast_status st = f->in.carry(v, left, (size_t)res->consumed)) return st;
    f->in.plan.done();
    return HAST_OK;
}

hast_status hast_sq_feed_take_tail(hast_sq_feed *f, uint8_t *dst, size_t *n_bytes) {
    if (!f) return set_error(HAST_ERR_INVALID, "null argument");
    if (hast_status st = f->in.take_tail(dst, n_bytes)) return st;
    f->format = 0;                                   // the input has ended
    f->fa_open = false;
    f->kept = 0;
    return HAST_OK;
}

hast_status hast_sq_feed_finish(hast_sq_feed *f, int parent, hast_sq_result *res) {
    if (!f || !res) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->in.plan.waiting()) return set_error(HAST_ERR_INVALID, "hast_sq_feed_finish: a submitted block has not been framed");
    if (f->format != 2) return set_error(HAST_ERR_INVALID, "hast_sq_feed_finish: the input is not FASTA; its end goes through hast_sq_feed_take_tail");
    HAST_HIP_TRY(hipSetDevice(f->in.device));
    if (hast_status st = feed_fasta_view(f, parent, f->in.plan.tail_view(), true, res)) return st;
    f->in.plan.drop_tail();
    f->kept = 0;
    f->format = 0;
    f->fa_open = false;
    return HAST_OK;
}

void hast_sq_feed_destroy(hast_sq_feed *f) {
    if (!f) return;
    f->in.release(false);    // (freed: a count table has no context whose end would free what is parked)
    hast_sq_destroy(f->sq);
    for (uint8_t *d : f->d_out)
        if (d) (void)hipFree(d);
    delete f;
}

}  // extern "C"
