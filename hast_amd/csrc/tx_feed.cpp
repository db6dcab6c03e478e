// tx_feed.cpp -- the paired, pipelined device route of one fake_10x run (include/hast.h "stage 02", hast_tx_feed_*): both inputs'
// bytes are written or uploaded into HBM, the whole pairs of a step converted there (hast_tx_pair_device), both runs deflated as one
// job of the encoder (dz_kernels.hip) on a second stream while the next step is read and converted.  Who reads when: tx_feed_plan.h.
//
// Memory, all of it from hast_tx_feed_create.  Per side two input slots of `room` bytes: a step's bytes are [carried | new], the
// carried ones at the slot's first byte, the new ones directly behind them; what a step leaves goes to the front of the side's
// OTHER slot (device to device, on the converting stream), so the next block can be written while that copy runs.  Two output
// slots hold both runs of a step (read 1's at 0, read 2's at off1): one dz job covers them.  Step n uses output slot n & 1, and
// at most two steps wait for hast_tx_feed_collect, so slot n & 1 is free again when step n + 2 converts into it.
// Streams: cs converts (and is the stream callers fill device blocks on), us uploads host blocks, zs deflates, ds downloads.
//   cs: [fill] pair_device(n) job(n) carry(n) | [fill] pair_device(n+1) ...
//   zs:                      wait cs, compress(n), result(n)            | compress(n+1) ...
//   ds:                                    collect(n): members(n) down  |
// The download is enqueued by _collect and not by _step: a run's compressed size is known on the host only when the encoder has
// run, and the pinned slot it goes to is the caller's until the collect before this one has been followed by another.
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <zlib.h>

#include <new>
#include <vector>

#include "dz_device.h"
#include "hast_internal.h"
#include "tx_device.h"
#include "tx_feed_plan.h"

using namespace hast;

namespace {

double wall() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

struct Waiting {                   // a step that has not been collected
    bool on_host = false;
    unsigned ring = 0;             // on_host: which of host_out[] holds its outputs
    uint64_t raw[2] = {0, 0};
};

// one zlib gzip member, level 6, as fake_10x's host steps write them; nothing for an empty run
bool gzip_member(const uint8_t *p, size_t n, std::vector<uint8_t> &out) {
    out.clear();
    if (!n) return true;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 6, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    int r = Z_OK;
    for (size_t at = 0; r != Z_STREAM_END;) {
        const size_t piece = n - at < ((size_t)1 << 30) ? n - at : (size_t)1 << 30;
        z.next_in = const_cast<uint8_t *>(p + at);
        z.avail_in = (uInt)piece;
        at += piece;
        do {
            const size_t had = out.size();
            out.resize(had + (1u << 20));
            z.next_out = out.data() + had;
            z.avail_out = 1u << 20;
            r = deflate(&z, at == n ? Z_FINISH : Z_NO_FLUSH);
            out.resize(had + (1u << 20) - z.avail_out);
            if (r == Z_STREAM_ERROR) {
                deflateEnd(&z);
                return false;
            }
        } while (z.avail_out == 0 && r != Z_STREAM_END);
    }
    deflateEnd(&z);
    return true;
}

}  // namespace

struct hast_tx_feed {
    hast_tx *tx = nullptr;
    TxParts parts{};
    size_t block = 0, room = 0;
    bool gz = false;
    hipStream_t cs = nullptr, us = nullptr, zs = nullptr, ds = nullptr;
    // inputs
    uint8_t *d_in[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};      // [side][slot]
    int cur[2] = {0, 0};                                                 // the slot a side's next step reads
    uint8_t *h_in[2] = {nullptr, nullptr};                               // pinned, block bytes: a host block
    hipEvent_t up_ev[2] = {nullptr, nullptr};
    bool up_pending[2] = {false, false};
    int handed[2] = {0, 0};                                              // what the caller holds: 0 nothing, 1 a host block, 2 a device block
    txfeed::Side side[2];
    // outputs
    size_t cap_out = 0, off1 = 0, cap_gz = 0, cap_host = 0;
    uint8_t *d_out[2] = {nullptr, nullptr}, *d_gz[2] = {nullptr, nullptr}, *h_out[2] = {nullptr, nullptr};
    dz::EncoderSlot enc;                                                 // one workspace, a job and a result per output slot
    dz::Result *h_res = nullptr;                                         // pinned, two of them
    hipEvent_t conv_ev[2] = {nullptr, nullptr}, done_ev[2] = {nullptr, nullptr};
    uint64_t n_steps = 0, n_collected = 0;
    Waiting waiting[2];
    // the steps hast_tx_pair_host converts: pageable copies of the inputs, and four sets of outputs (a set stays the caller's until the
    // collect but one behind its own, and by then two more steps may have been converted)
    uint8_t *h_fall[2] = {nullptr, nullptr};
    std::vector<uint8_t> host_out[4][2];
    unsigned n_host_steps = 0;
    hast_tx_times times{0, 0, 0, 0};
    double collect_wait_s = 0;
};

static hast_status feed_side(const hast_tx_feed *f, int side) {
    if (!f) return set_error(HAST_ERR_INVALID, "null feed");
    if (side < 0 || side > 1) return set_error(HAST_ERR_INVALID, "hast_tx_feed: side %d (0 or 1)", side);
    return HAST_OK;
}

extern "C" {

hast_status hast_tx_feed_create(hast_tx *t, size_t block_bytes, int gz_out, hast_tx_feed **out) {
    if (!t || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (block_bytes < 64) return set_error(HAST_ERR_INVALID, "hast_tx_feed_create: blocks of %zu bytes (64 at least)", block_bytes);
    const TxParts parts = tx_parts_of(t);
    if (block_bytes > kTxMaxIn || 2 * block_bytes + 4096 > kTxMaxIn || txfeed::room_of(block_bytes) > parts.max_in)
        return set_error(HAST_ERR_UNSUPPORTED, "hast_tx_feed_create: blocks of %zu bytes need %zu bytes a side, the converter was created for %zu (at most %zu)",
                         block_bytes, 2 * block_bytes + 4096, parts.max_in, kTxMaxIn);
    hast_tx_feed *f = new (std::nothrow) hast_tx_feed;
    if (!f) return set_error(HAST_ERR_OOM, "hast_tx_feed_create");
    f->tx = t;
    f->parts = parts;
    f->block = block_bytes;
    f->room = txfeed::room_of(block_bytes);
    f->gz = gz_out != 0;
    f->cap_out = 2 * f->room + 4096;
    f->off1 = (f->cap_out + 255) & ~(size_t)255;
    f->cap_host = 2 * f->off1;
    hipError_t e = hipSetDevice(parts.device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->cs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->us, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->zs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->ds, hipStreamNonBlocking);
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        for (int slot = 0; slot < 2 && e == hipSuccess; ++slot) e = dev_malloc(&f->d_in[s][slot], f->room + 64);
        if (e == hipSuccess) e = pinned_malloc(&f->h_in[s], f->block);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->up_ev[s], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->conv_ev[s], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->done_ev[s], hipEventDisableTiming);
        if (e == hipSuccess) e = dev_malloc(&f->d_out[s], 2 * f->off1 + 64);
        if (e == hipSuccess && !(f->h_fall[s] = static_cast<uint8_t *>(malloc(f->room)))) e = hipErrorOutOfMemory;
    }
    if (e == hipSuccess && f->gz) {
        f->cap_gz = (size_t)dz::max_out_bytes(2 * (uint64_t)f->cap_out);
        if (f->cap_gz > f->cap_host) f->cap_host = f->cap_gz;
        e = dz::slot_alloc(&f->enc, dz::max_pieces(2 * (uint64_t)f->cap_out), 2);
        if (e == hipSuccess) e = pinned_malloc(&f->h_res, 2 * sizeof(dz::Result));
        for (int slot = 0; slot < 2 && e == hipSuccess; ++slot) e = dev_malloc(&f->d_gz[slot], f->cap_gz + 64);
    }
    for (int slot = 0; slot < 2 && e == hipSuccess; ++slot) e = pinned_malloc(&f->h_out[slot], f->cap_host);
    if (e != hipSuccess) {
        hast_tx_feed_destroy(f);
        return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_tx_feed_create: blocks of %zu bytes: %s", block_bytes, hipGetErrorString(e));
    }
    *out = f;
    return HAST_OK;
}

int hast_tx_feed_wants(const hast_tx_feed *f, int side) { return f && side >= 0 && side <= 1 && f->side[side].wants(f->block) ? 1 : 0; }

size_t hast_tx_feed_room(const hast_tx_feed *f) { return f ? f->room : 0; }

static hast_status feed_block(hast_tx_feed *f, int side) {
    if (hast_status st = feed_side(f, side)) return st;
    if (!f->side[side].wants(f->block)) return set_error(HAST_ERR_INVALID, "hast_tx_feed: side %d reads nothing for this step", side);
    if (!txfeed::fits(f->side[side].carry, f->block, f->room))
        return set_error(HAST_ERR_INVALID, "hast_tx_feed: side %d carries %zu bytes, a block of %zu does not fit %zu", side, f->side[side].carry, f->block, f->room);
    return HAST_OK;
}

hast_status hast_tx_feed_device_block(hast_tx_feed *f, int side, uint8_t **d_buf, hast_stream *fill_stream) {
    if (hast_status st = feed_block(f, side)) return st;
    if (!d_buf || !fill_stream) return set_error(HAST_ERR_INVALID, "null argument");
    f->handed[side] = 2;
    *d_buf = f->d_in[side][f->cur[side]] + f->side[side].carry;      // (written on cs: behind everything that reads or writes this slot)
    *fill_stream = f->cs;
    return HAST_OK;
}

hast_status hast_tx_feed_host_block(hast_tx_feed *f, int side, uint8_t **h_buf) {
    if (hast_status st = feed_block(f, side)) return st;
    if (!h_buf) return set_error(HAST_ERR_INVALID, "null argument");
    f->handed[side] = 1;                                               // (its last upload was waited for by the step that read it)
    *h_buf = f->h_in[side];
    return HAST_OK;
}

hast_status hast_tx_feed_submit(hast_tx_feed *f, int side, size_t n_bytes) {
    if (hast_status st = feed_side(f, side)) return st;
    if (!f->handed[side] || n_bytes > f->block) return set_error(HAST_ERR_INVALID, "hast_tx_feed_submit: %zu bytes of a block of %zu", n_bytes, f->block);
    if (f->handed[side] == 1 && n_bytes) {
        // the slot's earlier readers are through (a step returns when its conversion has run); the copy of the carried bytes into the
        // slot's front may still run, beside this one
        const double t0 = wall();
        HAST_HIP_TRY(hipSetDevice(f->parts.device));
        HAST_HIP_TRY(hipMemcpyAsync(f->d_in[side][f->cur[side]] + f->side[side].carry, f->h_in[side], n_bytes, hipMemcpyHostToDevice, f->us));
        HAST_HIP_TRY(hipEventRecord(f->up_ev[side], f->us));
        f->up_pending[side] = true;
        f->times.upload_s += wall() - t0;
    }
    f->side[side].submitted(n_bytes, f->block);
    f->handed[side] = 0;
    return HAST_OK;
}

hast_status hast_tx_feed_step(hast_tx_feed *f, hast_tx_state *state, hast_tx_result *res, int *flags) {
    if (!f || !state || !res || !flags) return set_error(HAST_ERR_INVALID, "null argument");
    *flags = 0;
    if (f->handed[0] || f->handed[1]) return set_error(HAST_ERR_INVALID, "hast_tx_feed_step: a block has been handed out and not submitted");
    if (f->n_steps - f->n_collected >= 2) return set_error(HAST_ERR_INVALID, "hast_tx_feed_step: two steps are waiting for hast_tx_feed_collect");
    HAST_HIP_TRY(hipSetDevice(f->parts.device));
    const uint8_t *p[2];
    size_t n[2];
    for (int s = 0; s < 2; ++s) {
        if (f->up_pending[s]) {
            HAST_HIP_TRY(hipStreamWaitEvent(f->cs, f->up_ev[s], 0));
            f->up_pending[s] = false;
        }
        p[s] = f->d_in[s][f->cur[s]];
        n[s] = f->side[s].held();
    }
    const unsigned slot = (unsigned)(f->n_steps & 1);
    uint8_t *const d_o[2] = {f->d_out[slot], f->d_out[slot] + f->off1};
    hast_tx_state after = *state;
    double t0 = wall();
    hast_status st = hast_tx_pair_device(f->tx, p[0], n[0], p[1], n[1], &after, d_o[0], 2 * n[0] + 4096, d_o[1], 2 * n[1] + 4096, res, f->cs);
    f->times.kernel_s += wall() - t0;
    if (st != HAST_OK && st != HAST_ERR_UNSUPPORTED) return st;
    if (txfeed::mode_of(f->side[0].eof, f->side[1].eof, res->lines[0], res->lines[1]) != 0) {
        // an input has ended without a whole record: there was no whole pair, nothing was converted; the bytes stay where they are
        for (int s = 0; s < 2; ++s) f->side[s].stepped(res->lines[s], 0, 0);
        const uint32_t lines[2] = {res->lines[0], res->lines[1]};
        memset(res, 0, sizeof *res);
        res->lines[0] = lines[0];
        res->lines[1] = lines[1];
        *flags = (int)HAST_TX_ENDS;
        return HAST_OK;
    }
    Waiting &w = f->waiting[slot];
    w.on_host = st == HAST_ERR_UNSUPPORTED;
    if (w.on_host) {
        // the outputs outgrow their room: the step's two ranges come down and the host model converts them
        t0 = wall();
        for (int s = 0; s < 2; ++s)
            if (n[s]) HAST_HIP_TRY(hipMemcpyAsync(f->h_fall[s], p[s], n[s], hipMemcpyDeviceToHost, f->cs));
        HAST_HIP_TRY(hipStreamSynchronize(f->cs));
        f->times.download_s += wall() - t0;
        uint8_t *o[2] = {nullptr, nullptr};
        st = hast_tx_pair_host(f->parts.map, f->h_fall[0], n[0], f->h_fall[1], n[1], 0, &after, &o[0], &o[1], res);
        if (st != HAST_OK) return st;
        w.ring = f->n_host_steps++ & 3;
        bool ok = true;
        for (int s = 0; s < 2; ++s) {
            std::vector<uint8_t> &dst = f->host_out[w.ring][s];
            if (f->gz) ok = gzip_member(o[s], (size_t)res->raw_bytes[s], dst) && ok;
            else dst.assign(o[s], o[s] + res->raw_bytes[s]);
            hast_tx_free(o[s]);
        }
        if (!ok) return set_error(HAST_ERR_OOM, "hast_tx_feed_step: zlib could not deflate a run");
        *flags |= (int)HAST_TX_ON_HOST;
    } else {
        if (f->gz) HAST_HIP_TRY(dz::launch_job_from_tx(f->enc.job(slot), f->parts.d_state->out_bytes, f->off1, f->cs));
        HAST_HIP_TRY(hipEventRecord(f->conv_ev[slot], f->cs));
        HAST_HIP_TRY(hipStreamWaitEvent(f->zs, f->conv_ev[slot], 0));
        if (f->gz) {
            HAST_HIP_TRY(dz::launch_compress(f->enc.job(slot), f->d_out[slot], f->enc.max_pieces, f->enc.d_work, f->d_gz[slot], f->cap_gz, f->enc.res(slot), 0, f->zs));
            HAST_HIP_TRY(hipMemcpyAsync(f->h_res + slot, f->enc.res(slot), sizeof(dz::Result), hipMemcpyDeviceToHost, f->zs));
        }
        HAST_HIP_TRY(hipEventRecord(f->done_ev[slot], f->zs));
    }
    w.raw[0] = res->raw_bytes[0];
    w.raw[1] = res->raw_bytes[1];
    // what is left goes to the front of the side's other slot
    const uint64_t consumed[2] = {res->consumed1, res->consumed2};
    for (int s = 0; s < 2; ++s) {
        const size_t left = n[s] - (size_t)consumed[s];
        if (left) HAST_HIP_TRY(hipMemcpyAsync(f->d_in[s][f->cur[s] ^ 1], p[s] + consumed[s], left, hipMemcpyDeviceToDevice, f->cs));
        f->cur[s] ^= 1;
        f->side[s].stepped(res->lines[s], res->pairs, consumed[s]);
        if (f->side[s].wants(f->block) && !txfeed::fits(left, f->block, f->room)) *flags |= (int)HAST_TX_TAIL_TOO_LONG;
    }
    *state = after;
    ++f->n_steps;
    return HAST_OK;
}

hast_status hast_tx_feed_collect(hast_tx_feed *f, const uint8_t **out1, const uint8_t **out2, uint64_t out_bytes[2], uint64_t raw_bytes[2]) {
    if (!f || !out1 || !out2 || !out_bytes || !raw_bytes) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->n_collected == f->n_steps) return set_error(HAST_ERR_INVALID, "hast_tx_feed_collect: no step is waiting");
    const unsigned slot = (unsigned)(f->n_collected & 1);
    const Waiting &w = f->waiting[slot];
    const uint8_t *o[2] = {nullptr, nullptr};
    const double t_in = wall();
    if (w.on_host) {
        for (int s = 0; s < 2; ++s) {
            o[s] = f->host_out[w.ring][s].data();
            out_bytes[s] = f->host_out[w.ring][s].size();
        }
    } else {
        HAST_HIP_TRY(hipSetDevice(f->parts.device));
        double t0 = wall();
        HAST_HIP_TRY(hipEventSynchronize(f->done_ev[slot]));
        f->times.deflate_s += wall() - t0;
        t0 = wall();
        uint8_t *h = f->h_out[slot];
        if (f->gz) {
            const dz::Result r = f->h_res[slot];
            if (r.flags) return set_error(HAST_ERR_HIP, "hast_tx_feed_collect: the members did not fit their bound (flags %u)", r.flags);
            uint64_t total = 0;
            for (int s = 0; s < 2; ++s) {
                out_bytes[s] = r.out_bytes[s];
                o[s] = h + (r.out_bytes[s] ? r.member_off[s] : 0);
                if (r.out_bytes[s] && r.member_off[s] + r.out_bytes[s] > total) total = r.member_off[s] + r.out_bytes[s];
            }
            if (total > f->cap_gz) return set_error(HAST_ERR_HIP, "hast_tx_feed_collect: members of %llu bytes", (unsigned long long)total);
            if (total) HAST_HIP_TRY(hipMemcpyAsync(h, f->d_gz[slot], (size_t)total, hipMemcpyDeviceToHost, f->ds));
        } else {
            for (int s = 0; s < 2; ++s) {
                out_bytes[s] = w.raw[s];
                o[s] = h + (s ? f->off1 : 0);
                if (w.raw[s]) HAST_HIP_TRY(hipMemcpyAsync(h + (s ? f->off1 : 0), f->d_out[slot] + (s ? f->off1 : 0), (size_t)w.raw[s], hipMemcpyDeviceToHost, f->ds));
            }
        }
        HAST_HIP_TRY(hipStreamSynchronize(f->ds));
        f->times.download_s += wall() - t0;
    }
    raw_bytes[0] = w.raw[0];
    raw_bytes[1] = w.raw[1];
    *out1 = o[0];
    *out2 = o[1];
    f->collect_wait_s += wall() - t_in;
    ++f->n_collected;
    return HAST_OK;
}

hast_status hast_tx_feed_take_tail(hast_tx_feed *f, int side, uint8_t *dst, size_t *n_bytes) {
    if (hast_status st = feed_side(f, side)) return st;
    if (!dst || !n_bytes) return set_error(HAST_ERR_INVALID, "null argument");
    if (f->handed[side]) return set_error(HAST_ERR_INVALID, "hast_tx_feed_take_tail: a block has been handed out and not submitted");
    HAST_HIP_TRY(hipSetDevice(f->parts.device));
    if (f->up_pending[side]) {
        HAST_HIP_TRY(hipStreamWaitEvent(f->cs, f->up_ev[side], 0));
        f->up_pending[side] = false;
    }
    const size_t n = f->side[side].held();
    *n_bytes = n;
    if (n) HAST_HIP_TRY(hipMemcpyAsync(dst, f->d_in[side][f->cur[side]], n, hipMemcpyDeviceToHost, f->cs));
    HAST_HIP_TRY(hipStreamSynchronize(f->cs));
    const bool eof = f->side[side].eof;
    f->side[side] = txfeed::Side();
    f->side[side].eof = eof;
    return HAST_OK;
}

hast_status hast_tx_feed_times(const hast_tx_feed *f, hast_tx_times *times, double *collect_wait_s) {
    if (!f || !times) return set_error(HAST_ERR_INVALID, "null argument");
    times->upload_s += f->times.upload_s;
    times->kernel_s += f->times.kernel_s;
    times->deflate_s += f->times.deflate_s;
    times->download_s += f->times.download_s;
    if (collect_wait_s) *collect_wait_s = f->collect_wait_s;
    return HAST_OK;
}

void hast_tx_feed_destroy(hast_tx_feed *f) {
    if (!f) return;
    (void)hipSetDevice(f->parts.device);
    for (hipStream_t s : {f->cs, f->us, f->zs, f->ds})
        if (s) (void)hipStreamSynchronize(s);
    for (int s = 0; s < 2; ++s) {
        for (int slot = 0; slot < 2; ++slot)
            if (f->d_in[s][slot]) (void)hipFree(f->d_in[s][slot]);
        if (f->h_in[s]) (void)hipHostFree(f->h_in[s]);
        if (f->d_out[s]) (void)hipFree(f->d_out[s]);
        if (f->d_gz[s]) (void)hipFree(f->d_gz[s]);
        if (f->h_out[s]) (void)hipHostFree(f->h_out[s]);
        for (hipEvent_t ev : {f->up_ev[s], f->conv_ev[s], f->done_ev[s]})
            if (ev) (void)hipEventDestroy(ev);
        free(f->h_fall[s]);
    }
    dz::slot_release(&f->enc, false);
    if (f->h_res) (void)hipHostFree(f->h_res);
    for (hipStream_t s : {f->cs, f->us, f->zs, f->ds})
        if (s) (void)hipStreamDestroy(s);
    delete f;
}

}  // extern "C"
