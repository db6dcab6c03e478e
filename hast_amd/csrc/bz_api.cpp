// bz_api.cpp -- the stream behind hast_gz_open_blocked (include/hast.h): a BGZF file inflated on the GPU per member.
//
// One producer thread per open file: pread a piece into pinned memory, walk its members (bz_core.h plan_batch; a member cut by the
// piece's end is carried to the front of the next piece), upload the piece and the member records, launch k_bz_inflate and k_bz_crc
// on the stream's own HIP stream, record an event.  Three sets of buffers ("slots") take turns: batch n + 1 is read and uploaded
// while batch n is decoded and the reader copies out of batch n - 1 -- two batches in flight on the device, one with the reader.  The
// reader (stream_read, the body of hast_gz_read_device on such a handle) waits for a batch's event, looks at the 8 bytes the check
// kernel left (the first refused member, or none) and copies device to device on the caller's stream; a slot goes back to the
// producer with an event on that stream, which the producer's stream waits for before it writes the slot's output again.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hast.h"
#include "bz_core.h"
#include "bz_device.h"
#include "hast_internal.h"
#include "switches.h"

namespace hast {
namespace bz {

namespace {

// Default geometry: 32 MB of compressed bytes, 192 MB of output a batch (HAST_BZ_BATCH_IN_BYTES / HAST_BZ_BATCH_OUT_BYTES: measurements,
// and callers that cannot pass a geometry).  A member is one wave for ~3 ms whatever else runs, so a batch wants as many members as the
// part has wave slots at k_bz_inflate's occupancy (5 120): 20M reads as two BGZF files, read phase of `classify` at 8:64 MB 0.28-0.29 s,
// 16:96 0.23-0.24 s, 32:192 0.17-0.18 s, 64:384 0.15-0.16 s with the open twice as long (profiles/bgzf_geometry.txt); the ordinary-gzip
// device route on the same reads 0.18-0.20 s.  Three slots of 32 + 192 MB are 672 MB of HBM a stream, a quarter of what an ordinary
// .gz stream's symbol arenas take.
constexpr size_t kBatchIn = 32u << 20, kBatchOut = 192u << 20;
constexpr size_t kMaxBatchMembers = (size_t)1 << 18;      // records a batch holds (8 MB of pinned memory a slot); k_bz_crc packs index << 8 | reason
constexpr size_t kInPad = 256;                // zero bytes behind a batch's last input byte on the device (the bit readers look ahead)
constexpr size_t kCarryRoom = 2 * kMaxMember; // room for a carried member (or a long non-BGZF header) in front of a piece
constexpr int kSlots = 3;
constexpr size_t kMinMemberBytes = 28;        // header 18 + 2 of deflate + trailer 8

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Slot {
    uint8_t *h_in = nullptr;                  // pinned: carry + piece + padding
    Member *h_mem = nullptr;                  // pinned
    uint32_t *h_first = nullptr;              // pinned: what k_bz_crc left (2 words)
    uint8_t *d_in = nullptr, *d_out = nullptr;
    Member *d_mem = nullptr;
    MemberOut *d_res = nullptr;
    uint32_t *d_verdict = nullptr, *d_first = nullptr;
    hipEvent_t ev_begin = nullptr, ev_uploaded = nullptr, ev_done = nullptr;      // on the stream's own HIP stream
    hipEvent_t ev_copied = nullptr;           // on the caller's stream, behind the reader's last copy out of d_out
    bool copied_recorded = false;
};

// what the producer hands the reader, in stream order
struct Item {
    int slot = -1;                            // >= 0: a batch; -1: the end, or why the stream ends here
    size_t n_members = 0;
    uint64_t out_bytes = 0, file_off = 0;     // file_off: where the batch's first member lies in the file
    hast_status status = HAST_OK;             // slot < 0: HAST_OK = end of stream
    std::string error;
};

}  // namespace

struct Stream {
    hast_ctx *ctx = nullptr;
    int device = 0, fd = -1;
    std::string path;
    uint64_t file_size = 0;
    size_t batch_in = kBatchIn, batch_out = kBatchOut, in_cap = 0, mem_cap = 0;
    Slot slot[kSlots];
    hipStream_t stream = nullptr;
    std::thread producer;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Item> ready;
    bool slot_free[kSlots] = {true, true, true};
    bool stop = false;
    // reader
    bool have_cur = false, done = false;
    Item cur;
    uint64_t cur_avail = 0, cur_pos = 0;      // bytes of the current batch that may be delivered / that have been
    std::string cur_bad;                      // why the current batch ends in front of its last member
    hast_status err_status = HAST_OK;
    std::string err;
    uint64_t delivered = 0;
    // stats (mu)
    hast_gz_blocked_stats bs{};
    double open_s = 0;
};

namespace {

bool read_at(int fd, uint64_t off, size_t n, uint8_t *dst, size_t *got) {
    size_t g = 0;
    while (g < n) {
        const ssize_t r = pread(fd, dst + g, n - g, (off_t)(off + g));
        if (r < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        if (r == 0) break;
        g += (size_t)r;
    }
    *got = g;
    return true;
}

void publish(Stream *z, Item &&it) {
    std::lock_guard<std::mutex> lk(z->mu);
    z->ready.push_back(std::move(it));
    z->cv.notify_all();
}
void publish_end(Stream *z, hast_status st, const std::string &msg) {
    Item it;
    it.status = st;
    it.error = msg;
    publish(z, std::move(it));
}

void produce_loop(Stream *z) {
    (void)hipSetDevice(z->device);
    uint64_t file_pos = 0;                    // next byte of the file to read
    std::vector<uint8_t> carry;               // bytes read but not yet part of a batch
    bool eof = false;
    int next_slot = 0;
    // bytes a piece is topped up to.  A batch that ends on its output or record limit leaves the rest of its piece to be carried: on
    // input that compresses well that would be most of batch_in, copied twice for every batch -- so the goal follows what the last such
    // batch took (plus a quarter and one member), and grows again when the input limit binds.  Never less than kCarryRoom: with that
    // much present a whole member (or a whole non-BGZF header) is there, and the walk moves on.
    size_t read_goal = std::max(z->batch_in, kCarryRoom);
    auto hip_fail = [&](const char *what, hipError_t e) { publish_end(z, HAST_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
    for (;;) {
        const int si = next_slot;
        next_slot = (next_slot + 1) % kSlots;
        Slot &S = z->slot[si];
        {
            std::unique_lock<std::mutex> lk(z->mu);
            const double t0 = now_s();
            z->cv.wait(lk, [&] { return z->stop || z->slot_free[si]; });
            z->bs.wait_reader_s += now_s() - t0;
            if (z->stop) return;
            z->slot_free[si] = false;
        }
        const double t_read0 = now_s();
        // the piece: what was carried, then as much of the file as the slot holds
        size_t have = carry.size();
        if (have) memcpy(S.h_in, carry.data(), have);
        const uint64_t batch_file_off = file_pos - have;
        if (!eof) {
            const size_t want = have >= read_goal ? 0 : std::min(read_goal - have, z->in_cap - have);
            size_t got = 0;
            if (want && !read_at(z->fd, file_pos, want, S.h_in + have, &got)) {
                publish_end(z, HAST_ERR_IO, "read error");
                return;
            }
            file_pos += got;
            have += got;
            if (got < want || file_pos >= z->file_size) eof = true;
        }
        const Plan pl = plan_batch(S.h_in, have, eof, z->batch_in, z->batch_out, 0, S.h_mem, z->mem_cap);
        const bool cut = pl.stop == kStopCut || pl.stop == kStopFull;
        if (pl.stop == kStopFull && pl.resume < z->batch_in) read_goal = std::max(kCarryRoom, std::min(z->batch_in, pl.resume + pl.resume / 4 + kMaxMember));
        else if (pl.stop == kStopCut) read_goal = std::max(kCarryRoom, std::min(z->batch_in, 2 * read_goal));
        carry.assign(S.h_in + pl.resume, S.h_in + (cut ? have : pl.resume));
        memset(S.h_in + pl.resume, 0, kInPad);
        const double t_read1 = now_s();
        {
            std::lock_guard<std::mutex> lk(z->mu);
            z->bs.read_s += t_read1 - t_read0;
            z->bs.members += pl.n_members;
            if (pl.n_members) z->bs.batches++;
            if (pl.stop == kStopCut && !carry.empty()) z->bs.carried++;
        }
        if (pl.n_members) {
            hipError_t e = hipSuccess;
            auto step = [&](hipError_t r) { if (e == hipSuccess) e = r; };
            // (the reader's copies out of this slot's previous batch run on the caller's stream)
            if (S.copied_recorded) step(hipStreamWaitEvent(z->stream, S.ev_copied, 0));
            step(hipEventRecord(S.ev_begin, z->stream));
            step(hipMemcpyAsync(S.d_in, S.h_in, pl.resume + kInPad, hipMemcpyHostToDevice, z->stream));
            step(hipMemcpyAsync(S.d_mem, S.h_mem, pl.n_members * sizeof(Member), hipMemcpyHostToDevice, z->stream));
            step(hipMemsetAsync(S.d_first, 0xFF, 2 * sizeof(uint32_t), z->stream));
            step(hipEventRecord(S.ev_uploaded, z->stream));
            step(launch_inflate(S.d_mem, (uint32_t)pl.n_members, reinterpret_cast<const uint32_t *>(S.d_in), S.d_out, S.d_res, z->stream));
            step(launch_check(S.d_mem, (uint32_t)pl.n_members, S.d_out, S.d_res, S.d_verdict, S.d_first, z->stream));
            step(hipMemcpyAsync(S.h_first, S.d_first, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, z->stream));
            step(hipEventRecord(S.ev_done, z->stream));
            if (e != hipSuccess) {
                hip_fail("blocked inflate", e);
                return;
            }
            Item it;
            it.slot = si;
            it.n_members = pl.n_members;
            it.out_bytes = pl.out_bytes;
            it.file_off = batch_file_off;
            publish(z, std::move(it));
        } else {
            std::lock_guard<std::mutex> lk(z->mu);
            z->slot_free[si] = true;
        }
        const uint64_t stop_off = batch_file_off + pl.resume;
        char msg[200];
        switch (pl.stop) {
        case kStopFull:
        case kStopCut:
            if (pl.n_members == 0 && eof) {    // (cannot happen: at the end of the file a cut member is a truncated one)
                publish_end(z, HAST_ERR_IO, "bgzf: the file ends inside a block");
                return;
            }
            continue;
        case kStopEnd:
        case kStopNotGzip:
            publish_end(z, HAST_OK, "");
            return;
        case kStopTruncated:
            snprintf(msg, sizeof msg, "bgzf: the file ends inside the block at file offset %llu", (unsigned long long)stop_off);
            publish_end(z, HAST_ERR_IO, msg);
            return;
        case kStopTooLarge:
            snprintf(msg, sizeof msg, "bgzf: the block at file offset %llu claims more than 64 KB", (unsigned long long)stop_off);
            publish_end(z, HAST_ERR_IO, msg);
            return;
        case kStopNotBgzf:
            snprintf(msg, sizeof msg, "bgzf: a gzip member that is not blocked gzip: unsupported from file offset %llu", (unsigned long long)stop_off);
            {
                std::lock_guard<std::mutex> lk(z->mu);
                z->bs.unsupported_offset = stop_off;
            }
            publish_end(z, HAST_ERR_UNSUPPORTED, msg);
            return;
        }
    }
}

void free_slot_buffers(Slot &S, size_t in_bytes, size_t out_bytes, size_t mem_cap) {
    park_pinned(S.h_in, in_bytes, 1);
    park_pinned(S.h_mem, mem_cap * sizeof(Member), 1);
    park_pinned(S.h_first, 2 * sizeof(uint32_t), 1);
    park_device(S.d_in, in_bytes, 1);
    park_device(S.d_out, out_bytes, 1);
    park_device(S.d_mem, mem_cap * sizeof(Member), 1);
    park_device(S.d_res, mem_cap * sizeof(MemberOut), 1);
    park_device(S.d_verdict, mem_cap * sizeof(uint32_t), 1);
    park_device(S.d_first, 2 * sizeof(uint32_t), 1);
    for (hipEvent_t *e : {&S.ev_begin, &S.ev_uploaded, &S.ev_done, &S.ev_copied})
        if (*e) (void)hipEventDestroy(*e);
    S = Slot();
}

}  // namespace

hast_status stream_open(hast_ctx *ctx, const char *path, size_t batch_in_bytes, size_t batch_out_bytes, Stream **out) {
    *out = nullptr;
    const double t0 = now_s();
    const int fd = open(path, O_RDONLY | O_NONBLOCK);         // (a FIFO without a writer must not hang the open)
    if (fd < 0) return set_error(HAST_ERR_IO, "cannot read %s", path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        close(fd);
        return set_error(HAST_ERR_UNSUPPORTED, "%s is not a regular file: the device inflate reads by position", path);
    }
    if (sb.st_size == 0) {
        close(fd);
        return set_error(HAST_ERR_UNSUPPORTED, "%s is empty", path);
    }
    {   // the header rule on the file's first bytes (a BC subfield may lie anywhere in the extra field)
        std::vector<uint8_t> head((size_t)std::min<uint64_t>((uint64_t)sb.st_size, 12 + 65535));
        size_t got = 0, hdr = 0, total = 0;
        if (!read_at(fd, 0, head.size(), head.data(), &got)) {
            close(fd);
            return set_error(HAST_ERR_IO, "cannot read %s", path);
        }
        if (!parse_header(head.data(), got, hdr, total)) {
            close(fd);
            return set_error(HAST_ERR_UNSUPPORTED, "%s does not start with a blocked-gzip (BGZF) member", path);
        }
    }
    std::unique_ptr<Stream> z(new (std::nothrow) Stream());
    if (!z) {
        close(fd);
        return set_error(HAST_ERR_OOM, "host allocation failed");
    }
    z->ctx = ctx;
    z->device = ctx_device_of(ctx);
    z->fd = fd;
    z->path = path;
    z->file_size = (uint64_t)sb.st_size;
    if (!batch_in_bytes) sw::size(sw::HAST_BZ_BATCH_IN_BYTES, &batch_in_bytes);
    if (!batch_out_bytes) sw::size(sw::HAST_BZ_BATCH_OUT_BYTES, &batch_out_bytes);
    z->batch_in = std::max<size_t>(batch_in_bytes ? batch_in_bytes : kBatchIn, kMaxMember);
    z->batch_out = std::max<size_t>(batch_out_bytes ? batch_out_bytes : kBatchOut, kMaxIsize);
    if (z->batch_in > (1u << 30) || z->batch_out > (1ull << 32)) {
        close(fd);
        return set_error(HAST_ERR_INVALID, "hast_gz_open_blocked_ex: batch too large");
    }
    z->in_cap = z->batch_in + kCarryRoom;                      // (bytes of file a slot holds; kInPad of zeros follow)
    z->mem_cap = std::min<size_t>(z->batch_in / kMinMemberBytes + 1, kMaxBatchMembers);
    const size_t in_bytes = z->in_cap + kInPad, out_bytes = z->batch_out + 16;
    hipError_t e = hipSetDevice(z->device);
    auto step = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    step(hipStreamCreateWithFlags(&z->stream, hipStreamNonBlocking));
    for (Slot &S : z->slot) {
        step(pinned_malloc(&S.h_in, in_bytes));
        step(pinned_malloc(&S.h_mem, z->mem_cap * sizeof(Member)));
        step(pinned_malloc(&S.h_first, 2 * sizeof(uint32_t)));
        step(dev_malloc(&S.d_in, in_bytes));
        step(dev_malloc(&S.d_out, out_bytes));
        step(dev_malloc(&S.d_mem, z->mem_cap * sizeof(Member)));
        step(dev_malloc(&S.d_res, z->mem_cap * sizeof(MemberOut)));
        step(dev_malloc(&S.d_verdict, z->mem_cap * sizeof(uint32_t)));
        step(dev_malloc(&S.d_first, 2 * sizeof(uint32_t)));
        step(hipEventCreate(&S.ev_begin));
        step(hipEventCreate(&S.ev_uploaded));
        step(hipEventCreate(&S.ev_done));
        step(hipEventCreateWithFlags(&S.ev_copied, hipEventDisableTiming));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (Slot &S : z->slot) free_slot_buffers(S, in_bytes, out_bytes, z->mem_cap);
        if (z->stream) (void)hipStreamDestroy(z->stream);
        close(fd);
        if (e == hipErrorOutOfMemory) return set_error(HAST_ERR_UNSUPPORTED, "%s: no room on the device for the blocked inflate", path);
        return set_error(HAST_ERR_HIP, "hast_gz_open_blocked: %s", hipGetErrorString(e));
    }
    Stream *raw = z.release();
    raw->producer = std::thread(produce_loop, raw);
    raw->open_s = now_s() - t0;
    *out = raw;
    return HAST_OK;
}

hast_status stream_read(Stream *z, uint8_t *d_dst, size_t cap, size_t *n_out, hipStream_t hs) {
    *n_out = 0;
    if (!z->err.empty()) return set_error(z->err_status, "%s: %s", z->path.c_str(), z->err.c_str());
    if (hipSetDevice(z->device) != hipSuccess) return set_error(HAST_ERR_HIP, "hipSetDevice failed");
    size_t got = 0;
    while (got < cap && !z->done) {
        if (!z->have_cur) {
            {
                std::unique_lock<std::mutex> lk(z->mu);
                z->cv.wait(lk, [&] { return !z->ready.empty(); });
                z->cur = std::move(z->ready.front());
                z->ready.pop_front();
            }
            Item &it = z->cur;
            if (it.slot < 0) {
                if (it.status == HAST_OK) {
                    z->done = true;
                    break;
                }
                z->err_status = it.status;
                z->err = it.error;
                // what lies in front has been delivered; the error comes with the next call (as hast_gz_open's streams do)
                if (got) break;
                return set_error(z->err_status, "%s: %s", z->path.c_str(), z->err.c_str());
            }
            Slot &S = z->slot[it.slot];
            if (hipEventSynchronize(S.ev_done) != hipSuccess) return set_error(HAST_ERR_HIP, "%s: the blocked inflate failed: %s", z->path.c_str(), hipGetErrorString(hipGetLastError()));
            float up_ms = 0, k_ms = 0;
            if (hipEventElapsedTime(&up_ms, S.ev_begin, S.ev_uploaded) != hipSuccess || hipEventElapsedTime(&k_ms, S.ev_uploaded, S.ev_done) != hipSuccess) (void)hipGetLastError();
            {
                std::lock_guard<std::mutex> lk(z->mu);
                z->bs.upload_s += up_ms * 1e-3;
                z->bs.kernels_s += k_ms * 1e-3;
            }
            z->have_cur = true;
            z->cur_pos = 0;
            z->cur_avail = it.out_bytes;
            z->cur_bad.clear();
            const uint32_t bad = S.h_first[0];
            if (bad != 0xFFFFFFFFu) {                         // the members in front of the first refused one are delivered, nothing behind them
                const uint32_t why = S.h_first[1] & 0xFF;
                const size_t bi = std::min<size_t>(bad, it.n_members - 1);
                z->cur_avail = S.h_mem[bi].out_off;
                char msg[240];
                snprintf(msg, sizeof msg, "bgzf: the block at file offset %llu is damaged (%s)",
                         (unsigned long long)(it.file_off + (S.h_mem[bi].first_bit >> 3)), bad_text(why));
                z->cur_bad = msg;
            }
        }
        Slot &S = z->slot[z->cur.slot];
        const size_t n = (size_t)std::min<uint64_t>(z->cur_avail - z->cur_pos, cap - got);
        if (n && hipMemcpyAsync(d_dst + got, S.d_out + z->cur_pos, n, hipMemcpyDeviceToDevice, hs) != hipSuccess)
            return set_error(HAST_ERR_HIP, "hast_gz_read_device: copy failed: %s", hipGetErrorString(hipGetLastError()));
        got += n;
        z->cur_pos += n;
        z->delivered += n;
        if (z->cur_pos >= z->cur_avail) {
            // the batch is through: its slot is the producer's again once the caller's stream has run the copies.  ONE stream per
            // handle (include/hast.h): the event covers the copies of earlier calls out of this batch because they were put on the
            // same stream.  (A stream closed in mid-batch records nothing: its buffers are parked, and parked memory is not handed
            // out again before it is freed for real, which waits for the device.)
            if (hipEventRecord(S.ev_copied, hs) != hipSuccess) return set_error(HAST_ERR_HIP, "hipEventRecord failed");
            const int si = z->cur.slot;
            z->have_cur = false;
            if (!z->cur_bad.empty()) {
                // (the slot stays with the reader: the stream ends here, the producer may be anywhere)
                S.copied_recorded = true;
                z->err_status = HAST_ERR_IO;
                z->err = z->cur_bad;
                if (got) break;
                return set_error(z->err_status, "%s: %s", z->path.c_str(), z->err.c_str());
            }
            std::lock_guard<std::mutex> lk(z->mu);
            S.copied_recorded = true;
            z->slot_free[si] = true;
            z->cv.notify_all();
        }
    }
    *n_out = got;
    return HAST_OK;
}

void stream_stats(Stream *z, hast_gz_stats *gs, hast_gz_blocked_stats *bs) {
    std::lock_guard<std::mutex> lk(z->mu);
    if (gs) {
        memset(gs, 0, sizeof *gs);
        gs->compressed_bytes = z->file_size;
        gs->out_bytes = z->delivered;
        gs->members = z->bs.members;
        gs->open_s = z->open_s;
    }
    if (bs) *bs = z->bs;
}

void stream_close(Stream *z) {
    if (!z) return;
    {
        std::lock_guard<std::mutex> lk(z->mu);
        z->stop = true;
        z->cv.notify_all();
    }
    if (z->producer.joinable()) z->producer.join();
    (void)hipSetDevice(z->device);
    // batches in flight: the kernels and the reader's copies are let run to their end before the buffers go
    if (z->stream) (void)hipStreamSynchronize(z->stream);
    for (Slot &S : z->slot)
        if (S.copied_recorded) (void)hipEventSynchronize(S.ev_copied);
    for (Slot &S : z->slot) free_slot_buffers(S, z->in_cap + kInPad, z->batch_out + 16, z->mem_cap);
    if (z->stream) (void)hipStreamDestroy(z->stream);
    if (z->fd >= 0) close(z->fd);
    delete z;
}

}  // namespace bz
}  // namespace hast
