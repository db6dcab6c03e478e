// fq_feed.h -- one input file on its way to the GPU framer (hast_fq_*, include/hast.h), for the classify CLI.
//
// Both passes of the CLI over its inputs -- the classification pass and the routing pass of --phase-reads -- move a file's bytes
// the same way: a reader thread fills the buffers the stream hands out (pread / host inflate into pinned memory, or
// hast_gz_read_device into a block on the device), the main thread submits what is filled and opens the blocks whose framing has
// arrived.  That is all here, once: the wake-up the threads share, the feed of one file, its reader thread and the two steps of the
// main thread's loop that do not depend on what a pass does with an open block.
//
// Host only: nothing but include/hast.h, ingest.h and the standard library.  Nothing here ends the process: a failure comes back as
// a status and a message, and the caller decides.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <utility>

#include "../../include/hast.h"
#include "ingest.h"
#include "switches.h"

namespace hast {

// What the main thread sleeps on when nothing moved: readers (and a pass's own threads) wake it when they have produced something.
// A GPU event may be what it waits for instead, hence the timed wait.  wait() is the main thread's alone.
class FeedWake {
  public:
    void wake() {
        {
            std::lock_guard<std::mutex> g(mu_);
            ++gen_;
        }
        cv_.notify_one();
    }
    void wait(long microseconds) {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait_for(g, std::chrono::microseconds(microseconds), [this] { return gen_ != seen_; });
        seen_ = gen_;
    }

  private:
    std::mutex mu_;
    std::condition_variable cv_;
    uint64_t gen_ = 0, seen_ = 0;
};

enum class FeedStatus {
    ok,
    input_failed,        // the file: a read error, a damaged .gz -- the message names the file
    library_failed,      // a hast_fq_* call: the message says which step, hast_last_error() has the rest
};

inline bool feed_trace_blocks() {                     // HAST_TRACE_BLOCKS: a line on stderr per fill and per submit
    static const bool on = sw::flag(sw::HAST_TRACE_BLOCKS);
    return on;
}
inline double feed_now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct FqFeed {
    std::string name;
    size_t file_index = 0;
    BlockSource src;                                       // the bytes of a file the host reads (opened by the caller, threaded = false)
    hast_fq *fq = nullptr;
    hast_gz *gz = nullptr;                                 // the file is inflated on the GPU instead: blocks are filled there
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<uint8_t *, hast_stream>> empty;   // acquired, waiting for the reader (device blocks: the stream their writes go on)
    struct Filled { size_t n; bool last; std::string err; };
    std::deque<Filled> filled;                             // filled, in order, waiting for hast_fq_submit
    bool stop = false, eof_acquired = false;
    size_t held = 0;                                       // acquired and not yet committed: the caller takes one off per hast_fq_commit
    size_t acquired = 0, submitted = 0;
    size_t opened = 0;                                     // the caller adds one per block it opens (hast_fq_next / hast_fq_next_routed)
    size_t cap = 0, n_buffers = 0;                         // bytes per block; buffers of the stream over all its lanes

    const char *short_name() const { return name.c_str() + (name.size() > 5 ? name.size() - 5 : 0); }

    // `fq` (and `gz` or `src`) are set: starts the reader thread.  n_buf is the stream's buffer count per context.
    FeedStatus start(FeedWake &wake, size_t block_bytes, int n_buf, std::string &what) {
        if (hast_fq_block_bytes(fq) != block_bytes) {
            what = "internal: a stream's block size is not its input's";
            return FeedStatus::library_failed;
        }
        cap = block_bytes;
        n_buffers = (size_t)n_buf * (size_t)hast_fq_lanes(fq);
        th = std::thread([this, &wake] { read_blocks(wake); });
        return FeedStatus::ok;
    }

    // "At most n_buffers - 1 blocks may be in hand (hast_fq_device_block called, not yet submitted) at a time." (include/hast.h) --
    // and no stream has more than n_buffers between hast_fq_acquire and hast_fq_commit.
    bool may_acquire() const { return !eof_acquired && held < n_buffers && (!gz || acquired - submitted + 1 < n_buffers); }

    // Hands empty buffers to the reader and submits what it has filled (copy + framing run on the GPU from there on).  Returns
    // whether anything moved; a failure is in `st` and `what`, and nothing more should be asked of the feed then.
    bool pump(FeedStatus &st, std::string &what) {
        bool moved = false;
        auto failed = [&](FeedStatus s, std::string w) { st = s; what = std::move(w); return moved; };
        while (may_acquire()) {
            uint8_t *buf;
            hast_stream fill_stream = nullptr;
            if (hast_fq_acquire(fq, &buf) != HAST_OK) return failed(FeedStatus::library_failed, "staging a block");
            if (gz && hast_fq_device_block(fq, &buf, &fill_stream) != HAST_OK) return failed(FeedStatus::library_failed, "staging a block");
            held++;
            acquired++;
            std::lock_guard<std::mutex> g(mu);
            empty.push_back({buf, fill_stream});
            cv.notify_one();
            moved = true;
        }
        for (;;) {
            Filled fl;
            {
                std::lock_guard<std::mutex> g(mu);
                if (filled.empty()) break;
                fl = std::move(filled.front());
                filled.pop_front();
            }
            if (!fl.err.empty()) return failed(FeedStatus::input_failed, name + ": " + fl.err);
            if ((gz ? hast_fq_submit_device(fq, fl.n, fl.last ? 1 : 0) : hast_fq_submit(fq, fl.n, fl.last ? 1 : 0)) != HAST_OK)
                return failed(FeedStatus::library_failed, "framing a block");
            if (feed_trace_blocks()) fprintf(stderr, "trace %s submit at %.4f\n", short_name(), feed_now_s());
            submitted++;
            if (fl.last) eof_acquired = true;
            moved = true;
        }
        return moved;
    }

    // the record table (or the runs) of the oldest submitted block has arrived: opening it will not wait
    bool block_ready() const { return opened < submitted && hast_fq_poll(fq); }
    // every block of the file has been submitted and opened
    bool drained() const { return eof_acquired && opened == submitted; }

    void stop_reader() {                                   // also one that waits for a buffer
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }

  private:
    void read_blocks(FeedWake &wake) {
        for (;;) {
            uint8_t *buf;
            hast_stream fill_stream;
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [this] { return stop || !empty.empty(); });
                if (stop) return;
                buf = empty.front().first;
                fill_stream = empty.front().second;
                empty.pop_front();
            }
            Filled fl{0, false, std::string()};
            const double t0 = feed_trace_blocks() ? feed_now_s() : 0;
            if (gz) {                                      // (buf is a DEVICE address: the translate kernel writes the block there)
                size_t n = 0;
                if (hast_gz_read_device(gz, buf, cap, &n, fill_stream) != HAST_OK) fl.err = hast_last_error();
                else if (n < cap) {
                    // a short read is the end of the stream -- or what could be decoded in front of damage (delivered first, as
                    // gzread does): the next call says which.  Without it a file damaged behind its first pass would end here
                    // as if it were complete.
                    size_t more = 0;
                    if (hast_gz_read_device(gz, buf + n, cap - n, &more, fill_stream) != HAST_OK) fl.err = hast_last_error();
                    n += more;
                }
                fl.n = n;
            } else
                fl.n = src.read_into(reinterpret_cast<char *>(buf), cap, fl.err);
            if (feed_trace_blocks()) fprintf(stderr, "trace %s fill %.3f ms at %.4f\n", short_name(), (feed_now_s() - t0) * 1e3, feed_now_s());
            fl.last = fl.n < cap || !fl.err.empty();
            const bool last = fl.last;
            {
                std::lock_guard<std::mutex> g(mu);
                filled.push_back(std::move(fl));
            }
            wake.wake();
            if (last) return;
        }
    }
};

}  // namespace hast
