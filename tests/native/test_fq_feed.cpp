// Host-only test of hast_amd/csrc/fq_feed.h (no GPU, no libhast.so): the reader / submit / retire protocol that takes one input
// file to the GPU framer, against a fake stream in ordinary memory that fails the run when the caller breaks the contract of
// include/hast.h.  Built with -fsanitize=thread by tests/test_fq_feed_cpu.py.
//   test_fq_feed SCRATCH_DIR        (an empty directory the driver may write its input files to)
#include <pthread.h>
#include <time.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../hast_amd/csrc/fq_feed.h"

namespace {

constexpr size_t kBlock = 4096;

[[noreturn]] void fail(const std::string &what) {
    fprintf(stderr, "test_fq_feed: %s\n", what.c_str());
    fflush(stderr);
    _exit(1);                                      // (reader threads may be at work: no destructors)
}

std::string pattern(size_t n, unsigned seed) {
    std::string s(n, '\0');
    uint32_t x = 2463534242u + seed;
    for (size_t i = 0; i < n; i++) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        s[i] = (char)('A' + x % 26);
    }
    return s;
}

thread_local std::string g_last_error;

}  // namespace

// FeedWake::wait is condition_variable::wait_for, which libstdc++ turns into pthread_cond_clockwait on the steady clock.  The
// ThreadSanitizer runtime of GCC 11 has no interceptor for that call: it misses the unlock inside the wait and reports a double
// lock.  This definition takes its place in the driver only: the same deadline handed to pthread_cond_timedwait, which the runtime
// knows -- so the header's own wait path is what runs here, unchanged.
extern "C" int pthread_cond_clockwait(pthread_cond_t *cond, pthread_mutex_t *mutex, clockid_t clock, const struct timespec *abstime) {
    struct timespec now, real;
    clock_gettime(clock, &now);
    clock_gettime(CLOCK_REALTIME, &real);
    long long ns = (abstime->tv_sec - now.tv_sec) * 1000000000ll + (abstime->tv_nsec - now.tv_nsec);
    if (ns < 0) ns = 0;
    ns += real.tv_sec * 1000000000ll + real.tv_nsec;
    real.tv_sec = (time_t)(ns / 1000000000ll);
    real.tv_nsec = (long)(ns % 1000000000ll);
    return pthread_cond_timedwait(cond, mutex, &real);
}

// ---- the fake stream: what fq_feed.h calls of include/hast.h -------------------------------------------------------------------
struct hast_fq {
    int lanes = 1;
    bool device = false;
    int poll_delay = 2;                            // hast_fq_poll turns true only that many calls after the submit
    size_t n_total = 0;                            // n_buffers x lanes
    std::vector<std::vector<uint8_t>> bufs;        // handed out in ring order; "device" blocks live here as well
    size_t acquired = 0, device_blocks = 0, submitted = 0, opened = 0, committed = 0, n_last = 0;
    std::vector<size_t> ready_at;                  // per submitted block: the poll call from which on it is ready
    size_t poll_calls = 0;
    std::string got;                               // the submitted bytes, in order
    hast_fq(int n_buffers, int lanes_, bool device_) : lanes(lanes_), device(device_), n_total((size_t)n_buffers * (size_t)lanes_) {
        bufs.assign(n_total, std::vector<uint8_t>(kBlock));
    }
    void contract(bool ok, const char *what) const {
        if (!ok) fail(std::string("the caller broke the stream's contract: ") + what);
    }
    void submit(size_t n, int last) {
        contract(n_last == 0, "a submit after the last block");
        contract(submitted < acquired, "a submit without an acquire");
        contract(n <= kBlock, "more bytes than a block holds");
        contract(last || n == kBlock, "a block that is not the last one and not full");
        const std::vector<uint8_t> &b = bufs[submitted % n_total];
        got.append(reinterpret_cast<const char *>(b.data()), n);
        ready_at.push_back(poll_calls + (size_t)poll_delay);
        submitted++;
        if (last) n_last++;
    }
    void open_and_commit() {                       // what a pass does with a ready block comes down to this for the stream
        contract(opened < submitted, "a block opened that was not submitted");
        opened++;
        committed++;
    }
};
struct hast_gz {
    std::string data;
    size_t pos = 0;
    size_t first_call_bytes = ~(size_t)0;          // the first call delivers at most that many bytes ...
    bool then_error = false;                       // ... and the one behind it fails (damage) instead of finding the end
    size_t calls = 0;
};

extern "C" {
const char *hast_last_error(void) { return g_last_error.c_str(); }
int hast_fq_lanes(const hast_fq *q) { return q->lanes; }
size_t hast_fq_block_bytes(const hast_fq *) { return kBlock; }
hast_status hast_fq_acquire(hast_fq *q, uint8_t **host_buf) {
    q->contract(q->n_last == 0, "an acquire after the last block");
    q->contract(q->acquired - q->committed < q->n_total, "more buffers held than the stream has");
    *host_buf = q->device ? nullptr : q->bufs[q->acquired % q->n_total].data();
    q->acquired++;
    return HAST_OK;
}
hast_status hast_fq_device_block(hast_fq *q, uint8_t **d_block, hast_stream *fill_stream) {
    q->contract(q->device, "a device block of a stream of host blocks");
    q->contract(q->device_blocks < q->acquired, "a device block without an acquire");
    q->contract(q->device_blocks - q->submitted + 1 <= q->n_total - 1, "more than n_buffers - 1 device blocks in hand");
    *d_block = q->bufs[q->device_blocks % q->n_total].data();
    *fill_stream = nullptr;
    q->device_blocks++;
    return HAST_OK;
}
hast_status hast_fq_submit(hast_fq *q, size_t n, int last) {
    q->contract(!q->device, "a host submit on a stream of device blocks");
    q->submit(n, last);
    return HAST_OK;
}
hast_status hast_fq_submit_device(hast_fq *q, size_t n, int last) {
    q->contract(q->device && q->submitted < q->device_blocks, "a device submit without a device block");
    q->submit(n, last);
    return HAST_OK;
}
int hast_fq_poll(hast_fq *q) {
    q->poll_calls++;
    return q->opened < q->submitted && q->poll_calls >= q->ready_at[q->opened];
}
hast_status hast_gz_read_device(hast_gz *z, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream) {
    *n_out = 0;
    const size_t call = z->calls++;
    if (z->then_error && call >= 1) {
        g_last_error = "gz: damaged behind the first pass";
        return HAST_ERR_FORMAT;
    }
    size_t n = std::min(cap, z->data.size() - z->pos);
    if (call == 0) n = std::min(n, z->first_call_bytes);
    else if (z->first_call_bytes != ~(size_t)0) n = 0;
    memcpy(d_dst, z->data.data() + z->pos, n);
    z->pos += n;
    *n_out = n;
    return HAST_OK;
}
}

namespace {

struct Case {
    std::unique_ptr<hast::FqFeed> feed{new hast::FqFeed()};
    std::unique_ptr<hast_fq> fq;
    std::unique_ptr<hast_gz> gz;
    std::string expect;
};

std::string write_file(const std::string &dir, const std::string &name, const std::string &bytes) {
    const std::string path = dir + "/" + name;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) fail("cannot write " + path);
    return path;
}

// a feed over `bytes`: a plain file through BlockSource (path non-empty) or a fake device-inflated stream
std::unique_ptr<Case> make_case(const std::string &bytes, const std::string &path, int n_buffers, int lanes, hast::FeedWake &wake, bool start = true) {
    std::unique_ptr<Case> c(new Case());
    c->expect = bytes;
    const bool device = path.empty();
    c->fq.reset(new hast_fq(n_buffers, lanes, device));
    c->feed->name = device ? "device-inflated" : path;
    c->feed->fq = c->fq.get();
    if (device) {
        c->gz.reset(new hast_gz());
        c->gz->data = bytes;
        c->feed->gz = c->gz.get();
    } else if (!c->feed->src.open(path, kBlock, false)) fail("cannot open " + path);
    std::string what;
    if (start && c->feed->start(wake, kBlock, n_buffers, what) != hast::FeedStatus::ok) fail(what);
    return c;
}

struct Outcome {
    hast::FeedStatus st = hast::FeedStatus::ok;
    std::string what;
    size_t idle_waits = 0;
};

// the CLI's three-step loop; "opening a block" only counts
Outcome run(std::vector<Case *> active, hast::FeedWake &wake, bool slow_consumer) {
    Outcome out;
    for (size_t round = 0; !active.empty(); round++) {
        if (round > 5000000) fail("the loop does not end");
        bool progress = false;
        for (Case *c : active) {
            if (c->feed->pump(out.st, out.what)) progress = true;
            if (out.st != hast::FeedStatus::ok) {
                for (Case *a : active) a->feed->stop_reader();
                return out;
            }
        }
        for (size_t i = 0; i < active.size();) {
            hast::FqFeed &f = *active[i]->feed;
            if (f.block_ready()) {
                active[i]->fq->open_and_commit();
                f.opened++;
                f.held--;
                if (slow_consumer) std::this_thread::sleep_for(std::chrono::microseconds(200));
                progress = true;
            }
            if (f.drained()) {
                f.stop_reader();
                active.erase(active.begin() + (long)i);
                progress = true;
                continue;
            }
            ++i;
        }
        if (!progress) {
            out.idle_waits++;
            wake.wait(100);
        }
    }
    return out;
}

void check_arrived(const Case &c, const std::string &label) {
    if (c.fq->got != c.expect) fail(label + ": what was submitted is not the file (" + std::to_string(c.fq->got.size()) + " bytes of " + std::to_string(c.expect.size()) + ")");
    if (c.fq->n_last != 1) fail(label + ": " + std::to_string(c.fq->n_last) + " blocks carried `last`");   // (nothing behind it: the fake refuses that)
    if (c.fq->opened != c.fq->submitted) fail(label + ": blocks left unopened");       // (buffers handed out ahead of the end stay out)
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) fail("usage: test_fq_feed SCRATCH_DIR");
    const std::string dir = argv[1];
    size_t n_cases = 0;

    // every length around a block border, host-read and device-inflated, every buffer count and lane count
    const size_t lengths[] = {0, 1, 4095, 4096, 4097, 5 * 4096, 5 * 4096 + 17};
    for (size_t len : lengths) {
        const std::string bytes = pattern(len, (unsigned)len);
        const std::string path = write_file(dir, "plain_" + std::to_string(len), bytes);
        for (int device = 0; device < 2; device++)
            for (int n_buffers : {2, 3, 6})
                for (int lanes : {1, 3}) {
                    hast::FeedWake wake;
                    std::unique_ptr<Case> c = make_case(bytes, device ? "" : path, n_buffers, lanes, wake);
                    const Outcome o = run({c.get()}, wake, false);
                    const std::string label = std::string(device ? "device" : "plain") + " len " + std::to_string(len) + " buffers " + std::to_string(n_buffers) + " lanes " + std::to_string(lanes);
                    if (o.st != hast::FeedStatus::ok) fail(label + ": " + o.what);
                    check_arrived(*c, label);
                    n_cases++;
                }
    }

    // an inflate that comes up short and then finds the end: a clean end of file
    {
        hast::FeedWake wake;
        const std::string bytes = pattern(5000, 7);
        std::unique_ptr<Case> c = make_case(bytes, "", 3, 1, wake);
        c->gz->first_call_bytes = 100;
        c->expect = bytes.substr(0, 100);
        const Outcome o = run({c.get()}, wake, false);
        if (o.st != hast::FeedStatus::ok) fail("short read, then the end: " + o.what);
        check_arrived(*c, "short read, then the end");
        n_cases++;
    }
    // an inflate that comes up short and then fails: damage, reported, and the short block never submitted
    {
        hast::FeedWake wake;
        std::unique_ptr<Case> c = make_case(pattern(5000, 8), "", 3, 1, wake);
        c->gz->first_call_bytes = 100;
        c->gz->then_error = true;
        const Outcome o = run({c.get()}, wake, false);
        if (o.st != hast::FeedStatus::input_failed) fail("short read, then damage: not reported as the input's failure");
        if (o.what != "device-inflated: gz: damaged behind the first pass") fail("short read, then damage: the message is '" + o.what + "'");
        if (c->fq->submitted != 0) fail("short read, then damage: the short block was submitted");
        n_cases++;
    }
    // a read error of the host's source (a directory opens and cannot be read): reported, not an end of file
    {
        hast::FeedWake wake;
        std::unique_ptr<Case> c = make_case("", dir, 3, 1, wake);
        const Outcome o = run({c.get()}, wake, false);
        if (o.st != hast::FeedStatus::input_failed) fail("read error: taken for the end of the file");
        if (o.what.compare(0, dir.size() + 2, dir + ": ") != 0 || o.what.size() <= dir.size() + 2) fail("read error: the message is '" + o.what + "'");
        if (c->fq->submitted != 0) fail("read error: a block was submitted");
        n_cases++;
    }
    // four feeds on one wake-up object, a slow consumer, a stream whose blocks take long to be ready
    {
        hast::FeedWake wake;
        std::vector<std::unique_ptr<Case>> cs;
        std::vector<Case *> active;
        for (int i = 0; i < 4; i++) {
            const std::string bytes = pattern(7 * kBlock + 123 * (size_t)i, 100 + (unsigned)i);
            const bool device = i & 1;
            cs.push_back(make_case(bytes, device ? "" : write_file(dir, "multi_" + std::to_string(i), bytes), 2 + i % 2, 1 + 2 * (i / 2), wake));
            cs.back()->fq->poll_delay = 5;
            active.push_back(cs.back().get());
        }
        const Outcome o = run(active, wake, true);
        if (o.st != hast::FeedStatus::ok) fail("four feeds: " + o.what);
        for (int i = 0; i < 4; i++) check_arrived(*cs[(size_t)i], "four feeds, feed " + std::to_string(i));
        if (o.idle_waits == 0) fail("four feeds: the idle wait was never entered");
        n_cases++;
    }
    // stopping a feed whose reader waits for a buffer: before it was given one, and after it has filled all there are
    {
        hast::FeedWake wake;
        const std::string bytes = pattern(20 * kBlock, 9);
        const std::string path = write_file(dir, "stopped", bytes);
        std::unique_ptr<Case> never_fed = make_case(bytes, path, 3, 1, wake);
        never_fed->feed->stop_reader();
        std::unique_ptr<Case> c = make_case(bytes, path, 3, 1, wake);
        hast::FeedStatus st = hast::FeedStatus::ok;
        std::string what;
        for (size_t round = 0; c->fq->submitted < 3; round++) {             // every buffer out, filled and submitted; none comes back
            if (round > 5000000) fail("stop: the buffers were never filled");
            if (!c->feed->pump(st, what)) wake.wait(100);
            if (st != hast::FeedStatus::ok) fail("stop: " + what);
        }
        c->feed->stop_reader();
        if (c->fq->got != bytes.substr(0, 3 * kBlock)) fail("stop: the first blocks are not the file's");
        n_cases++;
    }
    // a stream whose block size is not the input's is refused before a thread is started
    {
        hast::FeedWake wake;
        std::unique_ptr<Case> c = make_case("", "", 3, 1, wake, false);
        std::string what;
        if (c->feed->start(wake, 2 * kBlock, 3, what) != hast::FeedStatus::library_failed || what.empty()) fail("a wrong block size was accepted");
        n_cases++;
    }
    printf("ok %zu cases\n", n_cases);
    return 0;
}
