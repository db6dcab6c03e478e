// fake_10x -- drop-in for HAST's 02.assemble_by_supernova/fake_10x.pl: stLFR read pairs -> 10x FASTQ for Supernova.
//   fake_10x READ1.gz READ2.gz MERGE.txt [--inflate host|zlib|device] [--block-mb N] [--plain-out] [--stats]
//            [--convert host|device] [--deflate host|device]
// writes SampleName_S1_L001_R1_001.fastq.gz and SampleName_S1_L001_R2_001.fastq.gz into the working directory and prints the
// script's stdout.  A host program: the inputs come through ingest.h (ordinary gzip inflated by several threads, BGZF, pipes, plain
// FASTQ), a block of each at a time; the whole pairs of what has been read go through the model of the script
// (hast_tx_pair_host, include/hast.h "stage 02"), what is left is carried in front of the next block; both outputs leave as one
// zlib gzip member per step, deflated side by side.  Memory stays at a few blocks whatever the inputs' lengths: when read 2 ends
// first, the rest of read 1 is still converted block by block, as the script pairs it with nothing.
// --convert device: the steps over whole pairs go to the GPU (hast_tx_pair_staged: upload through pinned staging, the kernels of
// tx_kernels.hip, with --deflate device -- the default then -- one gzip member per side and step from the GPU's encoder, download);
// one writer thread per output file writes step n beside step n + 1 (and deflates it, with --deflate host).  The steps at the end of
// the inputs, a step larger than the converter was created for and one whose outputs outgrow their room are the host model's.  A
// map the device cannot take (hast_tx_map_info.device_ok == 0) sends the whole run the host way, with one WARN line.
// --convert device --inflate device: the inputs do not pass through host memory at all (hast_tx_feed_*, include/hast.h): a .gz input is
// inflated on the GPU (hast_gz_read_device) straight into the feed's block in HBM -- an input hast_gz_open cannot take (plain FASTQ, a
// pipe) goes through ingest.h into the feed's pinned block and is uploaded -- the feed says who reads (the rule above, from the counts
// the step before left, tx_feed_plan.h), converts, and deflates and downloads step n while step n + 1 is read and converted.  The steps
// are the same steps; when an input has ended and left no whole record, or a record is longer than the feed's buffers, the bytes the
// feed still holds come down and the host loop above ends the run (a .gz still open on the GPU is read through a device buffer).
// Exit codes: 0 done; 1 usage; 2 an input that cannot be opened, or a .gz that is damaged or fails its CRC; 3 a failing library
// call or write; 4 --convert device without a usable GPU, or a failing GPU call.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hast.h"
#include "cli_common.h"
#include "ingest.h"

namespace {

struct Options {
    std::string in[2], map;
    bool plain_out = false, stats = false;
    std::string inflate = "host", convert = "host", deflate;      // deflate: "" = host, or device with --convert device
    size_t block = 16u << 20;
};

using hast::now_s;
namespace sw = hast::sw;

int usage() {
    fprintf(stderr, "usage: fake_10x READ1.gz READ2.gz MERGE.txt [--inflate host|zlib|device] [--block-mb N] [--plain-out] [--stats]\n"
                    "                [--convert host|device] [--deflate host|device]\n");
    return 1;
}

struct Outputs {
    FILE *f[2] = {nullptr, nullptr};
    bool plain = false;
    uint64_t bytes[2] = {0, 0};
    bool open(bool plain_out) {
        plain = plain_out;
        const char *names[2] = {"SampleName_S1_L001_R1_001.fastq", "SampleName_S1_L001_R2_001.fastq"};
        for (int s = 0; s < 2; ++s) {
            f[s] = fopen((std::string(names[s]) + (plain ? "" : ".gz")).c_str(), "wb");
            if (!f[s]) return false;
        }
        return true;
    }
    bool write(int s, const uint8_t *p, size_t n) {
        bytes[s] += n;
        return n == 0 || fwrite(p, 1, n, f[s]) == n;
    }
    // a run of converted records: as it is, or as one zlib gzip member (nothing for an empty run); zlib is fed pieces it can count
    bool write_host(int s, const uint8_t *p, size_t n) {
        if (plain || n == 0) return write(s, p, n);
        z_stream z;
        memset(&z, 0, sizeof z);
        if (deflateInit2(&z, 6, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        std::vector<uint8_t> out(1u << 20);
        bool ok = true;
        for (size_t at = 0; ok;) {
            const size_t piece = std::min<size_t>(n - at, 1u << 30);
            z.next_in = const_cast<uint8_t *>(p + at);
            z.avail_in = (uInt)piece;
            at += piece;
            int r;
            do {
                z.next_out = out.data();
                z.avail_out = (uInt)out.size();
                r = deflate(&z, at == n ? Z_FINISH : Z_NO_FLUSH);
                ok = r != Z_STREAM_ERROR && write(s, out.data(), out.size() - z.avail_out);
            } while (ok && z.avail_out == 0);
            if (at == n) {
                ok = ok && r == Z_STREAM_END;
                break;
            }
        }
        deflateEnd(&z);
        return ok;
    }
    // both outputs of a host step, deflated side by side (the script pipes its outputs through two gzip processes)
    bool write_host_both(uint8_t *const o[2], const uint64_t n[2]) {
        bool ok1 = true;
        std::thread side1([&] { ok1 = write_host(1, o[1], (size_t)n[1]); });
        const bool ok0 = write_host(0, o[0], (size_t)n[0]);
        side1.join();
        return ok0 && ok1;
    }
    bool close() {
        bool ok = true;
        for (int s = 0; s < 2; ++s)
            if (f[s] && fclose(f[s]) != 0) ok = false;
        return ok;
    }
};

// The writer of one output file (--convert device): takes one run at a time and writes it while the next step is converted.  submit
// waits until the run before has been written, so the memory of run n is free again once run n + 1 has been handed over.
struct Writer {
    struct Job {
        const uint8_t *p = nullptr;
        size_t n = 0;
        bool deflate = false;      // through zlib first (write_host), or as it is
        void *free_me = nullptr;   // a host step's output: hast_tx_free once written
    };
    Outputs *out = nullptr;
    int side = 0;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    Job job;
    bool have = false, quit = false, ok = true;
    double busy = 0;
    void start(Outputs *o, int s) {
        out = o;
        side = s;
        th = std::thread([this] {
            std::unique_lock<std::mutex> lk(mu);
            for (;;) {
                cv.wait(lk, [this] { return have || quit; });
                if (!have) return;
                const Job j = job;
                lk.unlock();
                const double t0 = now_s();
                const bool good = j.deflate ? out->write_host(side, j.p, j.n) : out->write(side, j.p, j.n);
                if (j.free_me) hast_tx_free(j.free_me);
                lk.lock();
                busy += now_s() - t0;
                ok = ok && good;
                have = false;
                cv.notify_all();
            }
        });
    }
    // false: a run before this one could not be written; this one is dropped (and freed), the run ends
    bool submit(const Job &j) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return !have; });
        if (!ok) {
            if (j.free_me) hast_tx_free(j.free_me);
            return false;
        }
        job = j;
        have = true;
        cv.notify_all();
        return true;
    }
    bool stop() {                  // everything handed over has been written
        if (!th.joinable()) return ok;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this] { return !have; });
            quit = true;
            cv.notify_all();
        }
        th.join();
        return ok;
    }
};

struct Input {
    std::string path;
    hast::BlockSource src;
    bool eof = false;
    // --inflate device: a .gz that is inflated on the GPU; the host loop reads it through a device buffer of a block and a download
    hast_gz *gz = nullptr;
    hast_ctx *ctx = nullptr;
    uint8_t *d_bounce = nullptr;
    bool gpu_failed = false;       // the trouble is a failing GPU call, not the input's
    size_t read(char *dst, size_t cap, std::string &trouble) {
        if (!gz) return src.read_into(dst, cap, trouble);
        size_t got = 0;
        while (got < cap) {        // a short read is followed by another until one returns nothing (include/hast.h)
            size_t n = 0;
            const hast_status st = hast_gz_read_device(gz, d_bounce + got, cap - got, &n, nullptr);
            if (st != HAST_OK) {
                trouble = hast_last_error();
                gpu_failed = st != HAST_ERR_IO;
                return 0;
            }
            if (!n) break;
            got += n;
        }
        if (got && (hast_stream_sync(ctx, nullptr) != HAST_OK || hast_memcpy_d2h(ctx, dst, d_bounce, got) != HAST_OK)) {
            trouble = hast_last_error();
            gpu_failed = true;
            return 0;
        }
        return got;
    }
};

struct Run {
    Options o;
    hast_tx_map *map = nullptr;
    hast_tx_map_info info{};
    hast_tx_state st{0, 0};
    Outputs out;
    uint64_t steps = 0, plain_in = 0;
    // --convert device
    hast_ctx *ctx = nullptr;
    hast_tx *tx = nullptr;         // null: every step is the host model's
    std::string fallback = "none";
    hast_tx_times times{0, 0, 0, 0};
    uint64_t pairs_device = 0, pairs_host = 0;
    Writer writer[2];
    double write_s = 0;
    // --inflate device
    hast_tx_feed *feed = nullptr;  // null: the inputs are inflated on the host
    int gz_on_device = 0, host_sides = 0;
    uint64_t steps_on_host = 0;
    std::string feed_fallback = "none";
};

void progress(uint64_t before, uint64_t after) {
    for (uint64_t mb = before / 1000000 + 1; mb * 1000000 <= after; ++mb) printf("process %llu (Mb) pair of reads now  \n", (unsigned long long)mb);
}

int fail_lib(const char *what) {
    fprintf(stderr, "fake_10x: %s: %s\n", what, hast_last_error());
    return 3;
}

bool has_record(const std::vector<uint8_t> &v) {
    size_t at = 0;
    for (int lines = 0; lines < 4; ++lines) {
        const void *nl = at < v.size() ? memchr(v.data() + at, '\n', v.size() - at) : nullptr;
        if (!nl) return false;
        at = (size_t)(static_cast<const uint8_t *>(nl) - v.data()) + 1;
    }
    return true;
}

// The program's loop.  have[]: per side, what the step before left + the block just read.  read_done: the reads of the first step have
// been made (the device feed hands over in the middle of a step: have[] is what that step was given).
int host_loop(Run &r, Input in[2], std::vector<uint8_t> have[2], bool read_done) {
    std::string trouble;
    for (int mode = 0; mode != 1; read_done = false) {
        // a side that has more than a block waiting, a whole record in it, reads nothing: the other side has to catch up
        for (int s = 0; s < 2 && !read_done; ++s) {
            if (in[s].eof || (have[s].size() > r.o.block && has_record(have[s]))) continue;
            const size_t at = have[s].size();
            have[s].resize(at + r.o.block);
            const size_t n = in[s].read(reinterpret_cast<char *>(have[s].data() + at), r.o.block, trouble);
            have[s].resize(at + n);
            r.plain_in += n;
            if (!trouble.empty()) {
                fprintf(stderr, "fake_10x: %s: %s\n", in[s].path.c_str(), trouble.c_str());
                return in[s].gpu_failed ? 4 : 2;
            }
            if (n < r.o.block) in[s].eof = true;
        }
        // 0: the whole pairs; 2: read 2 has ended, the whole records of read 1 pair with nothing; 1: the inputs end here
        mode = hast_tx_step_mode(in[0].eof, in[1].eof, have[0].data(), have[0].size(), have[1].data(), have[1].size());
        uint8_t *o[2] = {nullptr, nullptr};
        hast_tx_result res;
        const uint64_t before = r.st.headers;
        bool on_device = false;
        if (r.tx && mode == 0) {
            const bool gz = !r.o.plain_out && r.o.deflate == "device";
            const uint8_t *p[2];
            const hast_status st = hast_tx_pair_staged(r.tx, have[0].data(), have[0].size(), have[1].data(), have[1].size(), &r.st, gz, &p[0], &p[1], &res, &r.times);
            if (st == HAST_OK) {
                on_device = true;
                for (int s = 0; s < 2; ++s) {
                    Writer::Job j;
                    j.p = p[s];
                    j.n = (size_t)res.out_bytes[s];
                    j.deflate = !r.o.plain_out && !gz;
                    if (!r.writer[s].submit(j)) {
                        fprintf(stderr, "fake_10x: cannot write the outputs\n");
                        return 3;
                    }
                }
            } else if (st != HAST_ERR_UNSUPPORTED) {
                fprintf(stderr, "fake_10x: the conversion on the device: %s\n", hast_last_error());
                return 4;
            }
        }
        if (!on_device && hast_tx_pair_host(r.map, have[0].data(), have[0].size(), have[1].data(), have[1].size(), mode, &r.st, &o[0], &o[1], &res) != HAST_OK)
            return fail_lib("the conversion");
        progress(before, r.st.headers);
        ++r.steps;
        (on_device ? r.pairs_device : r.pairs_host) += res.pairs;
        bool ok = true;
        if (on_device) {
        } else if (r.tx) {                                         // behind the runs the writers still hold, in order
            for (int s = 0; s < 2; ++s) {
                Writer::Job j;
                j.p = o[s];
                j.n = (size_t)res.out_bytes[s];
                j.deflate = !r.o.plain_out;
                j.free_me = o[s];
                if (!r.writer[s].submit(j)) ok = false;          // (the other side's run is still handed over, or freed there)
            }
        } else {
            ok = r.out.write_host_both(o, res.out_bytes);
            hast_tx_free(o[0]);
            hast_tx_free(o[1]);
        }
        if (!ok) {
            fprintf(stderr, "fake_10x: cannot write the outputs\n");
            return 3;
        }
        have[0].erase(have[0].begin(), have[0].begin() + (size_t)res.consumed1);
        have[1].erase(have[1].begin(), have[1].begin() + (size_t)res.consumed2);
    }
    return 0;
}

int run(Run &r) {
    Input in[2];
    for (int s = 0; s < 2; ++s) {
        in[s].path = r.o.in[s];
        if (!in[s].src.open(in[s].path, r.o.block, false)) {
            fprintf(stderr, "fake_10x: cannot open %s\n", in[s].path.c_str());
            return 2;
        }
    }
    std::vector<uint8_t> have[2];
    return host_loop(r, in, have, false);
}

int fail_gpu(const char *what) {
    fprintf(stderr, "fake_10x: %s: %s\n", what, hast_last_error());
    return 4;
}

// --convert device --inflate device: the steps of host_loop with the bytes in HBM (hast_tx_feed_*).  Step n + 1 is read and converted
// before step n is collected, so the GPU deflates n meanwhile; the collected runs go to the writers in order.
int feed_loop(Run &r, Input in[2], std::vector<uint8_t> have[2], bool *read_done) {
    const size_t block = r.o.block;
    const bool writer_deflates = !r.o.plain_out && r.o.deflate != "device";
    std::string trouble;
    auto collect = [&]() -> int {
        const uint8_t *p[2];
        uint64_t n_out[2], n_raw[2];
        if (hast_tx_feed_collect(r.feed, &p[0], &p[1], n_out, n_raw) != HAST_OK) return fail_gpu("the conversion on the device");
        for (int s = 0; s < 2; ++s) {
            Writer::Job j;
            j.p = p[s];
            j.n = (size_t)n_out[s];
            j.deflate = writer_deflates;
            if (!r.writer[s].submit(j)) {
                fprintf(stderr, "fake_10x: cannot write the outputs\n");
                return 3;
            }
        }
        return 0;
    };
    bool waiting = false;          // a step has been made and not collected
    int flags = 0;
    for (;;) {
        for (int s = 0; s < 2; ++s) {
            if (!hast_tx_feed_wants(r.feed, s)) continue;
            size_t got = 0;
            if (in[s].gz) {
                uint8_t *d = nullptr;
                hast_stream fill = nullptr;
                if (hast_tx_feed_device_block(r.feed, s, &d, &fill) != HAST_OK) return fail_gpu("the feed");
                while (got < block) {          // a short read is followed by another until one returns nothing (include/hast.h)
                    size_t n = 0;
                    const hast_status st = hast_gz_read_device(in[s].gz, d + got, block - got, &n, fill);
                    if (st == HAST_ERR_IO) {
                        fprintf(stderr, "fake_10x: %s\n", hast_last_error());
                        return 2;
                    }
                    if (st != HAST_OK) return fail_gpu("the inflate on the device");
                    if (!n) break;
                    got += n;
                }
            } else {
                uint8_t *h = nullptr;
                if (hast_tx_feed_host_block(r.feed, s, &h) != HAST_OK) return fail_gpu("the feed");
                got = in[s].src.read_into(reinterpret_cast<char *>(h), block, trouble);
                if (!trouble.empty()) {
                    fprintf(stderr, "fake_10x: %s: %s\n", in[s].path.c_str(), trouble.c_str());
                    return 2;
                }
            }
            if (hast_tx_feed_submit(r.feed, s, got) != HAST_OK) return fail_gpu("the feed");
            r.plain_in += got;
            if (got < block) in[s].eof = true;
        }
        hast_tx_result res;
        const uint64_t before = r.st.headers;
        if (hast_tx_feed_step(r.feed, &r.st, &res, &flags) != HAST_OK) return fail_gpu("the conversion on the device");
        if (flags & (int)HAST_TX_ENDS) break;                    // nothing was converted: this step is the host loop's first
        progress(before, r.st.headers);
        ++r.steps;
        if (flags & (int)HAST_TX_ON_HOST) {
            ++r.steps_on_host;
            r.pairs_host += res.pairs;
        } else {
            r.pairs_device += res.pairs;
        }
        if (waiting)
            if (const int rc = collect()) return rc;
        waiting = true;
        if (flags & (int)HAST_TX_TAIL_TOO_LONG) break;
    }
    if (waiting)
        if (const int rc = collect()) return rc;
    // the host loop ends the run over what the feed still holds
    for (int s = 0; s < 2; ++s) {
        have[s].resize(hast_tx_feed_room(r.feed));
        size_t n = 0;
        if (hast_tx_feed_take_tail(r.feed, s, have[s].data(), &n) != HAST_OK) return fail_gpu("the feed");
        have[s].resize(n);
        if (in[s].gz && !in[s].eof) {
            void *d = nullptr;
            if (hast_dev_alloc(r.ctx, block + 64, &d) != HAST_OK) return fail_gpu("a device buffer of a block");
            in[s].d_bounce = static_cast<uint8_t *>(d);
        }
    }
    *read_done = (flags & (int)HAST_TX_ENDS) != 0;
    return 0;
}

int run_feed(Run &r) {
    Input in[2];
    int rc = 0;
    for (int s = 0; s < 2 && !rc; ++s) {
        in[s].path = r.o.in[s];
        in[s].ctx = r.ctx;
        const hast_status st = hast_gz_open(r.ctx, in[s].path.c_str(), &in[s].gz);
        if (st == HAST_OK) {
            ++r.gz_on_device;
        } else if (st == HAST_ERR_UNSUPPORTED) {                 // plain FASTQ, a pipe, no room: this side comes through the host
            in[s].gz = nullptr;
            ++r.host_sides;
            if (!in[s].src.open(in[s].path, r.o.block, false)) {
                fprintf(stderr, "fake_10x: cannot open %s\n", in[s].path.c_str());
                rc = 2;
            }
        } else if (st == HAST_ERR_IO) {
            fprintf(stderr, "fake_10x: cannot open %s: %s\n", in[s].path.c_str(), hast_last_error());
            rc = 2;
        } else {
            rc = fail_gpu("hast_gz_open");
        }
    }
    std::vector<uint8_t> have[2];
    bool read_done = false;
    if (!rc) rc = feed_loop(r, in, have, &read_done);
    if (!rc) rc = host_loop(r, in, have, read_done);
    for (int s = 0; s < 2; ++s) {
        if (in[s].gz) hast_gz_close(in[s].gz);
        if (in[s].d_bounce) hast_dev_free(r.ctx, in[s].d_bounce);
    }
    return rc;
}

}  // namespace

int main(int argc, char **argv) {
    Run r;
    std::vector<std::string> pos;
    bool block_given = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto value = [&]() -> const char * { return i + 1 < argc ? argv[++i] : nullptr; };
        if (a == "--inflate") { const char *v = value(); if (!v || (strcmp(v, "host") && strcmp(v, "zlib") && strcmp(v, "device"))) return usage(); r.o.inflate = v; }
        else if (a == "--block-mb") { const char *v = value(); if (!v || atoi(v) < 1 || atoi(v) > 1024) return usage(); r.o.block = (size_t)atoi(v) << 20; block_given = true; }
        else if (a == "--convert") { const char *v = value(); if (!v || (strcmp(v, "host") && strcmp(v, "device"))) return usage(); r.o.convert = v; }
        else if (a == "--deflate") { const char *v = value(); if (!v || (strcmp(v, "host") && strcmp(v, "device"))) return usage(); r.o.deflate = v; }
        else if (a == "--plain-out") r.o.plain_out = true;
        else if (a == "--stats") r.o.stats = true;
        else if (a.size() > 1 && a[0] == '-' && a[1] == '-') return usage();
        else pos.push_back(a);
    }
    if (pos.size() != 3) return usage();
    if (r.o.deflate == "device" && r.o.convert != "device") return usage();      // (the encoder takes device memory)
    if (r.o.inflate == "device" && r.o.convert != "device") return usage();      // (the inflated bytes stay in device memory)
    if (r.o.deflate.empty()) r.o.deflate = r.o.convert;
    r.o.in[0] = pos[0];
    r.o.in[1] = pos[1];
    r.o.map = pos[2];
    if (!block_given) sw::size(sw::HAST_TX_BLOCK, &r.o.block);         // tests: blocks of a few KB
    if (r.o.inflate == "zlib") setenv("HAST_INFLATE", "zlib", 1);
    printf("Merge stLFR reads into 10X format !\n read1 :  %s \n. read2 : %s \n map file : %s\n", pos[0].c_str(), pos[1].c_str(), pos[2].c_str());
    fflush(stdout);
    if (hast_tx_map_load(r.o.map.c_str(), &r.map, &r.info) != HAST_OK) {
        fprintf(stderr, "fake_10x: %s\n", hast_last_error());
        return 2;
    }
    if (r.o.convert == "device" && !r.info.device_ok) {
        fprintf(stderr, "WARN: fake_10x: the map cannot go to the device (%s): converting on the host\n", r.info.reason);
        r.fallback = r.info.reason;
        std::replace(r.fallback.begin(), r.fallback.end(), ' ', '_');
    } else if (r.o.convert == "device") {
        // a step holds what the step before left and a block: two blocks in all but odd cases; at least 1 MB, so that records far
        // larger than a small block still go to the device; at most what 32-bit offsets allow
        const size_t max_in = std::min<size_t>(std::max<size_t>(2 * r.o.block + 4096, 1u << 20), 128u << 20);
        if (hast_ctx_create(0, 21, &r.ctx) != HAST_OK || hast_tx_create(r.ctx, r.map, max_in, &r.tx) != HAST_OK) {
            fprintf(stderr, "fake_10x: --convert device: %s\n", hast_last_error());
            return 4;
        }
        if (r.o.inflate == "device") {
            const hast_status st = hast_tx_feed_create(r.tx, r.o.block, !r.o.plain_out && r.o.deflate == "device", &r.feed);
            if (st == HAST_ERR_UNSUPPORTED) {
                fprintf(stderr, "WARN: fake_10x: --inflate device cannot take blocks of %zu bytes: inflating on the host\n", r.o.block);
                r.feed_fallback = "block_too_large";
            } else if (st != HAST_OK) {
                fprintf(stderr, "fake_10x: --inflate device: %s\n", hast_last_error());
                return 4;
            }
        }
    }
    if (r.o.inflate == "device" && !r.tx) r.feed_fallback = r.fallback;
    if (!r.feed) r.host_sides = 2;
    if (!r.out.open(r.o.plain_out)) {
        fprintf(stderr, "fake_10x: cannot create the outputs in the working directory\n");
        return 3;
    }
    const double t0 = now_s();
    if (r.tx)
        for (int s = 0; s < 2; ++s) r.writer[s].start(&r.out, s);
    int rc = r.feed ? run_feed(r) : run(r);
    for (int s = 0; s < 2; ++s) {
        if (!r.writer[s].stop() && !rc) {
            fprintf(stderr, "fake_10x: cannot write the outputs\n");
            rc = 3;
        }
        r.write_s += r.writer[s].busy;
    }
    const bool closed = r.out.close();
    double collect_wait = 0;
    if (r.feed) hast_tx_feed_times(r.feed, &r.times, &collect_wait);
    hast_tx_feed_destroy(r.feed);
    hast_tx_destroy(r.tx);
    if (r.ctx) hast_ctx_destroy(r.ctx);
    hast_tx_map_destroy(r.map);
    if (rc) return rc;
    if (!closed) {
        fprintf(stderr, "fake_10x: cannot write the outputs\n");
        return 3;
    }
    printf("Total %llu pair reads and used %llu pairs.\n", (unsigned long long)r.st.headers, (unsigned long long)r.st.used);
    if (r.o.stats && r.o.convert == "device") {
        fprintf(stderr, "[stats] transform device: steps=%llu pairs_on_device=%llu pairs_on_host=%llu fallback=%s\n", (unsigned long long)r.steps,
                (unsigned long long)r.pairs_device, (unsigned long long)r.pairs_host, r.fallback.c_str());
        fprintf(stderr, "[stats] seconds: upload=%.3f kernels=%.3f deflate=%.3f download=%.3f write=%.3f read_phase=%.3f plain_in_bytes=%llu out_bytes=%llu+%llu\n",
                r.times.upload_s, r.times.kernel_s, r.times.deflate_s, r.times.download_s, r.write_s, now_s() - t0, (unsigned long long)r.plain_in,
                (unsigned long long)r.out.bytes[0], (unsigned long long)r.out.bytes[1]);
        if (r.o.inflate == "device")
            fprintf(stderr, "[stats] ingest device: gz_on_device=%d host_sides=%d steps_on_host=%llu collect_wait=%.3f fallback=%s\n", r.gz_on_device, r.host_sides,
                    (unsigned long long)r.steps_on_host, collect_wait, r.feed_fallback.c_str());
    } else if (r.o.stats) {
        fprintf(stderr, "[stats] transform host: steps=%llu pairs_on_device=0 pairs_on_host=%llu fallback=none\n", (unsigned long long)r.steps,
                (unsigned long long)r.st.headers);
        fprintf(stderr, "[stats] seconds: read_phase=%.3f plain_in_bytes=%llu out_bytes=%llu+%llu\n", now_s() - t0, (unsigned long long)r.plain_in,
                (unsigned long long)r.out.bytes[0], (unsigned long long)r.out.bytes[1]);
    }
    return 0;
}
