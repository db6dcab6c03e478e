// unshared_kmers -- MI355X replacement for the compute of the reference's stage 00
// (00.build_unshare_kmers_by_jellyfish/build_unshared_kmers.sh, cited below as s00:N): from the parents' read files to
// paternal.unique.filter.mer / maternal.unique.filter.mer in the working directory.
//
// Same options as the script (s00:6-38,57-118), same argument checks (s00:141-158,166-185), same final products:
// the two .mer files (one upper-case canonical k-mer per line; here in sorted order, the reference's order is the
// third-party counter's hash order) and, with --auto_bounds, {maternal,paternal}.histo and
// {maternal,paternal}.bounds.txt (analysis_kmercount.sh:7-13, find_bounds.awk).  The script's intermediate files
// (*.jf, *.mer.fa, *.mer.filter.fa, *.mer.unique.fa, step_NN_done markers) have no counterpart: one count table in
// HBM holds both parents' counts and the products are read out of it (include/hast.h, hast_kc_*).
//
// Extra options: --device N (repeat it, or --devices a,b,c, to split the key space over several GPUs), --table-gb X (size of the count table per GPU; default: from the input size, at most 85 % of the free HBM), --slices S (process
// the key space in S passes over the input; doubled automatically when the table overflows), --save-table FILE (the
// two sets as a binary stage-01 table for `classify --load-table`), --stats, --ingest host|device (HAST_KC_INGEST; device: the files'
// bytes are inflated and framed on the GPU, see "ingest on the device" below; default host), --device-fasta (HAST_KC_DEVICE_FASTA=1;
// with --ingest device: FASTA parents are framed on the GPU too instead of going back to the host parser; default off).
// Exit status: 0 ok / usage; 1 bad arguments, missing or malformed input (the script: exit 1); 4 GPU trouble.
//
// Layout: main(), at the end, is the list of the run's phases; each phase is a function above it, in that order.  What the command
// line asked for is an Options, what one phase leaves to the next is a Run.  Above the phases: the two ingests (the host parser's and
// the device framer's), which share the job list, the worker threads and the folding of their results, and one sweep over the inputs.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "../../include/hast.h"
#include "cli_common.h"
#include "ingest.h"
#include "raw_blocks.h"
#include "seqstream.h"

namespace {

using hast::now_s;
namespace sw = hast::sw;

void usage(FILE *f) {
    fputs("Usage: unshared_kmers [options]\n"
          "  Parent-specific k-mer sets from paternal and maternal short reads, counted on the GPU.\n"
          "  Writes paternal.unique.filter.mer and maternal.unique.filter.mer into the current directory.\n"
          "    --paternal FILE   paternal reads, FASTA or FASTQ, gzip if the name ends in .gz (repeatable)\n"
          "    --maternal FILE   maternal reads (repeatable); gz and plain files cannot be mixed for one parent\n"
          "    --mer K           k-mer size, 11..32 (default 21)\n"
          "    --thread N        host threads for reading and parsing (default 8)\n"
          "    --memory G        accepted for compatibility (the table size is --table-gb)\n"
          "    --m-lower N / --m-upper N   keep maternal k-mers seen N..N times (default 9 / 33)\n"
          "    --p-lower N / --p-upper N   the same for paternal k-mers (default 9 / 33)\n"
          "    --auto_bounds     derive the four bounds from the count histograms (also writes *.histo, *.bounds.txt)\n"
          "    --device N (repeatable) / --devices a,b,c   GPUs; the k-mer space is split between them\n"
          "    --table-gb X  --slices S  --save-table FILE  --stats\n"
          "    --ingest host|device   device: inflate .gz and frame four-line FASTQ on the GPU (one GPU; anything else\n"
          "                      is read by the host parser after all); default host, or HAST_KC_INGEST\n"
          "    --device-fasta    with --ingest device: frame FASTA on the GPU too (records of any length, a line has to fit\n"
          "                      a block); without it a FASTA parent goes back to the host parser; or HAST_KC_DEVICE_FASTA=1\n",
          f);
}

const char *const kParentName[2] = {"paternal", "maternal"};

bool ends_gz(const std::string &s) { return hast::ends_gz(s, 0); }   // s00:169: the last three bytes alone

struct Options {
    long mer = 21, cpu = 8, memory = 10, lower[2] = {9, 9}, upper[2] = {33, 33};     // s00:44-55; [0] paternal, [1] maternal
    std::vector<std::string> files[2];
    bool auto_bounds = false, stats = false;
    std::vector<int> devices;        // --device N (repeatable) or --devices a,b,c; default: device 0
    double table_gb = 0;
    long slices = 1;
    std::string save_table;
    std::string ingest = "host";     // --ingest host|device
    bool device_fasta = false;       // --device-fasta
};

// ---- ingest: files -> byte stream of bases -> GPU ---------------------------------------------------------------
// One count table per GPU.  With several GPUs the KEY SPACE is split between them (device d of D owns the slices
// d, d+D, ... of the minimizer hash): every GPU sees every chunk of bases and counts only its own k-mers, so there is no
// exchange between the GPUs at all; histograms add up and selections concatenate on the host.
struct Gpu {
    std::vector<hast_kc *> all;
    hast_kc *kc = nullptr;           // all[0]: also sorts and formats the output
    std::vector<std::unique_ptr<std::mutex>> dev_mu;
    std::mutex mu;
    std::string error;               // first failure of a submit
    hast_ctx *gz_ctx = nullptr;      // --ingest device: the context hast_gz_open wants, on the table's device
    bool ok() {
        std::lock_guard<std::mutex> g(mu);
        return error.empty();
    }
    void fail(const char *what) {
        std::lock_guard<std::mutex> g(mu);
        if (error.empty()) error = what;
    }
    void destroy() {
        for (hast_kc *k : all) hast_kc_destroy(k);
        if (gz_ctx) hast_ctx_destroy(gz_ctx);
        gz_ctx = nullptr;
        all.clear();
        kc = nullptr;
    }
};

// collects the parser's output into chunks; a full chunk goes to the GPU and its last K-1 bytes open the next one, so
// that the windows across the cut are counted exactly once
class ChunkSink {
  public:
    ChunkSink(Gpu &gpu, int parent, int k) : gpu_(gpu), parent_(parent), keep_((size_t)k - 1) { buf_.reserve(kChunk + 64); }
    void append(const char *p, size_t n) {
        bases_ += n;
        while (n) {
            const size_t room = kChunk - buf_.size();
            const size_t take = std::min(room, n);
            buf_.insert(buf_.end(), p, p + take);
            p += take;
            n -= take;
            if (buf_.size() >= kChunk) flush(false);
        }
    }
    void separator() {
        buf_.push_back('\n');
        if (buf_.size() >= kChunk) flush(false);
    }
    void flush(bool last) {
        if (buf_.size() > fresh_from_ && gpu_.ok())
            for (size_t d = 0; d < gpu_.all.size(); ++d) {
                std::lock_guard<std::mutex> g(*gpu_.dev_mu[d]);
                if (hast_kc_count(gpu_.all[d], parent_, reinterpret_cast<const uint8_t *>(buf_.data()), buf_.size()) != HAST_OK) {
                    gpu_.fail(hast_last_error());
                    break;
                }
            }
        if (last) {
            buf_.clear();
            fresh_from_ = 0;
            return;
        }
        const size_t keep = std::min(keep_, buf_.size());
        if (keep) memmove(buf_.data(), buf_.data() + buf_.size() - keep, keep);
        buf_.resize(keep);
        fresh_from_ = keep;          // nothing new yet: a chunk that only holds the carried bytes is not sent again
    }
    size_t bases() const { return bases_; }

  private:
    static constexpr size_t kChunk = 32u << 20;
    Gpu &gpu_;
    int parent_;
    size_t keep_, fresh_from_ = 0, bases_ = 0;
    std::vector<char> buf_;
};

struct IngestResult {
    std::string error;
    size_t bases = 0, records = 0, bytes = 0;
    bool clean_end = true;           // the stream ended exactly between two records
    char first = 0;                  // its first byte
};

struct ParentTotals { size_t bases = 0, records = 0, bytes = 0; };

// How a sweep over the inputs, or its ingest, ended.  The three in the middle make count() start over.
enum class Sweep {
    Ok,
    InputError,      // reported on stdout as the script would: exit status 1
    TableFull,       // start over with twice the slices
    GzInOrder,       // a gz file ends inside a record: start over and read each parent's gz files in order, as one stream
    DeviceRefused,   // the device framer does not take the input (DeviceIngest::refused): start over with the host ingest
    GpuError,        // exit status 4
};

// ---- one driver for both ingests -------------------------------------------------------------------------------------------------
// Both parents' files, read by up to --thread workers at once.  Plain files are independent inputs of the counter (s00:190).  The gz
// files of a parent are ONE concatenated stream in the reference (`zcat files | ...`, s00:187-188).  The host ingest still reads them
// in parallel, which gives the same result whenever every file ends exactly between two records and all start with the same byte --
// if not (gz_files_are_one_stream), the caller starts over and reads them in order.  The device ingest reads a parent's files in
// order from the start, plain ones too: one feed per parent.
struct Job {
    int parent;
    std::vector<std::string> paths;  // read one after the other
    bool gz;
    bool one_stream;                 // the files are one input: only the end of the last one is an end of input
    bool check;                      // a gz file read on its own although it is part of a stream: how it starts and ends matters
    IngestResult res;
};

std::vector<Job> build_jobs(const Options &o, bool device, bool gz_in_order) {
    std::vector<Job> jobs;
    for (int p = 1; p >= 0; --p) {                                              // maternal first, as the script does
        std::vector<std::string> order(o.files[p].rbegin(), o.files[p].rend());   // s00:105,109: each new file is put in front
        const bool gz = ends_gz(order[0]);
        if (device || (gz && gz_in_order)) jobs.push_back({p, order, gz, gz, false, {}});
        else
            for (size_t i = 0; i < order.size(); ++i) jobs.push_back({p, {order[i]}, gz, false, gz && order.size() > 1, {}});
    }
    return jobs;
}

template <class Worker>
void run_jobs(std::vector<Job> &jobs, long threads, Worker work) {
    std::atomic<size_t> next{0};
    const int nt = (int)std::max<long>(1, std::min<long>(threads, (long)jobs.size()));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&] {
            for (size_t i; (i = next.fetch_add(1)) < jobs.size();) work(jobs[i]);
        });
    for (auto &t : th) t.join();
}

// the jobs' totals per parent (of this pass over the files alone), and what went wrong: the first input's error before the GPU's
std::string fold_jobs(const std::vector<Job> &jobs, Gpu &gpu, ParentTotals tot[2]) {
    std::string err;
    tot[0] = tot[1] = ParentTotals();
    for (const auto &j : jobs) {
        if (!j.res.error.empty() && err.empty()) err = j.res.error;
        tot[j.parent].bases += j.res.bases;
        tot[j.parent].records += j.res.records;
        tot[j.parent].bytes += j.res.bytes;
    }
    if (err.empty() && !gpu.ok()) err = gpu.error;
    return err;
}

// Every block of a file as BlockSource delivers it (a .gz file inflated), its payload handed to use(bytes, n); use returns false to
// stop early.  What keeps the file from being read to its end is left in err.
template <class Use>
void for_each_block(const std::string &path, size_t block_bytes, std::string &err, Use use) {
    hast::BlockSource src;
    if (!src.open(path, block_bytes)) {
        err = "cannot open " + path;
        return;
    }
    for (;;) {
        std::vector<char> b = src.next();
        if (b.empty()) {
            if (!src.error().empty()) err = path + ": " + src.error();
            return;
        }
        const bool go_on = use(b.data() + hast::BlockSource::kFrontPad, b.size() - hast::BlockSource::kFrontPad);
        src.recycle(std::move(b));
        if (!go_on) return;
    }
}

// ---- the host ingest: files -> SeqParser -> chunks of bases -> GPU ------------------------------------------------------------------
void ingest_stream(Gpu &gpu, int k, Job &job) {
    IngestResult &res = job.res;
    ChunkSink sink(gpu, job.parent, k);
    hast::SeqParser<ChunkSink> parser(sink);
    for (size_t i = 0; i < job.paths.size() && res.error.empty(); ++i) {
        const std::string &path = job.paths[i];
        for_each_block(path, 16u << 20, res.error, [&](const char *p, size_t n) {
            res.bytes += n;
            if (!parser.feed(p, n)) res.error = path + ": " + parser.error();
            return res.error.empty() && gpu.ok();
        });
        if (res.error.empty() && (!job.one_stream || i + 1 == job.paths.size())) {
            res.clean_end = parser.at_record_boundary();
            res.first = parser.first_byte();
            if (!parser.finish()) res.error = path + ": " + parser.error();
        }
    }
    sink.flush(true);
    res.bases = sink.bases();
    res.records = parser.records();
}

// the gz files of a parent, each read on its own: did that give what reading them as one stream gives?
bool gz_files_are_one_stream(const std::vector<Job> &jobs) {
    bool same = true;
    for (size_t i = 0; i < jobs.size(); ++i) {
        const Job &j = jobs[i];
        if (!j.check) continue;
        const bool last = i + 1 == jobs.size() || jobs[i + 1].parent != j.parent;
        const bool first = i == 0 || jobs[i - 1].parent != j.parent;
        if ((!last && !j.res.clean_end) || (!first && j.res.first != jobs[i - 1].res.first && j.res.first && jobs[i - 1].res.first)) same = false;
        if (!j.res.error.empty() && !first) same = false;                       // may parse differently as part of the whole stream
    }
    return same;
}

// ---- ingest on the device (--ingest device, one count table) -------------------------------------------------------------------
// The host only moves raw bytes: a .gz file is inflated on the GPU straight into the framer's input (hast_gz_*), anything else is
// read (or, where hast_gz_open passes, inflated by BlockSource) into pinned memory and uploaded; the framer (hast_sq_*, sq_core.h)
// turns four-line FASTQ into the base stream and hast_kc_count_device counts it.  One feed per parent's input stream, as a thread.
// With --device-fasta the feed takes FASTA as well: an input's first byte decides, as it does for SeqParser, and a FASTA input ends in
// the feed itself (hast_sq_feed_finish) -- there is no tail for the parser, and no record is too long, only a line.
// The gz files of a parent are read IN ORDER as one stream (`zcat a b`): what file a leaves unframed is carried in front of file
// b's bytes.  At the end of an input the bytes behind the last complete record go through SeqParser and the ChunkSink, so the
// unterminated last line and the "ends inside a quality string" error stay the parser's.  Whatever the framer refuses -- a record
// that is not four lines, a full block without a record, an end the parser does not take -- makes the sweep start over with the
// host ingest, which then reports errors in its own words.
struct DeviceIngest {
    bool on = false;
    size_t block = 16u << 20;        // HAST_KC_INGEST_BLOCK
    std::mutex mu;
    std::string refused;             // first refusal of the sweep
    uint64_t blocks_framed = 0, gz_on_device = 0;
    bool fasta = false;              // --device-fasta
    uint64_t fastq_blocks = 0, fasta_blocks = 0;
    std::string fallback = "none";   // why the host ingest ran after all
    void refuse(const std::string &why) {
        std::lock_guard<std::mutex> g(mu);
        if (refused.empty()) refused = why;
    }
    bool is_refused() {
        std::lock_guard<std::mutex> g(mu);
        return !refused.empty();
    }
};

// One job on its way through the framer.  At most one block is ahead of the framer (submit), every block a file has submitted is framed
// before its decoder is closed (file), and the tail goes to the parser only at the end of an input (end_of_input).
// Locks: hast_sq_feed_create, _next, _take_tail and _destroy are called under the table's mutex (dev_mu[0], which hast_kc_count inside
// ChunkSink::flush holds too: "the caller serialises it with the table's other users", include/hast.h); hast_sq_feed_submit,
// _device_block, _host_block and hast_gz_open / _read_device / _close are called without it, so that one parent's thread reads, inflates
// and uploads while the other's block is framed and counted.
struct DeviceStream {
    DeviceStream(Gpu &g, DeviceIngest &d, int k, Job &j, hast_sq_feed *f)
        : gpu(g), di(d), job(j), res(j.res), table_mu(*g.dev_mu[0]), feed(f), sink(g, j.parent, k), tail(d.block) {}
    Gpu &gpu;
    DeviceIngest &di;
    const Job &job;
    IngestResult &res;
    std::mutex &table_mu;
    hast_sq_feed *feed;              // ours: run() destroys it
    ChunkSink sink;
    std::vector<uint8_t> tail;
    int pending = 0;                 // blocks submitted and not framed yet
    uint64_t blocks = 0, gz_dev = 0, fa_blocks = 0;
    size_t bases = 0;

    bool good() { return res.error.empty() && gpu.ok() && !di.is_refused(); }
    bool ck(hast_status st) {        // a call of the library's that failed is the GPU's failure
        if (st != HAST_OK) gpu.fail(hast_last_error());
        return st == HAST_OK;
    }
    bool step() {                    // frame and count the oldest submitted block
        hast_sq_result r;
        bool framed;
        {
            std::lock_guard<std::mutex> g(table_mu);
            framed = ck(hast_sq_feed_next(feed, job.parent, &r));
        }
        --pending;
        if (!framed) return false;
        if (r.flags & HAST_SQ_NOT_FOUR_LINE) {
            di.refuse("not four-line FASTQ (record " + std::to_string(res.records + r.first_bad + 1) + " of a " + kParentName[job.parent] + " input)");
            return false;
        }
        if (r.flags & HAST_SQ_TAIL_TOO_LONG) {
            di.refuse("a full block holds no record");
            return false;
        }
        if (r.records || r.out_bytes) ++blocks;      // (a FASTA view may hold the middle of a record and no header)
        if ((r.records || r.out_bytes) && hast_sq_feed_format(feed) == 2) ++fa_blocks;
        res.records += r.records;
        bases += r.bases;
        return true;
    }
    bool submit(size_t n) {          // ... and keep one block ahead of the framer
        if (!ck(hast_sq_feed_submit(feed, n))) return false;
        res.bytes += n;
        ++pending;
        return pending < 2 || step();
    }
    bool end_of_input(const std::string &path) {
        while (pending)
            if (!step()) return false;
        if (hast_sq_feed_format(feed) == 2) {        // FASTA ends in the feed: the unterminated last line and the closing separator
            hast_sq_result r;
            std::lock_guard<std::mutex> g(table_mu);
            if (!ck(hast_sq_feed_finish(feed, job.parent, &r))) return false;
            res.records += r.records;
            bases += r.bases;
            return true;
        }
        size_t n = 0;
        {
            std::lock_guard<std::mutex> g(table_mu);
            if (!ck(hast_sq_feed_take_tail(feed, tail.data(), &n))) return false;
        }
        hast::SeqParser<ChunkSink> parser(sink);
        if (!parser.feed(reinterpret_cast<const char *>(tail.data()), n) || !parser.finish()) {
            di.refuse("the end of " + path + " is the host parser's (" + parser.error() + ")");
            return false;
        }
        res.records += parser.records();
        sink.flush(true);
        return true;
    }
    // one file's bytes (raw_blocks.h) into the feed's blocks; the block asked for last stays unsubmitted
    void file(const std::string &path) {
        hast::RawBlocks raw;
        std::string err;
        if (!raw.open(path, job.gz, gpu.gz_ctx, di.block, &res.error)) return;
        const bool dev = raw.kind() == hast::RawBlocks::gz_on_device;
        gz_dev += dev;
        for (bool first = raw.kind() == hast::RawBlocks::plain; good(); first = false) {
            uint8_t *b = nullptr;
            size_t n = 0;
            if (!ck(dev ? hast_sq_feed_device_block(feed, &b) : hast_sq_feed_host_block(feed, &b))) break;
            if (!(dev ? raw.read_device(b, hast_kc_stream(gpu.kc), &n) : raw.read_host(b, &n, &err))) {
                if (dev) di.refuse("hast_gz: " + std::string(hast_last_error()));
                else if (raw.kind() == hast::RawBlocks::gz_on_host) res.error = path + ": " + err;
                break;                               // (a plain file that cannot be read on ends there)
            }
            if (n == 0) break;                       // (only a read that returns nothing ends the stream, include/hast.h)
            if (first && b[0] != '@' && !(di.fasta && b[0] == '>')) {
                di.refuse(b[0] == '>' ? path + " is FASTA" : path + " does not start with '@'");
                break;
            }
            if (!submit(n)) break;
        }
        while (dev && pending && good())             // before the decoder goes: its kernels wrote the blocks still waiting
            if (!step()) break;
    }

    void run() {
        for (size_t i = 0; i < job.paths.size() && good(); ++i) {
            file(job.paths[i]);
            if (good() && (!job.one_stream || i + 1 == job.paths.size())) end_of_input(job.paths[i]);
        }
        {
            std::lock_guard<std::mutex> g(table_mu);
            hast_sq_feed_destroy(feed);          // (waits for what this feed has put on the table's stream)
        }
        res.bases = bases + sink.bases();
        std::lock_guard<std::mutex> g(di.mu);
        di.blocks_framed += blocks;
        di.gz_on_device += gz_dev;
        di.fasta_blocks += fa_blocks;
        di.fastq_blocks += blocks - fa_blocks;
    }
};

// the feed first: without one there is no stream, and nothing else is allocated for it
void ingest_device_stream(Gpu &gpu, DeviceIngest &di, int k, Job &job) {
    hast_sq_feed *feed = nullptr;
    {
        std::lock_guard<std::mutex> g(*gpu.dev_mu[0]);
        if (hast_sq_feed_create(gpu.kc, di.block, &feed) != HAST_OK) {
            gpu.fail(hast_last_error());
            return;
        }
        if (di.fasta && hast_sq_feed_set_formats(feed, HAST_SQ_TAKE_FASTQ | HAST_SQ_TAKE_FASTA) != HAST_OK) {
            gpu.fail(hast_last_error());
            hast_sq_feed_destroy(feed);
            return;
        }
    }
    DeviceStream(gpu, di, k, job, feed).run();
}

bool write_histo(const char *path, const std::vector<uint64_t> &h) {
    FILE *f = fopen(path, "w");
    if (!f) return false;
    for (unsigned c = 1; c <= HAST_KC_HISTO_HIGH + 1; ++c)
        if (h[c]) fprintf(f, "%u %llu\n", c, (unsigned long long)h[c]);       // `jellyfish histo` rows
    return fclose(f) == 0;
}

// ---- the run ---------------------------------------------------------------------------------------------------------------------
// What a run holds from one phase of main() to the next.
struct Run {
    Options o;
    Gpu gpu;
    DeviceIngest di;
    double windows = 0;              // an upper bound on the input's k-mer windows
    size_t table_bytes = 0;
    long slices = 1;                 // of the key space: --slices, doubled whenever a table overflows
    bool gz_in_order = false;        // the host ingest reads each parent's gz files in order, as one stream
    std::vector<uint64_t> histo[2];
    ParentTotals tot[2];             // of the last slice read
    uint64_t stats_sum[6] = {0, 0, 0, 0, 0, 0};
    size_t n_sel[2] = {0, 0};
    double t_start = 0, t_table = 0, t_ingest = 0, t_count = 0, t_end = 0;
};

// the only way out once a Run exists
int leave(Run &r, int status) {
    r.gpu.destroy();
    return status;
}

// the exit status of GPU trouble, said on stderr
int gpu_trouble(const char *what) {
    fprintf(stderr, "unshared_kmers: %s: %s\n", what, hast_last_error());
    return 4;
}

// false: leave with `status`
bool parse_command_line(int argc, char **argv, Options &o, int &status) {
    status = 0;
    if (argc == 1) {                                                            // s00:57-60
        usage(stdout);
        return false;
    }
    printf("CMD :");
    for (int i = 0; i < argc; ++i) printf(" %s", argv[i]);
    printf("\n");
    bool ingest_given = false, device_fasta_given = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "-h" || a == "--help") { usage(stdout); return false; }
        else if (a == "--memory") o.memory = atol(val());
        else if (a == "--thread") o.cpu = atol(val());
        else if (a == "--m-lower") o.lower[1] = atol(val());
        else if (a == "--m-upper") o.upper[1] = atol(val());
        else if (a == "--p-lower") o.lower[0] = atol(val());
        else if (a == "--p-upper") o.upper[0] = atol(val());
        else if (a == "--mer") o.mer = atol(val());
        else if (a == "--auto_bounds") o.auto_bounds = true;
        else if (a == "--paternal") o.files[0].push_back(val());
        else if (a == "--maternal") o.files[1].push_back(val());
        else if (a == "--device") o.devices.push_back(atoi(val()));
        else if (a == "--devices") {
            for (const char *q = val(); *q;) {
                o.devices.push_back(atoi(q));
                while (*q && *q != ',') ++q;
                if (*q == ',') ++q;
            }
        }
        else if (a == "--table-gb") o.table_gb = atof(val());
        else if (a == "--slices") o.slices = atol(val());
        else if (a == "--save-table") o.save_table = val();
        else if (a == "--stats") o.stats = true;
        else if (a == "--ingest") { o.ingest = val(); ingest_given = true; }
        else if (a == "--device-fasta") o.device_fasta = device_fasta_given = true;
        else {                                                                  // s00:113-116: message, then a bare `exit`
            printf("unknown option \"%s\"\n", a.c_str());
            return false;
        }
    }
    if (!ingest_given && sw::word_is(sw::HAST_KC_INGEST, "device")) o.ingest = "device";
    if (!device_fasta_given) o.device_fasta = sw::flag(sw::HAST_KC_DEVICE_FASTA);
    if (o.ingest != "host" && o.ingest != "device") {
        printf("ERROR: --ingest %s: host or device\n", o.ingest.c_str());
        status = 1;
        return false;
    }
    return true;
}

// false: said why on stdout, the exit status is 1
bool check_arguments(const Options &o) {
    if (o.memory < 1 || o.cpu < 1 || o.files[0].empty() || o.files[1].empty() || o.mer < 11 || o.lower[1] < 1 ||
        o.upper[1] > 100000000 || o.lower[0] < 1 || o.upper[0] > 100000000 || o.slices < 1 || o.slices > 4096) {   // s00:141-152
        printf("ERROR: invalid arguments\n");
        return false;
    }
    if (o.mer > 32) {
        printf("ERROR: --mer %ld: this build handles k-mers up to 32 bases\n", o.mer);
        return false;
    }
    for (int p = 1; p >= 0; --p)                                                // s00:153-158
        for (const auto &f : o.files[p])
            if (access(f.c_str(), F_OK) != 0) {
                printf("ERROR: input file \"%s\" does not exist\n", f.c_str());
                return false;
            }
    for (int p = 1; p >= 0; --p)                                                // s00:166-185, 197-216
        for (const auto &f : o.files[p])
            if (ends_gz(f) != ends_gz(o.files[p][0])) {
                printf("ERROR: gz and plain inputs mixed for one parent\n");
                return false;
            }
    return true;
}

// Table size when not given: from the input -- an upper bound on its windows from the file sizes (about half the bytes of a
// FASTQ are bases, a gz file holds at most ~3 bases per byte) and a slot (16 B) per window: every window a different k-mer would
// fill the table to the brim, sequencing data (30 x coverage, 15 % error k-mers) fills a quarter to a third of it.  Round 4 took
// twice that, and the record buffers "what is left of the device": 100 GB for a 20-Mbp job, which a box that had just freed
// them took 6 s to hand out (profiles/round4_measure.txt).  Too small a guess only costs a restart with more slices; capped by
// the library at 85 % of the free HBM.
void estimate_windows_and_size_table(Run &r) {
    const Options &o = r.o;
    r.table_bytes = (size_t)(o.table_gb * (double)(1ull << 30));
    for (int p = 0; p < 2; ++p)
        for (const auto &f : o.files[p]) {
            struct stat sb;
            if (stat(f.c_str(), &sb) != 0) continue;
            bool fasta = false;
            if (!ends_gz(f)) {
                if (FILE *fp = fopen(f.c_str(), "rb")) {
                    fasta = fgetc(fp) == '>';
                    fclose(fp);
                }
            }
            r.windows += ends_gz(f) ? 3.0 * (double)sb.st_size : fasta ? (double)sb.st_size : 0.55 * (double)sb.st_size;
        }
    if (r.table_bytes == 0) r.table_bytes = (size_t)std::max(256.0 * (1 << 20), r.windows * 16.0);
}

// one count table per --device; 0, or the exit status
int create_tables(Run &r) {
    Options &o = r.o;
    if (o.devices.empty()) o.devices.push_back(0);
    const size_t n_dev = o.devices.size();
    for (int dev : o.devices) {
        hast_kc *k = nullptr;
        // --table-gb is per GPU; the automatic size is for the whole key space, i.e. divided between the GPUs
        const size_t per_dev = o.table_gb > 0 ? r.table_bytes : r.table_bytes / n_dev + 1;
        if (hast_kc_create_ex(dev, (int)o.mer, per_dev, (uint64_t)(r.windows / (double)n_dev * 1.1) + 1, &k) != HAST_OK)
            return gpu_trouble(("device " + std::to_string(dev)).c_str());
        r.gpu.all.push_back(k);
        r.gpu.dev_mu.emplace_back(new std::mutex());
    }
    r.gpu.kc = r.gpu.all[0];
    return 0;
}

void set_up_device_ingest(Run &r) {
    const Options &o = r.o;
    if (o.ingest != "device") return;
    if (r.gpu.all.size() > 1) {
        fprintf(stderr, "--ingest device works with one count table, there are %zu: using the host ingest\n", r.gpu.all.size());
        r.di.fallback = "several tables";
        return;
    }
    r.di.on = true;
    r.di.fasta = o.device_fasta;
    sw::size(sw::HAST_KC_INGEST_BLOCK, &r.di.block);
    bool any_gz = false;
    for (int p = 0; p < 2; ++p) any_gz = any_gz || ends_gz(o.files[p][0]);
    // (without a context the .gz files are inflated on the host and uploaded)
    if (any_gz && hast_ctx_create(o.devices[0], (int)o.mer, &r.gpu.gz_ctx) != HAST_OK) r.gpu.gz_ctx = nullptr;
}

// ---- counting --------------------------------------------------------------------------------------------------------------------
// the sets of the tables as they stand, appended to the first GPU's selection
bool select_all(Run &r) {
    const Options &o = r.o;
    for (hast_kc *k : r.gpu.all) {
        for (int p = 0; p < 2; ++p) {
            // a bound pair that selects nothing (upper < lower, e.g. from an empty histogram) is an empty set
            if (o.upper[p] < o.lower[p] || o.upper[p] < 1) continue;
            if (hast_kc_select(k, p, (uint32_t)o.lower[p], (uint32_t)std::min<long>(o.upper[p], 0xFFFFFFFFl), nullptr) != HAST_OK) return false;
        }
        if (k != r.gpu.kc && hast_kc_selection_adopt(r.gpu.kc, k) != HAST_OK) return false;
    }
    return true;
}

hast_status sync_all(Gpu &gpu) {                                                // table-full on any device wins
    hast_status worst = HAST_OK;
    for (hast_kc *k : gpu.all) {
        const hast_status st = hast_kc_sync(k);
        if (st == HAST_ERR_TABLE_FULL || (st != HAST_OK && worst == HAST_OK)) worst = st;
    }
    return worst;
}

// Both parents' files into the tables' current slice, by the device framer or the host parser.  Ok (r.tot: this slice's totals),
// GzInOrder, DeviceRefused, or InputError for any failure: err says what, whose it is the caller finds out.
Sweep ingest(Run &r, std::string &err) {
    std::vector<Job> jobs = build_jobs(r.o, r.di.on, r.gz_in_order);
    const int k = (int)r.o.mer;
    if (r.di.on) {
        r.di.refused.clear();
        run_jobs(jobs, r.o.cpu, [&](Job &j) { ingest_device_stream(r.gpu, r.di, k, j); });
        if (!r.di.refused.empty()) return Sweep::DeviceRefused;
    } else {
        run_jobs(jobs, r.o.cpu, [&](Job &j) { ingest_stream(r.gpu, k, j); });
        if (!r.gz_in_order && !gz_files_are_one_stream(jobs)) return Sweep::GzInOrder;
    }
    err = fold_jobs(jobs, r.gpu, r.tot);
    return err.empty() ? Sweep::Ok : Sweep::InputError;
}

// the tables' statistics summed (table_slots: of this slice), their histograms added up
bool collect_slice(Run &r, bool take_histo) {
    r.stats_sum[3] = 0;
    for (hast_kc *k : r.gpu.all) {
        uint64_t stt[6];
        if (hast_kc_stats(k, stt) != HAST_OK) return false;
        for (int i = 0; i < 6; ++i) r.stats_sum[i] += stt[i];
        if (take_histo)
            for (int p = 0; p < 2; ++p)
                if (hast_kc_histo(k, p, r.histo[p].data()) != HAST_OK) return false;
    }
    return true;
}

// One sweep = every slice of the key space: count both parents, then take what this sweep is for.
Sweep sweep(Run &r, bool take_histo, bool take_sets) {
    Gpu &gpu = r.gpu;
    const long n_dev = (long)gpu.all.size();
    for (int p = 0; p < 2 && take_histo; ++p) r.histo[p].assign(HAST_KC_HISTO_HIGH + 2, 0);
    for (auto &x : r.stats_sum) x = 0;
    r.di.blocks_framed = r.di.gz_on_device = r.di.fastq_blocks = r.di.fasta_blocks = 0;
    if (take_sets)                                                              // a sweep that starts over starts from nothing
        for (hast_kc *k : gpu.all)
            if (hast_kc_selection_clear(k) != HAST_OK) return Sweep::GpuError;
    for (long s = 0; s < r.slices; ++s) {
        for (long d = 0; d < n_dev; ++d)
            if (hast_kc_set_slice(gpu.all[d], (uint32_t)(s * n_dev + d), (uint32_t)(r.slices * n_dev)) != HAST_OK) return Sweep::GpuError;
        std::string err;
        const double t_in = now_s();
        const Sweep in = ingest(r, err);
        r.t_ingest += now_s() - t_in;
        if (in == Sweep::InputError) {
            // A count the table refused leaves gpu.error, and then the tables decide: one of them full is a reason to start over,
            // whatever an input said meanwhile; anything else of the GPU's goes to stderr, an input's error to stdout.
            const bool gpu_side = !gpu.error.empty();
            if (gpu_side && sync_all(gpu) == HAST_ERR_TABLE_FULL) return Sweep::TableFull;
            fprintf(gpu_side ? stderr : stdout, "ERROR: %s\n", err.c_str());
            return gpu_side ? Sweep::GpuError : Sweep::InputError;
        }
        if (in != Sweep::Ok) return in;
        const hast_status st = sync_all(gpu);
        if (st == HAST_ERR_TABLE_FULL) return Sweep::TableFull;
        if (st != HAST_OK || !collect_slice(r, take_histo)) return Sweep::GpuError;
        if (take_sets && !select_all(r)) return Sweep::GpuError;
    }
    return Sweep::Ok;
}

// A sweep, started over for as long as it asks to be.  Ok, InputError or GpuError.
Sweep count(Run &r, bool take_histo, bool take_sets) {
    for (;;) {
        r.gpu.error.clear();
        const Sweep s = sweep(r, take_histo, take_sets);
        if (s == Sweep::GzInOrder) {
            fprintf(stderr, "a gz input ends inside a record: reading each parent's gz files in order, as one stream\n");
            r.gz_in_order = true;
            for (hast_kc *k : r.gpu.all) hast_kc_sync(k);
        } else if (s == Sweep::DeviceRefused) {
            fprintf(stderr, "--ingest device: %s: starting over with the host ingest\n", r.di.refused.c_str());
            r.di.on = false;
            r.di.fallback = r.di.refused;
            for (hast_kc *k : r.gpu.all) hast_kc_sync(k);
        } else if (s == Sweep::TableFull) {
            if (r.slices >= 4096) {
                fprintf(stderr, "unshared_kmers: the count table is too small even with %ld slices\n", r.slices);
                return Sweep::GpuError;
            }
            r.slices *= 2;
            fprintf(stderr, "count table full: starting over with %ld slices of the key space\n", r.slices);
        } else return s;
    }
}

// the process's exit status after count(), the one place that turns a Sweep into one; what is the GPU's is said here ("counting")
int exit_status(Sweep s) { return s == Sweep::Ok ? 0 : s == Sweep::InputError ? 1 : gpu_trouble("counting"); }

// --auto_bounds: the four bounds out of the histograms, which go to *.histo and *.bounds.txt (analysis_kmercount.sh:7-13); 0, or the exit status
int write_histograms_and_bounds(Run &r) {
    for (int p = 1; p >= 0; --p) {
        long b[4];
        hast_kc_find_bounds(r.histo[p].data(), b);
        r.o.lower[p] = b[2];
        r.o.upper[p] = b[3];
        const std::string hp = std::string(kParentName[p]) + ".histo", bp = std::string(kParentName[p]) + ".bounds.txt";
        FILE *f = write_histo(hp.c_str(), r.histo[p]) ? fopen(bp.c_str(), "w") : nullptr;
        if (!f) {
            printf("ERROR: cannot write %s / %s\n", hp.c_str(), bp.c_str());
            return 1;
        }
        fprintf(f, "MIN_INDEX=%ld\nMAX_INDEX=%ld\nLOWER_INDEX=%ld\nUPPER_INDEX=%ld\n", b[0], b[1], b[2], b[3]);   // find_bounds.awk:31
        fclose(f);
    }
    return 0;
}

// Everything in one sweep when the bounds are known up front or the table holds the whole key space (1 slice:
// histogram, bounds and sets all come out of the resident table); otherwise histograms first, sets in a second sweep.
// 0, or the exit status
int count_and_select(Run &r) {
    if (!r.o.auto_bounds) return exit_status(count(r, false, true));
    if (int st = exit_status(count(r, true, false))) return st;
    if (int st = write_histograms_and_bounds(r)) return st;
    if (r.slices == 1) return select_all(r) ? 0 : gpu_trouble("counting");      // the tables still hold everything
    return exit_status(count(r, false, true));
}

// ---- the products ----------------------------------------------------------------------------------------------------------------
// a parent's sorted selection as text, one k-mer per line; 0, or the exit status
int write_mer_file(Run &r, int p) {
    hast_kc *kc = r.gpu.kc;
    if (hast_kc_selection_sort(kc, p, &r.n_sel[p]) != HAST_OK) return gpu_trouble("sorting the selection");
    const std::string path = std::string(kParentName[p]) + ".unique.filter.mer";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) {
        printf("ERROR: cannot write %s\n", path.c_str());
        return 1;
    }
    const size_t rows = 4u << 20, width = (size_t)r.o.mer + 1, n_sel = r.n_sel[p];
    std::vector<char> text(std::min(rows, std::max<size_t>(n_sel, 1)) * width);
    for (size_t at = 0; at < n_sel; at += rows) {
        const size_t n = std::min(rows, n_sel - at);
        if (hast_kc_selection_text(kc, p, at, n, text.data()) != HAST_OK) {
            fclose(f);
            return gpu_trouble("formatting the selection");
        }
        if (fwrite(text.data(), 1, n * width, f) != n * width) {
            printf("ERROR: short write to %s\n", path.c_str());
            fclose(f);
            return 1;
        }
    }
    if (fclose(f) != 0) {
        printf("ERROR: cannot write %s\n", path.c_str());
        return 1;
    }
    return 0;
}

int sort_and_write_mer_files(Run &r) {
    for (hast_kc *k : r.gpu.all)
        if (hast_kc_release_table(k) != HAST_OK) return gpu_trouble("releasing the table");
    for (int p = 0; p < 2; ++p)
        if (int st = write_mer_file(r, p)) return st;
    return 0;
}

// --save-table: the two sets as a stage-01 table; hap 0 = paternal, hap 1 = maternal (classify -p / -m).  0, or the exit status
int save_table(Run &r) {
    const Options &o = r.o;
    if (o.save_table.empty()) return 0;
    hast_ctx *ctx = nullptr;
    if (hast_ctx_create(o.devices[0], (int)o.mer, &ctx) != HAST_OK) return gpu_trouble("--save-table");
    bool ok = hast_table_reserve(ctx, r.n_sel[0] + r.n_sel[1] + 64, 0.0) == HAST_OK;
    std::vector<uint64_t> keys;
    for (int p = 0; p < 2 && ok; ++p)
        for (size_t at = 0; at < r.n_sel[p] && ok; at += 8u << 20) {
            const size_t n = std::min<size_t>(8u << 20, r.n_sel[p] - at);
            keys.resize(n);
            ok = hast_kc_selection_keys(r.gpu.kc, p, at, n, keys.data()) == HAST_OK && hast_table_insert_keys(ctx, p, keys.data(), n) == HAST_OK;
        }
    ok = ok && hast_table_save(ctx, o.save_table.c_str()) == HAST_OK;
    const int status = ok ? 0 : gpu_trouble("--save-table");
    hast_ctx_destroy(ctx);
    return status;
}

void print_stats(const Run &r) {
    const Options &o = r.o;
    const long n_dev = (long)o.devices.size();
    fprintf(stderr, "[stats] K=%ld gpus=%ld slices=%ld table_slots=%llu keys_in_table=%llu\n", o.mer, n_dev, r.slices * n_dev,
            (unsigned long long)r.stats_sum[3], (unsigned long long)r.stats_sum[2]);
    for (int p = 0; p < 2; ++p)
        fprintf(stderr, "[stats] %s: %zu input bytes, %zu records, %zu bases, %llu k-mers counted, %llu distinct, %zu selected\n", kParentName[p],
                r.tot[p].bytes, r.tot[p].records, r.tot[p].bases, (unsigned long long)r.stats_sum[4 + p], (unsigned long long)r.stats_sum[p], r.n_sel[p]);
    if (o.ingest == "device")
        fprintf(stderr, "[stats] ingest device: blocks_framed=%llu gz_on_device=%llu fallback=%s\n", (unsigned long long)r.di.blocks_framed,
                (unsigned long long)r.di.gz_on_device, r.di.fallback.c_str());
    if (o.ingest == "device" && o.device_fasta)
        fprintf(stderr, "[stats] ingest device formats: fastq_blocks=%llu fasta_blocks=%llu\n", (unsigned long long)r.di.fastq_blocks,
                (unsigned long long)r.di.fasta_blocks);
    fprintf(stderr, "[stats] table %.3f s, read+parse+count %.3f s, table passes %.3f s, output %.3f s, total %.3f s\n", r.t_table - r.t_start, r.t_ingest,
            r.t_count - r.t_table - r.t_ingest, r.t_end - r.t_count, r.t_end - r.t_start);
}

}  // namespace

int main(int argc, char **argv) {
    Run r;
    int status = 0;
    if (!parse_command_line(argc, argv, r.o, status)) return leave(r, status);
    if (!check_arguments(r.o)) return leave(r, 1);
    r.slices = r.o.slices;
    r.t_start = now_s();
    estimate_windows_and_size_table(r);
    if ((status = create_tables(r))) return leave(r, status);
    set_up_device_ingest(r);
    r.t_table = now_s();
    if ((status = count_and_select(r))) return leave(r, status);
    r.t_count = now_s();
    printf("bounds used for maternal: [%ld, %ld]\n", r.o.lower[1], r.o.upper[1]);   // s00:254-255
    printf("bounds used for paternal: [%ld, %ld]\n", r.o.lower[0], r.o.upper[0]);
    if ((status = sort_and_write_mer_files(r))) return leave(r, status);
    if ((status = save_table(r))) return leave(r, status);
    printf("paternal-unique k-mers kept: %zu (paternal.unique.filter.mer)\n", r.n_sel[0]);      // s00:300-303 (wc -l of the products)
    printf("maternal-unique k-mers kept: %zu (maternal.unique.filter.mer)\n", r.n_sel[1]);
    r.t_end = now_s();
    if (r.o.stats) print_stats(r);
    return leave(r, 0);
}
