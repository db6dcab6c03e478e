// classify_read_main.cpp -- drop-in for the per-read classifier of HAST stage 03 on MI355X
// (reference: /root/reference/03.mkoutput_by_fabulous2.0/src_main/classify.cpp, cited s03:N; usage name
// "classify_read", s03:305).  Same flags (--hap F --hap F --read F [--read F] [--thread N] [--format fasta|fastq],
// s03:316-358) and the same stdout rows "name \t haplotypeN|ambiguous \t density" in read order (s03:104-135).
// K-mer lookups run on the GPU through include/hast.h (hast_classify_perread); this file does what the
// reference does on the host around them: flag parsing, FASTA/FASTQ framing (s03:248-302), the density and
// the call (s03:110-133, 215-216).
//
// Additive flags: --device N, --devices A,B,... (several GPUs of this node: the table is built on the first one and copied to
// the others over xGMI; every batch of reads is cut into one contiguous share per GPU, balanced by bases, classified at the same
// time and printed in read order -- per-read rows need no reduction, BASELINE config 5's "barcode-free per-read assignment").
//
// --ingest device (opt-in; the default, host, is everything described above): the host moves raw file bytes and formats rows, it never
// looks at a base.  A .gz input is inflated on the GPU (hast_gz_*) straight into the read-stream feed (hast_rs_*, rules: rs_core.h),
// anything else is read into the feed's pinned block; the feed frames FASTA / FASTQ on the GPU, classifies the reads where they lie
// and hands back names and votes.  --block-mb N: the feed's block (default 64; HAST_RS_BLOCK=<bytes> for tests).  What the device
// route does not take runs through the host route with one WARN line and the same stdout: several --devices (the whole run), an
// input that is not a regular file, a record that does not fit two blocks (that file, from its start).  --stats: two lines on stderr.
//
// --bin-reads (additive, off by default): besides the rows, every read is written, as its bytes lie in the input, to one of
// DIR/B.haplotype0.E, B.haplotype1.E, B.ambiguous.E (B: the input's basename minus a trailing .gz, E: fasta | fastq by --format, DIR:
// --bin-dir, default "."; --gz-out: gzip members, ".gz" appended).  The rule is rb_core.h's, the class the row's.  With --ingest device
// the runs are partitioned (and deflated) on the GPU and come from hast_rs_next_binned; the host route, every fallback and the FASTQ
// tail write through the model of rb_host.h (zlib members with --gz-out).  A class without reads gets no file; an input that ends in
// the format error leaves none of its files; a failed write is exit 3.
//
// --rows device (additive, with --ingest device; the default is host): the rows are made on the GPU too (hast_rs_next_rows; the rule,
// integer code that prints the density as "%0.6f" does: rr_core.h), so that names and votes stay in HBM and only text comes back.
// format_rows (rr_host.h) stays the route of --rows host, of every fallback above, of the FASTQ tail, of a view whose rows outgrow the
// feed's buffer, and of a run with an empty k-mer set (its rows print inf / nan; one WARN line, fallback=empty_set).
//
// Requirement (deviation): k-mer lines must be upper-case A/C/G/T of one length K <= 32 -- what jellyfish/meryl
// dumps are.  The reference would also store other bytes literally (s03:59-65); we stop with exit 3 instead.
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hast.h"
#include <zlib.h>

#include "cli_common.h"
#include "ingest.h"
#include "raw_blocks.h"
#include "rb_host.h"
#include "rr_host.h"
#include "rs_host.h"

namespace {

using hast::format_rows;
using hast::now_s;
namespace sw = hast::sw;

[[noreturn]] void die(int code, const std::string &what) {
    fprintf(stderr, "classify_read: ERROR: %s", what.c_str());
    const char *e = hast_last_error();
    if (e && *e) fprintf(stderr, " (%s)", e);
    fputc('\n', stderr);
    // (no destructors: a batch may be on the GPU in the background thread, and exit() would take the HIP runtime down under it)
    fflush(stdout);
    fflush(stderr);
    _exit(code);
}

void print_usage() {   // same flags as the reference (s03:316-324); stderr is free-form
    fputs("classify_read (MI355X) -- per-read haplotype assignment\n"
          "  classify_read --hap HAP0.mer --hap HAP1.mer --read READS [--read ...] [--format fasta|fastq] [--thread N]\n"
          "  reads may be gzip files when the name ends in .gz; --format defaults to fasta\n"
          "  --device N / --devices A,B,..   GPU(s); with several, every batch of reads is shared out between them\n"
          "  --ingest host|device            device: reads are inflated and framed on the GPU (one GPU; default host)\n"
          "  --block-mb N                    block of the device ingest (default 64)\n"
          "  --rows host|device              device (with --ingest device): the rows are formatted on the GPU too (default host)\n"
          "  --stats                         counts and seconds of the read phase on stderr\n"
          "  --bin-reads                     also write every input's reads to B.haplotype0|haplotype1|ambiguous.fasta|fastq\n"
          "  --gz-out                        (with --bin-reads) gzip those files, names end in .gz\n"
          "  --bin-dir DIR                   (with --bin-reads) where they go (default: the working directory)\n",
          stderr);
}

// What a FASTQ file's end leaves behind its last complete record (fewer than four newlines) as a batch of one read: the header needs
// its newline, the bases are the next piece, terminated or not (s03:255-260; hast::rs::fq_tail).  No record: an empty batch.  False:
// the header starts with '>', the format error.  Both ingest routes end a file through this.
bool tail_batch(const char *tail, size_t n, std::vector<std::string> &names, std::vector<uint8_t> &bases, std::vector<uint64_t> &offsets) {
    hast::rs::Tail t;
    if (!hast::rs::fq_tail(reinterpret_cast<const uint8_t *>(tail), n, &t)) return false;
    names.clear();
    if (!t.record) return true;
    names.push_back(t.name);
    bases.assign(t.seq.begin(), t.seq.end());
    bases.resize(bases.size() + 16);
    offsets.assign({0, (uint64_t)t.seq.size()});
    return true;
}

// The three files of one input under --bin-reads.  A file is created at its first byte (a class without reads gets none); start()
// removes what an earlier input of the same run cannot have written (the names are distinct) but an earlier run may have left.
struct BinFiles {
    std::string path[3];
    FILE *f[3] = {nullptr, nullptr, nullptr};
    bool gz = false;
    void start(const std::string &dir, const std::string &base, const char *ext, bool gz_out) {
        static const char *const cls[3] = {"haplotype0", "haplotype1", "ambiguous"};
        gz = gz_out;
        for (int c = 0; c < 3; ++c) {
            path[c] = dir + "/" + base + "." + cls[c] + "." + ext + (gz ? ".gz" : "");
            ::remove(path[c].c_str());
        }
    }
    // bytes as they are (the device route's runs: plain, or finished gzip members)
    bool write(int c, const void *p, size_t n) {
        if (!n) return true;
        if (!f[c] && !(f[c] = fopen(path[c].c_str(), "wb"))) return false;
        return fwrite(p, 1, n, f[c]) == n;
    }
    // plain bytes from the host model: with --gz-out one zlib member per call
    bool write_plain(int c, const std::string &run) {
        if (run.empty() || !gz) return write(c, run.data(), run.size());
        z_stream z;
        memset(&z, 0, sizeof(z));
        if (deflateInit2(&z, 1, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        std::vector<unsigned char> buf(1u << 20);
        bool ok = true;
        size_t at = 0;
        int rc = Z_OK;
        while (ok && rc != Z_STREAM_END) {                          // (avail_in is 32 bits wide: a run goes in by pieces)
            if (z.avail_in == 0 && at < run.size()) {
                const size_t k = std::min<size_t>(run.size() - at, 1u << 30);
                z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(run.data() + at));
                z.avail_in = (uInt)k;
                at += k;
            }
            z.next_out = buf.data();
            z.avail_out = (uInt)buf.size();
            rc = deflate(&z, at == run.size() ? Z_FINISH : Z_NO_FLUSH);
            if (rc == Z_STREAM_ERROR) ok = false;
            else ok = write(c, buf.data(), buf.size() - z.avail_out);
        }
        deflateEnd(&z);
        return ok;
    }
    bool write_runs(const hast::rb::Runs &r) {
        for (int c = 0; c < 3; ++c)
            if (!write_plain(c, r.run[c])) return false;
        return true;
    }
    bool close_all() {
        bool ok = true;
        for (int c = 0; c < 3; ++c)
            if (f[c]) {
                ok = fclose(f[c]) == 0 && ok;
                f[c] = nullptr;
            }
        return ok;
    }
    void discard() {                                                // the input ended in the format error, or is read again from its start
        (void)close_all();
        for (int c = 0; c < 3; ++c) ::remove(path[c].c_str());
    }
};

// the format error in the reference's words (s03:262,288); false, for the caller to hand on
bool wrong_format(bool fastq) {
    fprintf(stderr, fastq ? "fasta detected . ERROR . please use \"--format fasta\". exit ... \n" : "fasta detected . ERROR . please use \"--format fastq\". exit ... \n");
    return false;
}

struct Options {
    std::vector<std::string> haps, read, bin_base;          // bin_base: with --bin-reads, per input its basename minus a trailing .gz
    std::string format = "fasta", bin_dir = ".";
    std::vector<int> devices;
    bool fastq = false, ingest_device = false, stats = false, bin_reads = false, gz_out = false;
    bool rows_device = false, rows_given = false;          // --rows device; --rows was said at all (--stats then has a line on it)
    long t_num = 8, block_mb = 64;
};

// a parsed batch of reads on its way to the GPU
struct Batch {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets;
    std::vector<std::string> names;
    std::string raw;                                        // --bin-reads: the view the records lie in, and their extents in it
    std::vector<hast::rb::Extent> ext;
};

// What the ONE background thread works on: the host route hands it a batch (HostRoute::classify_batch) so that the upload, the kernel
// and the formatting of block i run while block i + 1 is indexed and copied; one thread, so rows stay in order.  From that hand-over to
// wait() everything here is the thread's alone; the main thread touches it, run_batch and DeviceRoute::step included, only after wait().
struct Shared {
    Batch bt[2];                                            // the batch in flight and the one before it (its buffers are reused)
    int cur = 0;
    std::string out_rows;                                   // the rows of the input at hand
    BinFiles bins;
    hast::rb::Runs bin_runs;
    bool bin_failed = false;
    std::string error;                                      // the thread's failure, said by wait()
    uint64_t st_records = 0;                                // what --stats prints of them
    struct BinStats { uint64_t cls[3] = {0, 0, 0}, dev = 0, host = 0; } st_bin;
    double st_kernels = 0, st_rows = 0;
    std::thread thread;
    ~Shared() { join(); }                                   // every way out of main() waits for the batch in flight
    void join() { if (thread.joinable()) thread.join(); }
    void wait() {
        join();
        if (!error.empty()) die(4, error);
    }
};

// what one phase of main() leaves to the next
struct Run {
    explicit Run(const Options &opt) : o(opt), pool(opt.t_num) {}
    const Options o;
    size_t K = 0, rs_block = 0;                             // rs_block: the device ingest's block
    hast_ctx *ctx = nullptr;                                // ctxs[0]: the table is built there
    std::vector<hast_ctx *> ctxs;
    int total_kmers[2] = {0, 0};                            // s03:50,68 (an `int` in the reference)
    hast::WorkerPool pool;
    hast_rs *feed = nullptr;                                // --ingest device
    uint64_t st_blocks = 0, st_gz = 0;                      // the main thread's part of --stats
    bool rows_on_device = false;                            // --rows device, and the feed makes them
    uint64_t st_row_views[2] = {0, 0}, st_row_bytes = 0;    // views whose rows came as text / were formatted here; bytes of that text
    std::string st_rows_fallback = "none";
    double st_read = 0, st_upload = 0, t_phase = 0;
    std::string st_fallback = "none";
    bool output_failed = false;
    Shared sh;                                              // (last: its thread is joined before anything above goes)
};

// false: the usage text or the reference's word on --format has been printed, the exit status is -1
bool parse_options(int argc, char **argv, Options &o) {
    static struct option long_options[] = {{"hap", required_argument, NULL, 'p'},    {"read", required_argument, NULL, 'r'},
                                           {"format", required_argument, NULL, 'f'}, {"thread", required_argument, NULL, 't'},
                                           {"help", no_argument, NULL, 'h'},         {"device", required_argument, NULL, 1001},
                                           {"devices", required_argument, NULL, 1002}, {"ingest", required_argument, NULL, 1003},
                                           {"block-mb", required_argument, NULL, 1004}, {"stats", no_argument, NULL, 1005},
                                           {"bin-reads", no_argument, NULL, 1006},   {"gz-out", no_argument, NULL, 1007},
                                           {"bin-dir", required_argument, NULL, 1008}, {"rows", required_argument, NULL, 1009},
                                           {0, 0, 0, 0}};
    int device = 0;
    bool ok = true;
    while (ok) {
        int c = getopt_long(argc, argv, "p:r:t:f:h", long_options, NULL);   // s03:324
        if (c < 0) break;
        switch (c) {
        case 'p': o.haps.push_back(optarg); break;
        case 'r': o.read.push_back(optarg); break;
        case 'f': o.format = optarg; break;
        case 't': o.t_num = atoi(optarg); break;
        case 1001: device = atoi(optarg); break;
        case 1002: ok = hast::parse_device_list(optarg, o.devices); break;
        case 1003: o.ingest_device = strcmp(optarg, "device") == 0; ok = o.ingest_device || strcmp(optarg, "host") == 0; break;
        case 1004: o.block_mb = atol(optarg); ok = o.block_mb >= 1 && o.block_mb <= 1024; break;
        case 1005: o.stats = true; break;
        case 1006: o.bin_reads = true; break;
        case 1007: o.gz_out = true; break;
        case 1008: o.bin_dir = optarg; break;
        case 1009: o.rows_given = true; o.rows_device = strcmp(optarg, "device") == 0; ok = o.rows_device || strcmp(optarg, "host") == 0; break;
        case 'h':
        default: ok = false;
        }
    }
    ok = ok && o.haps.size() == 2 && !o.read.empty() && o.t_num >= 1;        // s03:351-354
    ok = ok && !(o.gz_out && !o.bin_reads);
    ok = ok && !(o.rows_device && !o.ingest_device);
    for (size_t i = 0; ok && o.bin_reads && i < o.read.size(); ++i) {
        const std::string &r = o.read[i];
        std::string b = r.substr(r.find_last_of('/') == std::string::npos ? 0 : r.find_last_of('/') + 1);
        if (hast::ends_gz(b)) b.resize(b.size() - 3);
        ok = std::find(o.bin_base.begin(), o.bin_base.end(), b) == o.bin_base.end();   // two inputs would write the same files
        o.bin_base.push_back(b);
    }
    if (!ok) {
        print_usage();
        return false;
    }
    if (o.devices.empty()) o.devices.push_back(device);
    o.fastq = o.format == "fastq";
    if (o.format != "fasta" && !o.fastq) {
        fprintf(stderr, " ERROR : invalid format : [%s] . exit ...\n", o.format.c_str());
        return false;
    }
    return true;
}

// ---- load_kmers (s03:51-70): hast::KmerFiles reads; ours are the library's check, on the device, that every line is K upper-case
// A/C/G/T bytes, the complete lines only of a file read into memory (s03:63), and the words of what goes wrong
void load_kmers(Run &rs) {
    hast::KmerFiles kf;
    std::string msg;
    if (int code = kf.open(rs.o.haps[0], rs.o.haps[1], &msg)) die(code, msg);
    rs.K = kf.K;                                                                // s03:57-58
    if (rs.K < 1 || rs.K > 32) die(3, "K (length of the first k-mer line) must be in [1,32]");
    if (hast_ctx_create(rs.o.devices[0], (int)rs.K, &rs.ctx) != HAST_OK) die(4, "cannot create GPU context");
    if (hast_ctx_set_text_check(rs.ctx, 1) != HAST_OK) die(4, "cannot create GPU context");
    if (hast_table_reserve(rs.ctx, kf.capacity(), 0.0) != HAST_OK) die(4, "allocating the k-mer table");
    for (int h = 0; h < 2; h++) {
        fprintf(stderr, "__load hap%d kmers__\n", h);
        uint64_t lines = 0;
        if (int code = kf.insert(rs.ctx, h, true, true, &lines, &msg))
            die(code, msg.empty() ? std::string(hast_last_error()) + " (k-mer files must hold one K-mer of upper-case A/C/G/T per line)" : msg);
        rs.total_kmers[h] = (int)lines;
        fprintf(stderr, "Recorded %d haplotype %d specific %zu-mers\n", rs.total_kmers[h], h, rs.K);
    }
}

// the other GPUs get a copy of the finished table, peer to peer
void clone_to_other_gpus(Run &rs) {
    rs.ctxs.assign(1, rs.ctx);
    for (size_t i = 1; i < rs.o.devices.size(); i++) {
        hast_ctx *c2 = nullptr;
        if (hast_ctx_create(rs.o.devices[i], (int)rs.K, &c2) != HAST_OK) die(4, "cannot create GPU context");
        rs.ctxs.push_back(c2);
    }
    if (rs.ctxs.size() == 1) return;
    // (all at once: every GPU pulls its copy over its own xGMI link; the source's filter is built first, the clones only read the source)
    if (hast_filter_build(rs.ctx) != HAST_OK) die(4, "building the k-mer filter");
    std::vector<std::thread> cloners;
    std::vector<int> failed(rs.ctxs.size(), 0);
    for (size_t i = 1; i < rs.ctxs.size(); i++)
        cloners.emplace_back([&rs, &failed, i] { failed[i] = hast_table_clone(rs.ctxs[i], rs.ctx) != HAST_OK; });
    for (std::thread &t : cloners) t.join();
    for (int f : failed)
        if (f) die(4, "copying the k-mer table to another GPU");
}

// --ingest device: one feed on the context's GPU (hast_rs_*), unless the run has several
void create_device_feed(Run &rs) {
    const Options &o = rs.o;
    rs.rs_block = (size_t)o.block_mb << 20;
    sw::size(sw::HAST_RS_BLOCK, &rs.rs_block);
    if (!o.ingest_device) return;
    if (rs.ctxs.size() > 1) {
        fprintf(stderr, "classify_read: WARN: --ingest device takes one GPU: host ingest for this run (fallback=several_devices)\n");
        rs.st_fallback = "several_devices";
        if (o.rows_device) rs.st_rows_fallback = "several_devices";
        return;
    }
    if (hast_rs_create(rs.ctx, o.fastq ? HAST_RS_FASTQ : HAST_RS_FASTA, rs.rs_block, &rs.feed) != HAST_OK) die(4, "cannot create the device ingest");
    if (o.bin_reads && hast_rs_set_bins(rs.feed, o.gz_out ? 2 : 1, (uint32_t)rs.total_kmers[0], (uint32_t)rs.total_kmers[1]) != HAST_OK) die(4, "cannot create the device ingest's bins");
    if (!o.rows_device) return;
    if (rs.total_kmers[0] < 1 || rs.total_kmers[1] < 1) {
        fprintf(stderr, "classify_read: WARN: a k-mer set is empty: --rows device: rows are made on the host (fallback=empty_set)\n");
        rs.st_rows_fallback = "empty_set";
        return;
    }
    if (hast_rs_set_rows(rs.feed, 1, (uint32_t)rs.total_kmers[0], (uint32_t)rs.total_kmers[1]) != HAST_OK) die(4, "cannot create the device ingest's rows");
    rs.rows_on_device = true;
}

// the votes of b's reads, one contiguous share of the reads per GPU; what went wrong, or nothing
std::string classify_shares(Run &rs, const Batch &b, std::vector<uint32_t> &v) {
    const size_t n = b.names.size(), G = rs.ctxs.size();
    if (G == 1) return hast_classify_perread(rs.ctx, b.bases.data(), b.offsets.data(), n, v.data()) == HAST_OK ? "" : hast_last_error();
    // cut where the bases divide evenly (reads differ in length by orders of magnitude); the shares run at the same time, every one
    // on a thread of its own (a context is driven by one thread)
    std::vector<size_t> cut(G + 1, n);
    cut[0] = 0;
    const uint64_t total = b.offsets[n] - b.offsets[0];
    for (size_t g = 1; g < G; g++) {
        const uint64_t want = b.offsets[0] + total * g / G;
        cut[g] = (size_t)(std::lower_bound(b.offsets.begin(), b.offsets.begin() + (long)n, want) - b.offsets.begin());
        if (cut[g] < cut[g - 1]) cut[g] = cut[g - 1];
    }
    std::vector<std::string> errs(G);
    std::vector<std::thread> th;
    for (size_t g = 0; g < G; g++)
        th.emplace_back([&rs, &b, &v, &cut, &errs, g] {
            const size_t lo = cut[g], hi = cut[g + 1];
            if (hi > lo && hast_classify_perread(rs.ctxs[g], b.bases.data(), b.offsets.data() + lo, hi - lo, v.data() + 2 * lo) != HAST_OK)
                errs[g] = hast_last_error();
        });
    for (std::thread &t : th) t.join();
    for (const std::string &e : errs)
        if (!e.empty()) return e;
    return "";
}

// Classify the parsed batch and append its rows (and, with --bin-reads, its reads through the host model into the input's files).
// The background thread's work; the device route's FASTQ tail runs it on the main thread.
void run_batch(Run &rs, Batch &b) {
    Shared &sh = rs.sh;
    if (b.names.empty()) return;
    const size_t n = b.names.size();
    const double t0 = now_s();
    std::vector<uint32_t> v(n * 2, 0);
    const std::string trouble = classify_shares(rs, b, v);
    if (!trouble.empty()) return (void)(sh.error = "classifying a batch (" + trouble + ")");
    const double t1 = now_s();
    for (size_t i = 0; i < n; i++) {
        const uint32_t off[2] = {0, (uint32_t)b.names[i].size()};
        format_rows(sh.out_rows, reinterpret_cast<const uint8_t *>(b.names[i].data()), off, v.data() + 2 * i, 1, rs.total_kmers);
    }
    if (rs.o.bin_reads && b.ext.size() == n) {
        hast::rb::append_runs(reinterpret_cast<const uint8_t *>(b.raw.data()), b.ext.data(), v.data(), n, (uint32_t)rs.total_kmers[0], (uint32_t)rs.total_kmers[1], &sh.bin_runs);
        if (!sh.bins.write_runs(sh.bin_runs)) sh.bin_failed = true;
        for (int c = 0; c < 3; ++c) {
            sh.st_bin.cls[c] += sh.bin_runs.count[c];
            sh.st_bin.host += sh.bin_runs.run[c].size();
        }
        sh.bin_runs.clear();
    }
    sh.st_records += n;
    sh.st_kernels += t1 - t0;
    sh.st_rows += now_s() - t1;
}

// the FASTQ tail as a record of the bins: its bytes as they lie, plus a newline if they do not end in one (rb_host.h: append_tail)
void bin_tail(Batch &b, const char *tail, size_t n_tail) {
    b.raw.assign(tail, n_tail);
    if (b.raw.back() != '\n') b.raw += '\n';
    b.ext.assign(1, hast::rb::Extent{0, b.raw.size()});
}

// ---- the host route: block ingest with t_num parser threads (ingest.h), one GPU batch per block ------------------------
// Framing as in the reference: FASTQ = 4 getlines per record, the header must be newline-terminated (s03:255-263);
// FASTA = '>' lines start a record, other non-empty lines are appended, a last line without '\n' is dropped
// (s03:279-296).  Rows of a file are printed when the file is done, like PrintOutput after the loop (s03:269,301).
struct HostRoute {
    explicit HostRoute(Run &run) : rs(run), T(run.pool.size()), part((size_t)T + 1), bad((size_t)T), hl((size_t)T) { sw::size(sw::HAST_READ_BLOCK_BYTES, &block_bytes); }
    Run &rs;
    const int T;
    size_t block_bytes = (size_t)256 << 20;                 // HAST_READ_BLOCK_BYTES
    Batch w;                                                // the batch being parsed: classify_batch hands it to the background thread
    struct RecSpan { uint32_t head, seq_first, seq_end; };  // line indices; sequence lines [seq_first, seq_end)
    std::vector<RecSpan> recs;
    std::vector<uint64_t> part;
    std::vector<int> bad;
    std::vector<std::vector<uint32_t>> hl;
    bool seen_header = false;                               // FASTA: lines before the first '>' belong to no record (s03:286-292)

    static size_t line_start(const hast::BlockWork &a, size_t i) { return i ? (size_t)a.nl[i - 1] + 1 : 0; }
    // recs (over the area's lines) -> names/offsets/bases of w, in parallel
    void build_batch(const hast::BlockWork &a) {
        const size_t n = recs.size();
        const char *data = a.data;
        w.names.assign(n, std::string());
        w.offsets.assign(n + 1, 0);
        if (n == 0) return w.bases.clear();
        rs.pool.run([&](int t) {
            uint64_t sum = 0;
            for (size_t i = n * (size_t)t / T; i < n * (size_t)(t + 1) / T; i++) {
                const RecSpan &r = recs[i];
                if (r.seq_end > r.seq_first) sum += ((uint64_t)a.nl[r.seq_end - 1] - line_start(a, r.seq_first)) - (r.seq_end - r.seq_first - 1);
            }
            part[t + 1] = sum;
        });
        part[0] = 0;
        for (int t = 0; t < T; t++) part[t + 1] += part[t];
        w.bases.resize(part[T] + 16);
        rs.pool.run([&](int t) {
            uint64_t off = part[t];
            for (size_t i = n * (size_t)t / T; i < n * (size_t)(t + 1) / T; i++) {
                const RecSpan &r = recs[i];
                const size_t hs = line_start(a, r.head), he = a.nl[r.head];
                w.names[i].assign(data + hs + (he > hs ? 1 : 0), data + he);             // head.substr(1), s03:207
                w.offsets[i] = off;
                for (uint32_t li = r.seq_first; li < r.seq_end; li++) {
                    const size_t ls = line_start(a, li), le = a.nl[li];
                    memcpy(w.bases.data() + off, data + ls, le - ls);
                    off += le - ls;
                }
            }
        });
        w.offsets[n] = part[T];
        if (!rs.o.bin_reads) return;
        w.ext.resize(n);                                    // the records' extents (rb_core.h) and the bytes they lie in, for the background thread
        uint64_t end = 0;
        for (size_t i = 0; i < n; i++) {
            const RecSpan &r = recs[i];
            w.ext[i].lo = line_start(a, r.head);
            w.ext[i].hi = rs.o.fastq ? (uint64_t)a.nl[r.head + 3] + 1 : line_start(a, r.seq_end);
            end = w.ext[i].hi;
        }
        w.raw.assign(data, end);
    }
    // w to the background thread; the batch before the one in flight becomes the next work area
    void classify_batch() {
        Shared &sh = rs.sh;
        sh.wait();                                          // one batch in flight; its rows are in out_rows now
        if (w.names.empty()) return;
        Batch &b = sh.bt[sh.cur];
        std::swap(b, w);
        sh.thread = std::thread(run_batch, std::ref(rs), std::ref(b));
        sh.cur ^= 1;
        Batch &o = sh.bt[sh.cur];                           // idle since the wait above: its vectors (and their capacity) are the next work area
        w.bases.swap(o.bases);
        w.offsets.swap(o.offsets);
        w.names.swap(o.names);
        w.raw.clear();
        w.ext.clear();
    }
    // One area of a FASTQ file: its complete records as a batch; at the end of the file what is left behind them (header terminated;
    // bases = next piece, terminated or not, s03:260) as a batch of one.  false: the format error
    bool fastq_area(const hast::BlockWork &a, size_t *consumed) {
        const size_t n_lines = a.nl.size(), n_rec = n_lines / 4;
        for (size_t i = 0; i < n_rec; i++) recs.push_back({(uint32_t)(4 * i), (uint32_t)(4 * i + 1), (uint32_t)(4 * i + 2)});
        *consumed = n_rec ? (size_t)a.nl[4 * n_rec - 1] + 1 : 0;
        for (const RecSpan &x : recs)
            if (a.len && a.data[line_start(a, x.head)] == '>') return wrong_format(true);
        build_batch(a);
        classify_batch();
        if (!a.last || n_lines % 4 == 0) return true;
        if (!tail_batch(a.data + *consumed, a.len - *consumed, w.names, w.bases, w.offsets)) return wrong_format(true);
        if (rs.o.bin_reads && !w.names.empty()) bin_tail(w, a.data + *consumed, a.len - *consumed);
        classify_batch();
        return true;
    }
    // One area of a FASTA file: header lines have '>' as their first byte; '@' / '+' at the start of a non-empty line is the
    // reference's format error (false)
    bool fasta_area(const hast::BlockWork &a, size_t *consumed) {
        const size_t n_lines = a.nl.size();                 // complete ('\n'-terminated) lines in the work area
        rs.pool.run([&](int t) {
            bad[t] = 0;
            hl[t].clear();
            for (size_t i = n_lines * (size_t)t / T; i < n_lines * (size_t)(t + 1) / T; i++) {
                const size_t ls = line_start(a, i);
                if (a.nl[i] == ls) continue;                                            // empty line: skipped (s03:280)
                const char c = a.data[ls];
                if (c == '>') hl[t].push_back((uint32_t)i);
                else if (c == '@' || c == '+') bad[t] = 1;
            }
        });
        std::vector<uint32_t> heads;
        for (int t = 0; t < T; t++) {
            if (bad[t]) return wrong_format(false);
            heads.insert(heads.end(), hl[t].begin(), hl[t].end());
        }
        // complete records: header j .. header j+1; at EOF the last header's record ends at the last complete line
        for (size_t j = 0; j + 1 < heads.size(); j++) recs.push_back({heads[j], heads[j] + 1, heads[j + 1]});
        if (a.last && !heads.empty()) recs.push_back({heads.back(), heads.back() + 1, (uint32_t)n_lines});
        if (!heads.empty()) seen_header = true;
        if (a.last) *consumed = a.len;
        else if (!heads.empty()) *consumed = line_start(a, heads.back());     // carry the (possibly incomplete) last record
        else *consumed = seen_header ? 0 : (n_lines ? (size_t)a.nl[n_lines - 1] + 1 : 0);   // no header yet: drop complete lines
        build_batch(a);
        classify_batch();
        return true;
    }
    // one input: its rows into out_rows; 1: the format error (its message is printed)
    int file(const std::string &r) {
        hast::BlockSource src;
        if (!src.open(r, block_bytes)) die(2, "cannot open " + r);
        hast::BlockWork a;
        rs.sh.wait();
        rs.sh.out_rows.clear();
        seen_header = false;
        for (;;) {
            const double t_read = now_s();
            if (!a.next(src)) die(2, r + ": " + src.error());
            rs.st_read += now_s() - t_read;
            if (a.len >= (1ull << 32)) die(3, "a single record spans more than 4 GB");
            a.index(rs.pool);
            recs.clear();
            size_t consumed = 0;
            if (!(rs.o.fastq ? fastq_area(a, &consumed) : fasta_area(a, &consumed))) return 1;
            if (a.last) return 0;
            a.keep(src, consumed);
        }
    }
};

// ---- the device route: an input's raw bytes (raw_blocks.h) through the run's feed, one block ahead of the framer ----
struct DeviceRoute {
    explicit DeviceRoute(Run &run) : rs(run), sh(run.sh), feed(run.feed) {}
    Run &rs;
    Shared &sh;                                             // (no batch is in flight while an input is on this route)
    hast_rs *feed;
    int pending = 0;                                        // blocks submitted and not framed yet
    int verdict = 0;                                        // of the input at hand; 1: the format error, 2: a record too long
    uint64_t framed_records = 0;                            // counted once the file is through: a refused file is read again
    std::vector<uint8_t> tail;

    void step() {                                           // frame and classify the oldest submitted block, format its rows
        hast_rs_block b;
        hast_rs_binned rb;
        hast_rs_rows rw{};
        const double t0 = now_s();
        const hast_status st = rs.rows_on_device ? hast_rs_next_rows(feed, &b, rs.o.bin_reads ? &rb : nullptr, &rw)
                               : rs.o.bin_reads  ? hast_rs_next_binned(feed, &b, &rb)
                                                 : hast_rs_next(feed, &b);
        if (st != HAST_OK) die(4, "framing and classifying a block");
        const double t1 = now_s();
        --pending;
        ++rs.st_blocks;
        sh.st_kernels += t1 - t0;
        if (b.flags & HAST_RS_FORMAT_ERROR) verdict = 1;
        else if (b.flags & HAST_RS_RECORD_TOO_LONG) verdict = 2;
        if (verdict) return;
        if (rs.rows_on_device && !rw.on_host) {              // finished text: nothing is formatted here
            sh.out_rows.append(reinterpret_cast<const char *>(rw.text), (size_t)rw.bytes);
            ++rs.st_row_views[0];
            rs.st_row_bytes += rw.bytes;
        } else {
            format_rows(sh.out_rows, b.names, b.name_off, b.votes, (size_t)b.records, rs.total_kmers);
            ++rs.st_row_views[1];
        }
        framed_records += b.records;
        if (rs.o.bin_reads)
            for (int c = 0; c < 3; ++c) {
                if (!sh.bins.write(c, rb.run[c], (size_t)rb.run_bytes[c])) sh.bin_failed = true;
                sh.st_bin.cls[c] += rb.count[c];
                sh.st_bin.dev += rb.raw_bytes[c];
            }
        sh.st_rows += now_s() - t1;
    }
    void submit(size_t n) {                                 // (empty: the input's last) ... and keep one block ahead of the framer
        const double t0 = now_s();
        if (hast_rs_submit(feed, n, n == 0) != HAST_OK) die(4, "submitting a block");
        rs.st_upload += now_s() - t0;
        if (++pending == 2) step();
    }
    uint8_t *block(bool on_device, hast_stream *fill) {     // the block the next bytes go to: the decoder's, or the pinned one
        uint8_t *b = nullptr;
        const double t0 = now_s();
        if (on_device && hast_rs_device_block(feed, &b, fill) != HAST_OK) die(4, "the device ingest's block");
        if (!on_device && hast_rs_host_block(feed, &b) != HAST_OK) die(4, "the device ingest's staging block");
        if (!on_device) rs.st_upload += now_s() - t0;
        return b;
    }
    // what a FASTQ file leaves behind its last complete record, classified here and now
    void fastq_tail() {
        size_t n_tail = 0;
        tail.resize(rs.rs_block);
        if (hast_rs_take_tail(feed, tail.data(), &n_tail) != HAST_OK) die(4, "the end of the input");
        Batch tb;
        const char *t = reinterpret_cast<const char *>(tail.data());
        if (!tail_batch(t, n_tail, tb.names, tb.bases, tb.offsets)) return (void)(verdict = 1);
        if (rs.o.bin_reads && !tb.names.empty()) bin_tail(tb, t, n_tail);
        run_batch(rs, tb);
        if (!sh.error.empty()) die(4, sh.error);
    }
    // one input: its rows into out_rows; 1: the format error (its message is printed), 2: a record too long
    int file(const std::string &r) {
        hast::RawBlocks raw;
        std::string err;
        if (!raw.open(r, hast::ends_gz(r), rs.ctx, rs.rs_block, &err)) die(2, err);
        const bool on_device = raw.kind() == hast::RawBlocks::gz_on_device;
        if (on_device) ++rs.st_gz;
        sh.out_rows.clear();
        verdict = 0;
        framed_records = 0;
        size_t got = 1;
        while (!verdict && got) {                           // (only a read that returns nothing ends the stream, include/hast.h)
            const double t0 = now_s();
            hast_stream fill = nullptr;
            uint8_t *b = block(on_device, &fill);
            if (!(on_device ? raw.read_device(b, fill, &got) : raw.read_host(b, &got, &err))) die(2, r + ": " + (on_device ? hast_last_error() : err));
            rs.st_read += now_s() - t0;
            submit(got);
        }
        if (got) {                                          // given up: the feed wants the file's last block all the same
            block(on_device, nullptr);
            submit(0);
        }
        while (pending) step();                             // (before the decoder goes: its kernels wrote the blocks still waiting)
        raw.close();
        if (!verdict) sh.st_records += framed_records;
        if (!verdict && rs.o.fastq) fastq_tail();
        if (verdict == 1) wrong_format(rs.o.fastq);
        return verdict;
    }
};

// One input down the ladder: the device route if there is one and it takes the input, else (with one WARN line) the host route; then its
// bins closed and its rows written.  1: the format error -- the input leaves no files, as it leaves no rows, and the run ends.
int process_input(Run &rs, HostRoute &host, DeviceRoute *dev, size_t ri) {
    const Options &o = rs.o;
    Shared &sh = rs.sh;
    const std::string &r = o.read[ri];
    fprintf(stderr, "__process read: %s\n", r.c_str());
    if (o.bin_reads) sh.bins.start(o.bin_dir, o.bin_base[ri], o.fastq ? "fastq" : "fasta", o.gz_out);
    const Shared::BinStats bin_before = sh.st_bin;
    int v = -1;                                             // the device route's word on the input; -1: not asked
    struct stat sb;
    if (dev && (stat(r.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode))) {
        fprintf(stderr, "classify_read: WARN: %s is not a regular file: host ingest for this input (fallback=not_a_regular_file)\n", r.c_str());
        rs.st_fallback = "not_a_regular_file";
        if (rs.rows_on_device) rs.st_rows_fallback = "not_a_regular_file";
    } else if (dev) v = dev->file(r);
    if (v == 2) {
        fprintf(stderr, "classify_read: WARN: a record of %s does not fit two blocks of %zu bytes: host ingest for this input (fallback=record_too_long)\n",
                r.c_str(), rs.rs_block);
        rs.st_fallback = "record_too_long";
        if (rs.rows_on_device) rs.st_rows_fallback = "record_too_long";
        if (o.bin_reads) {                                  // the file is read again from its start: so are its bins
            sh.bins.discard();
            sh.bins.start(o.bin_dir, o.bin_base[ri], o.fastq ? "fastq" : "fasta", o.gz_out);
            sh.st_bin = bin_before;
        }
    }
    if (v == 1 || (v != 0 && host.file(r))) {               // (give up: the feed and the contexts stay as they are)
        sh.join();
        if (o.bin_reads) sh.bins.discard();
        return 1;
    }
    sh.wait();
    if (o.bin_reads && (!sh.bins.close_all() || sh.bin_failed)) die(3, "writing the reads of " + r + " to " + o.bin_dir + " failed");
    if (fwrite(sh.out_rows.data(), 1, sh.out_rows.size(), stdout) != sh.out_rows.size()) rs.output_failed = true;
    fprintf(stderr, "__process read done__\n");
    return 0;
}

void print_stats(const Run &rs) {
    const Shared &sh = rs.sh;
    fprintf(stderr, "[stats] ingest %s: blocks_framed=%llu records=%llu gz_on_device=%llu fallback=%s\n", rs.feed ? "device" : "host", (unsigned long long)rs.st_blocks,
            (unsigned long long)sh.st_records, (unsigned long long)rs.st_gz, rs.st_fallback.c_str());
    fprintf(stderr, "[stats] seconds: read=%.3f upload=%.3f kernels=%.3f rows=%.3f read_phase=%.3f\n", rs.st_read, rs.st_upload, sh.st_kernels, sh.st_rows, now_s() - rs.t_phase);
    if (rs.o.rows_given)
        fprintf(stderr, "[stats] rows: route=%s views_on_device=%llu views_on_host=%llu bytes=%llu fallback=%s\n", rs.rows_on_device ? "device" : "host",
                (unsigned long long)(rs.rows_on_device ? rs.st_row_views[0] : 0), (unsigned long long)(rs.rows_on_device ? rs.st_row_views[1] : 0),
                (unsigned long long)rs.st_row_bytes, rs.st_rows_fallback.c_str());
    if (rs.o.bin_reads)
        fprintf(stderr, "[stats] bins: haplotype0=%llu haplotype1=%llu ambiguous=%llu bytes_on_device=%llu bytes_on_host=%llu gz=%d\n", (unsigned long long)sh.st_bin.cls[0],
                (unsigned long long)sh.st_bin.cls[1], (unsigned long long)sh.st_bin.cls[2], (unsigned long long)sh.st_bin.dev, (unsigned long long)sh.st_bin.host, rs.o.gz_out ? 1 : 0);
}

}  // namespace

int main(int argc, char **argv) {
    Options o;
    if (!parse_options(argc, argv, o)) return -1;
    Run rs(o);
    fprintf(stderr, "__START__\n");
    load_kmers(rs);
    clone_to_other_gpus(rs);
    HostRoute host(rs);
    create_device_feed(rs);
    std::unique_ptr<DeviceRoute> dev(rs.feed ? new DeviceRoute(rs) : nullptr);
    rs.t_phase = now_s();
    for (size_t ri = 0; ri < o.read.size(); ++ri)
        if (process_input(rs, host, dev.get(), ri)) return 1;
    if (o.stats) print_stats(rs);
    if (rs.feed) hast_rs_destroy(rs.feed);
    // (mkoutput_by_fabulous2.0.sh redirects stdout into a file and goes on: a full disk or a closed pipe must not pass as exit 0)
    if (fflush(stdout) != 0) rs.output_failed = true;
    if (rs.output_failed) {
        fprintf(stderr, "classify: ERROR: writing the result to stdout failed (%s)\n", strerror(errno));
        return 2;
    }
    fprintf(stderr, "__END__\n");
    for (hast_ctx *c : rs.ctxs) hast_ctx_destroy(c);
    return 0;
}

