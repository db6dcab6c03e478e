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
// Requirement (deviation): k-mer lines must be upper-case A/C/G/T of one length K <= 32 -- what jellyfish/meryl
// dumps are.  The reference would also store other bytes literally (s03:59-65); we stop with exit 3 instead.
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <fcntl.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <string_view>
#include <vector>

#include "../../include/hast.h"
#include <zlib.h>

#include "ingest.h"
#include "rb_host.h"
#include "rs_host.h"

namespace {

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
          "  --stats                         counts and seconds of the read phase on stderr\n"
          "  --bin-reads                     also write every input's reads to B.haplotype0|haplotype1|ambiguous.fasta|fastq\n"
          "  --gz-out                        (with --bin-reads) gzip those files, names end in .gz\n"
          "  --bin-dir DIR                   (with --bin-reads) where they go (default: the working directory)\n",
          stderr);
}

// the whole input, front to back (also from a pipe, which has no size to ask for)
bool slurp(const std::string &path, std::vector<char> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    size_t have = 0;
    for (;;) {
        if (out.size() - have < (1u << 20)) out.resize(std::max<size_t>(out.size() * 2, 4u << 20));
        const size_t n = fread(out.data() + have, 1, out.size() - have, f);
        have += n;
        if (n == 0) break;
    }
    const bool ok = !ferror(f);
    fclose(f);
    out.resize(have);
    return ok;
}

// the rows of n reads: names[name_off[i], name_off[i + 1]) and votes[2 i], votes[2 i + 1] -> "name \t haplotypeN|ambiguous \t density"
void format_rows(std::string &out, const uint8_t *names, const uint32_t *name_off, const uint32_t *votes, size_t n, const int *total_kmers) {
    char row[96];
    for (size_t i = 0; i < n; i++) {
        const double d0 = hast::rb::density(votes[2 * i], total_kmers[0]), d1 = hast::rb::density(votes[2 * i + 1], total_kmers[1]);   // s03:215-216
        // s03:110-133 for two haplotypes: both zero -> ambiguous 0.0; else the larger density, ties to haplotype0 (rb_core.h: the bins' rule)
        const uint32_t cls = hast::rb::class_of(d0, d1);
        if (cls == hast::rb::kAmbiguous) snprintf(row, sizeof(row), "\tambiguous\t0.0\n");
        else if (cls == hast::rb::kHap1) snprintf(row, sizeof(row), "\thaplotype1\t%0.6f\n", d1);
        else snprintf(row, sizeof(row), "\thaplotype0\t%0.6f\n", d0);
        out.append(reinterpret_cast<const char *>(names) + name_off[i], name_off[i + 1] - name_off[i]);
        out += row;
    }
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

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int main(int argc, char **argv) {
    static struct option long_options[] = {{"hap", required_argument, NULL, 'p'},    {"read", required_argument, NULL, 'r'},
                                           {"format", required_argument, NULL, 'f'}, {"thread", required_argument, NULL, 't'},
                                           {"help", no_argument, NULL, 'h'},         {"device", required_argument, NULL, 1001},
                                           {"devices", required_argument, NULL, 1002}, {"ingest", required_argument, NULL, 1003},
                                           {"block-mb", required_argument, NULL, 1004}, {"stats", no_argument, NULL, 1005},
                                           {"bin-reads", no_argument, NULL, 1006},   {"gz-out", no_argument, NULL, 1007},
                                           {"bin-dir", required_argument, NULL, 1008},
                                           {0, 0, 0, 0}};
    std::vector<std::string> haps, read;
    std::string format = "fasta";
    int t_num = 8, device = 0;
    std::vector<int> devices;
    bool ingest_device = false, stats = false, bin_reads = false, gz_out = false;
    std::string bin_dir = ".";
    long block_mb = 64;
    for (;;) {
        int c = getopt_long(argc, argv, "p:r:t:f:h", long_options, NULL);   // s03:324
        if (c < 0) break;
        switch (c) {
        case 'p': haps.push_back(optarg); break;
        case 'r': read.push_back(optarg); break;
        case 'f': format = optarg; break;
        case 't': t_num = atoi(optarg); break;
        case 1001: device = atoi(optarg); break;
        case 1002:
            for (const char *q = optarg; *q;) {
                char *end;
                const long v = strtol(q, &end, 10);
                if (end == q || v < 0 || (*end && *end != ',')) { print_usage(); return -1; }
                devices.push_back((int)v);
                q = *end == ',' ? end + 1 : end;
            }
            break;
        case 1003:
            if (strcmp(optarg, "host") != 0 && strcmp(optarg, "device") != 0) { print_usage(); return -1; }
            ingest_device = strcmp(optarg, "device") == 0;
            break;
        case 1004:
            block_mb = atol(optarg);
            if (block_mb < 1 || block_mb > 1024) { print_usage(); return -1; }
            break;
        case 1005: stats = true; break;
        case 1006: bin_reads = true; break;
        case 1007: gz_out = true; break;
        case 1008: bin_dir = optarg; break;
        case 'h':
        default: print_usage(); return -1;
        }
    }
    if (haps.size() != 2 || read.empty() || t_num < 1) {                     // s03:351-354
        print_usage();
        return -1;
    }
    if (gz_out && !bin_reads) {
        print_usage();
        return -1;
    }
    std::vector<std::string> bin_base;                                      // per input: its basename minus a trailing .gz
    if (bin_reads)
        for (const std::string &r : read) {
            std::string b = r.substr(r.find_last_of('/') == std::string::npos ? 0 : r.find_last_of('/') + 1);
            if (b.size() > 3 && b.compare(b.size() - 3, 3, ".gz") == 0) b.resize(b.size() - 3);
            if (std::find(bin_base.begin(), bin_base.end(), b) != bin_base.end()) {   // two inputs would write the same files
                print_usage();
                return -1;
            }
            bin_base.push_back(b);
        }
    if (devices.empty()) devices.push_back(device);
    device = devices[0];
    if (format != "fasta" && format != "fastq") {
        fprintf(stderr, " ERROR : invalid format : [%s] . exit ...\n", format.c_str());
        return -1;
    }
    fprintf(stderr, "__START__\n");
    // ---- load_kmers (s03:51-70) --------------------------------------------------------------------
    // K = length of the first line of the first file (s03:57-58); regular files are streamed into the table by the library,
    // which also checks on the device that every line is K upper-case A/C/G/T bytes; anything else is read into memory first
    // (a pipe can be read only once: it is read whole now and its first bytes serve as the head)
    std::vector<char> txt[2], head;
    bool streamed[2] = {false, false};
    size_t text_bytes[2] = {0, 0};
    for (int h = 0; h < 2; h++) {
        struct stat sb;
        if (stat(haps[h].c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) {
            streamed[h] = true;
            text_bytes[h] = (size_t)sb.st_size;
        } else {
            if (!slurp(haps[h], txt[h])) die(2, "cannot read " + haps[h]);
            text_bytes[h] = txt[h].size();
        }
    }
    if (streamed[0]) {
        FILE *f = fopen(haps[0].c_str(), "rb");
        if (!f) die(2, "cannot read " + haps[0]);
        head.resize(4096);
        head.resize(fread(head.data(), 1, head.size(), f));
        fclose(f);
    } else head.assign(txt[0].begin(), txt[0].begin() + (long)std::min<size_t>(txt[0].size(), 4096));
    const void *nl0 = memchr(head.data(), '\n', head.size());
    const size_t K = nl0 ? (size_t)((const char *)nl0 - head.data()) : head.size();   // s03:57-58
    if (K < 1 || K > 32) die(3, "K (length of the first k-mer line) must be in [1,32]");
    hast_ctx *ctx = nullptr;
    if (hast_ctx_create(device, (int)K, &ctx) != HAST_OK) die(4, "cannot create GPU context");
    if (hast_ctx_set_text_check(ctx, 1) != HAST_OK) die(4, "cannot create GPU context");
    if (hast_table_reserve(ctx, text_bytes[0] / (K + 1) + text_bytes[1] / (K + 1) + 2, 0.0) != HAST_OK) die(4, "allocating the k-mer table");
    int total_kmers[2] = {0, 0};                                             // s03:50,68 (an `int` in the reference)
    for (int h = 0; h < 2; h++) {
        fprintf(stderr, "__load hap%d kmers__\n", h);
        uint64_t lines = 0;
        hast_status st;
        if (streamed[h]) st = hast_table_insert_text_file(ctx, h, haps[h].c_str(), &lines);
        else {
            // complete lines only: a trailing piece without '\n' is dropped (s03:63) -- except a lone first line
            size_t usable = txt[h].size();
            while (usable && txt[h][usable - 1] != '\n') usable--;
            st = hast_table_insert_text(ctx, h, txt[h].data(), usable, &lines);
        }
        if (st == HAST_ERR_FORMAT) die(3, std::string(hast_last_error()) + " (k-mer files must hold one K-mer of upper-case A/C/G/T per line)");
        if (st == HAST_ERR_IO) die(2, "cannot read " + haps[h]);
        if (st != HAST_OK) die(4, "building the k-mer table");
        if (h == 0 && !nl0 && text_bytes[0] == K) {
            for (size_t i = 0; i < K; i++)
                if (!strchr("ACGT", head[i])) die(3, "k-mer files must hold upper-case A/C/G/T lines only");
            uint64_t key = hast_canon_kmer(head.data(), (int)K);
            if (hast_table_insert_keys(ctx, 0, &key, 1) != HAST_OK) die(4, "building the k-mer table");
            lines = 1;
        }
        total_kmers[h] = (int)lines;
        fprintf(stderr, "Recorded %d haplotype %d specific %zu-mers\n", total_kmers[h], h, K);
        std::vector<char>().swap(txt[h]);
    }
    // the other GPUs get a copy of the finished table, peer to peer
    std::vector<hast_ctx *> ctxs{ctx};
    for (size_t i = 1; i < devices.size(); i++) {
        hast_ctx *c2 = nullptr;
        if (hast_ctx_create(devices[i], (int)K, &c2) != HAST_OK) die(4, "cannot create GPU context");
        ctxs.push_back(c2);
    }
    if (ctxs.size() > 1) {
        // (all at once: every GPU pulls its copy over its own xGMI link; the source's filter is built first, the clones only read the source)
        if (hast_filter_build(ctx) != HAST_OK) die(4, "building the k-mer filter");
        std::vector<std::thread> cloners;
        std::vector<int> failed(ctxs.size(), 0);
        for (size_t i = 1; i < ctxs.size(); i++)
            cloners.emplace_back([&, i] { failed[i] = hast_table_clone(ctxs[i], ctx) != HAST_OK; });
        for (std::thread &t : cloners) t.join();
        for (int f : failed)
            if (f) die(4, "copying the k-mer table to another GPU");
    }
    // ---- reads: block ingest with t_num parser threads (ingest.h), one GPU batch per block ------------------------
    // Framing as in the reference: FASTQ = 4 getlines per record, the header must be newline-terminated (s03:255-263);
    // FASTA = '>' lines start a record, other non-empty lines are appended, a last line without '\n' is dropped
    // (s03:279-296).  Rows of a file are printed when the file is done, like PrintOutput after the loop (s03:269,301).
    hast::WorkerPool pool(t_num);
    const int T = pool.size();
    std::vector<std::vector<uint32_t>> nl(T);
    std::vector<uint32_t> allnl;
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets;
    std::vector<std::string> names;
    std::vector<uint64_t> part(T + 1);
    std::vector<int> bad(T);
    std::string out_rows;
    const bool fastq = format == "fastq";
    // Classify the parsed batch (names/offsets/bases) and append its rows.  The batch is handed to ONE background thread (rows
    // stay in order) so that the upload, the kernel and the formatting of block i run while block i+1 is indexed and copied.
    struct Batch {
        std::vector<uint8_t> bases;
        std::vector<uint64_t> offsets;
        std::vector<std::string> names;
        std::string raw;                                    // --bin-reads: the view the records lie in, and their extents in it
        std::vector<hast::rb::Extent> ext;
    };
    BinFiles bins;
    hast::rb::Runs bin_runs;                                // the background thread's while a batch is in flight
    bool bin_failed = false;
    uint64_t st_bin[3] = {0, 0, 0}, st_bin_dev = 0, st_bin_host = 0;
    const uint32_t bin_total[2] = {(uint32_t)total_kmers[0], (uint32_t)total_kmers[1]};
    std::string raw;                                        // what classify_batch hands on with the batch
    std::vector<hast::rb::Extent> ext;
    // the runs of the host model into the input's files
    auto flush_runs = [&]() {
        if (!bins.write_runs(bin_runs)) bin_failed = true;
        for (int c = 0; c < 3; ++c) {
            st_bin[c] += bin_runs.count[c];
            st_bin_host += bin_runs.run[c].size();
        }
        bin_runs.clear();
    };
    std::thread bg;
    struct Joiner {                                         // every way out of main() waits for the batch in flight
        std::thread &t;
        ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{bg};
    Batch bt[2];                                            // the batch in flight and the one before it (its buffers are reused)
    int cur = 0;
    std::string bg_error;
    // what --stats prints; the background thread adds to records / kernels / rows, and is joined before they are read
    uint64_t st_blocks = 0, st_records = 0, st_gz = 0;
    double st_read = 0, st_upload = 0, st_kernels = 0, st_rows = 0;
    std::string st_fallback = "none";
    auto wait_bg = [&]() {
        if (bg.joinable()) bg.join();
        if (!bg_error.empty()) die(4, bg_error);
    };
    auto run_batch = [&](Batch &b) {
        if (b.names.empty()) return;
        const size_t n = b.names.size(), G = ctxs.size();
        const double t0 = now_s();
        std::vector<uint32_t> v(n * 2, 0);
        if (G == 1) {
            if (hast_classify_perread(ctx, b.bases.data(), b.offsets.data(), n, v.data()) != HAST_OK) {
                bg_error = std::string("classifying a batch (") + hast_last_error() + ")";
                return;
            }
        } else {
            // one contiguous share of the reads per GPU, cut where the bases divide evenly (reads differ in length by orders of
            // magnitude); the shares run at the same time, every one on a thread of its own (a context is driven by one thread)
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
                th.emplace_back([&, g] {
                    const size_t lo = cut[g], hi = cut[g + 1];
                    if (hi > lo && hast_classify_perread(ctxs[g], b.bases.data(), b.offsets.data() + lo, hi - lo, v.data() + 2 * lo) != HAST_OK)
                        errs[g] = hast_last_error();
                });
            for (std::thread &t : th) t.join();
            for (const std::string &e : errs)
                if (!e.empty()) {
                    bg_error = "classifying a batch (" + e + ")";
                    return;
                }
        }
        const double t1 = now_s();
        for (size_t i = 0; i < n; i++) {
            const uint32_t off[2] = {0, (uint32_t)b.names[i].size()};
            format_rows(out_rows, reinterpret_cast<const uint8_t *>(b.names[i].data()), off, v.data() + 2 * i, 1, total_kmers);
        }
        if (bin_reads && b.ext.size() == n) {
            hast::rb::append_runs(reinterpret_cast<const uint8_t *>(b.raw.data()), b.ext.data(), v.data(), n, bin_total[0], bin_total[1], &bin_runs);
            flush_runs();
        }
        st_records += n;
        st_kernels += t1 - t0;
        st_rows += now_s() - t1;
    };
    auto classify_batch = [&]() {
        wait_bg();                                          // one batch in flight; its rows are in out_rows now
        if (names.empty()) return;
        Batch &b = bt[cur];
        b.bases.swap(bases);
        b.offsets.swap(offsets);
        b.names.swap(names);
        b.raw.swap(raw);
        b.ext.swap(ext);
        bg = std::thread([&run_batch, &b] { run_batch(b); });
        cur ^= 1;
        Batch &o = bt[cur];                                 // idle since the wait above: its vectors (and their capacity) are the next work area
        bases.swap(o.bases);
        offsets.swap(o.offsets);
        names.swap(o.names);
        raw.clear();
        ext.clear();
    };
    // records = [first, last) pairs of line indices: header line, then sequence lines; fills names/offsets/bases in parallel
    struct RecSpan { uint32_t head, seq_first, seq_end; };             // line indices; sequence lines [seq_first, seq_end)
    std::vector<RecSpan> recs;
    auto line_start = [&](size_t i) -> size_t { return i ? (size_t)allnl[i - 1] + 1 : 0; };
    auto build_batch = [&](const char *data) {
        const size_t n = recs.size();
        names.assign(n, std::string());
        offsets.assign(n + 1, 0);
        if (n == 0) { bases.clear(); return; }
        std::vector<uint64_t> len(n);
        pool.run([&](int t) {
            uint64_t sum = 0;
            for (size_t i = n * (size_t)t / T; i < n * (size_t)(t + 1) / T; i++) {
                const RecSpan &r = recs[i];
                uint64_t l = 0;
                if (r.seq_end > r.seq_first) l = ((uint64_t)allnl[r.seq_end - 1] - line_start(r.seq_first)) - (r.seq_end - r.seq_first - 1);
                len[i] = l;
                sum += l;
            }
            part[t + 1] = sum;
        });
        part[0] = 0;
        for (int t = 0; t < T; t++) part[t + 1] += part[t];
        bases.resize(part[T] + 16);
        pool.run([&](int t) {
            uint64_t off = part[t];
            for (size_t i = n * (size_t)t / T; i < n * (size_t)(t + 1) / T; i++) {
                const RecSpan &r = recs[i];
                const size_t hs = line_start(r.head), he = allnl[r.head];
                names[i].assign(data + hs + (he > hs ? 1 : 0), data + he);               // head.substr(1), s03:207
                offsets[i] = off;
                for (uint32_t li = r.seq_first; li < r.seq_end; li++) {
                    const size_t ls = line_start(li), le = allnl[li];
                    memcpy(bases.data() + off, data + ls, le - ls);
                    off += le - ls;
                }
            }
        });
        offsets[n] = part[T];
        if (bin_reads) {                                    // the records' extents (rb_core.h) and the bytes they lie in, for the background thread
            ext.resize(n);
            uint64_t end = 0;
            for (size_t i = 0; i < n; i++) {
                const RecSpan &r = recs[i];
                ext[i].lo = line_start(r.head);
                ext[i].hi = fastq ? (uint64_t)allnl[r.head + 3] + 1 : line_start(r.seq_end);
                end = ext[i].hi;
            }
            raw.assign(data, end);
        }
    };
    // the FASTQ tail as a record of the bins: its bytes as they lie, plus a newline if they do not end in one (rb_host.h: append_tail)
    auto bin_tail = [&](const char *tail, size_t n_tail) {
        if (!bin_reads || names.empty()) return;
        raw.assign(tail, n_tail);
        if (raw.back() != '\n') raw += '\n';
        ext.assign(1, hast::rb::Extent{0, raw.size()});
    };
    const size_t block_bytes = (size_t)std::max(1L, getenv("HAST_READ_BLOCK_BYTES") ? atol(getenv("HAST_READ_BLOCK_BYTES")) : (256L << 20));
    bool output_failed = false;
    // the host route for one input: its rows into out_rows; 1: the format error (its message is printed)
    auto host_file = [&](const std::string &r) -> int {
        hast::BlockSource src;
        if (!src.open(r, block_bytes)) die(2, "cannot open " + r);
        std::vector<char> carry;
        wait_bg();
        out_rows.clear();
        bool seen_header = false;                       // FASTA: lines before the first '>' belong to no record (s03:286-292)
        for (;;) {
            const double t_read = now_s();
            std::vector<char> blk = src.next();
            st_read += now_s() - t_read;
            const bool last = blk.empty();
            if (last && !src.error().empty()) die(2, r + ": " + src.error());
            constexpr size_t kPad = hast::BlockSource::kFrontPad;
            const char *data;
            size_t len;
            if (last) { data = carry.data(); len = carry.size(); }
            else if (carry.size() <= kPad) {
                if (!carry.empty()) memcpy(blk.data() + kPad - carry.size(), carry.data(), carry.size());
                data = blk.data() + kPad - carry.size();
                len = blk.size() - kPad + carry.size();
            } else {
                carry.insert(carry.end(), blk.begin() + kPad, blk.end());
                data = carry.data();
                len = carry.size();
            }
            if (len >= (1ull << 32)) die(3, "a single record spans more than 4 GB");
            pool.run([&](int t) {
                auto &v = nl[t];
                v.clear();
                const char *p = data + len * (size_t)t / T, *e = data + len * (size_t)(t + 1) / T;
                while (p < e && (p = (const char *)memchr(p, '\n', (size_t)(e - p)))) { v.push_back((uint32_t)(p - data)); ++p; }
            });
            allnl.clear();
            for (int t = 0; t < T; t++) allnl.insert(allnl.end(), nl[t].begin(), nl[t].end());
            const size_t n_lines = allnl.size();                 // complete ('\n'-terminated) lines in the work area
            recs.clear();
            size_t consumed = 0;
            if (fastq) {
                const size_t n_rec = n_lines / 4;
                for (size_t i = 0; i < n_rec; i++) recs.push_back({(uint32_t)(4 * i), (uint32_t)(4 * i + 1), (uint32_t)(4 * i + 2)});
                consumed = n_rec ? (size_t)allnl[4 * n_rec - 1] + 1 : 0;
                if (last && n_lines % 4 >= 1) {
                    // tail: header terminated; bases = next piece, terminated or not (s03:260); the tail becomes a full record,
                    // handled after the block's records, as a one-record batch
                    for (const RecSpan &x : recs)
                        if (data[line_start(x.head)] == '>') { fprintf(stderr, "fasta detected . ERROR . please use \"--format fasta\". exit ... \n"); return 1; }
                    build_batch(data);
                    classify_batch();
                    if (!tail_batch(data + consumed, len - consumed, names, bases, offsets)) { fprintf(stderr, "fasta detected . ERROR . please use \"--format fasta\". exit ... \n"); return 1; }
                    bin_tail(data + consumed, len - consumed);
                    classify_batch();
                    break;
                }
                for (const RecSpan &x : recs)
                    if (len && data[line_start(x.head)] == '>') { fprintf(stderr, "fasta detected . ERROR . please use \"--format fasta\". exit ... \n"); return 1; }
            } else {
                // header lines (first byte '>'); '@'/'+' at the start of a non-empty line is the reference's format error
                std::vector<std::vector<uint32_t>> hl(T);
                pool.run([&](int t) {
                    bad[t] = 0;
                    hl[t].clear();
                    for (size_t i = n_lines * (size_t)t / T; i < n_lines * (size_t)(t + 1) / T; i++) {
                        const size_t ls = line_start(i);
                        if (allnl[i] == ls) continue;                                       // empty line: skipped (s03:280)
                        const char c = data[ls];
                        if (c == '>') hl[t].push_back((uint32_t)i);
                        else if (c == '@' || c == '+') bad[t] = 1;
                    }
                });
                std::vector<uint32_t> heads;
                for (int t = 0; t < T; t++) {
                    if (bad[t]) { fprintf(stderr, "fasta detected . ERROR . please use \"--format fastq\". exit ... \n"); return 1; }
                    heads.insert(heads.end(), hl[t].begin(), hl[t].end());
                }
                // complete records: header j .. header j+1; at EOF the last header's record ends at the last complete line
                for (size_t j = 0; j + 1 < heads.size(); j++) recs.push_back({heads[j], heads[j] + 1, heads[j + 1]});
                if (last && !heads.empty()) recs.push_back({heads.back(), heads.back() + 1, (uint32_t)n_lines});
                if (!heads.empty()) seen_header = true;
                if (last) consumed = len;
                else if (!heads.empty()) consumed = line_start(heads.back());      // carry the (possibly incomplete) last record
                else consumed = seen_header ? 0 : (n_lines ? (size_t)allnl[n_lines - 1] + 1 : 0);   // no header yet: drop complete lines
            }
            build_batch(data);
            classify_batch();
            if (last) break;
            std::vector<char> keep(data + consumed, data + len);
            carry.swap(keep);
            src.recycle(std::move(blk));
        }
        return 0;
    };
    // ---- --ingest device: one feed on the context's GPU (hast_rs_*) ---------------------------------------------------------
    hast_rs *feed = nullptr;
    size_t rs_block = (size_t)block_mb << 20;
    if (getenv("HAST_RS_BLOCK")) rs_block = (size_t)std::max(64L, atol(getenv("HAST_RS_BLOCK")));
    if (ingest_device && ctxs.size() > 1) {
        fprintf(stderr, "classify_read: WARN: --ingest device takes one GPU: host ingest for this run (fallback=several_devices)\n");
        st_fallback = "several_devices";
        ingest_device = false;
    }
    if (ingest_device && hast_rs_create(ctx, fastq ? HAST_RS_FASTQ : HAST_RS_FASTA, rs_block, &feed) != HAST_OK) die(4, "cannot create the device ingest");
    if (feed && bin_reads && hast_rs_set_bins(feed, gz_out ? 2 : 1, bin_total[0], bin_total[1]) != HAST_OK) die(4, "cannot create the device ingest's bins");
    std::vector<uint8_t> rs_tail;
    // the device route for one input: its rows into out_rows; 1: the format error (its message is printed), 2: a record too long
    auto device_file = [&](const std::string &r) -> int {
        const size_t n = r.size();
        hast_gz *z = nullptr;
        if (n > 3 && r.compare(n - 3, 3, ".gz") == 0 && hast_gz_open(ctx, r.c_str(), &z) != HAST_OK) z = nullptr;   // (BGZF, not gzip, unreadable: BlockSource's words)
        int fd = -1;
        hast::BlockSource src;
        const bool plain = !(n > 3 && r.compare(n - 3, 3, ".gz") == 0);
        if (z) ++st_gz;
        else if (plain) {
            if ((fd = open(r.c_str(), O_RDONLY)) < 0) die(2, "cannot open " + r);
        } else if (!src.open(r, rs_block)) die(2, "cannot open " + r);
        out_rows.clear();
        int pending = 0, verdict = 0;
        uint64_t framed_records = 0;                             // counted once the file is through: a refused file is read again
        // frame and classify the oldest submitted block, format its rows
        auto step = [&]() {
            hast_rs_block b;
            hast_rs_binned rb;
            const double t0 = now_s();
            if ((bin_reads ? hast_rs_next_binned(feed, &b, &rb) : hast_rs_next(feed, &b)) != HAST_OK) die(4, "framing and classifying a block");
            const double t1 = now_s();
            --pending;
            ++st_blocks;
            st_kernels += t1 - t0;
            if (b.flags & HAST_RS_FORMAT_ERROR) verdict = 1;
            else if (b.flags & HAST_RS_RECORD_TOO_LONG) verdict = 2;
            if (verdict) return;
            format_rows(out_rows, b.names, b.name_off, b.votes, (size_t)b.records, total_kmers);
            framed_records += b.records;
            if (bin_reads)
                for (int c = 0; c < 3; ++c) {
                    if (!bins.write(c, rb.run[c], (size_t)rb.run_bytes[c])) bin_failed = true;
                    st_bin[c] += rb.count[c];
                    st_bin_dev += rb.raw_bytes[c];
                }
            st_rows += now_s() - t1;
        };
        auto submit = [&](size_t n_bytes, bool last) {           // ... and keep one block ahead of the framer
            const double t0 = now_s();
            if (hast_rs_submit(feed, n_bytes, last) != HAST_OK) die(4, "submitting a block");
            st_upload += now_s() - t0;
            ++pending;
            if (pending == 2) step();
        };
        auto host_block = [&]() {
            uint8_t *h = nullptr;
            const double t0 = now_s();
            if (hast_rs_host_block(feed, &h) != HAST_OK) die(4, "the device ingest's staging block");
            st_upload += now_s() - t0;
            return h;
        };
        bool ended = false;                                      // the file's last block has been submitted
        std::vector<char> blk;
        size_t blk_at = 0;
        while (!verdict && !ended) {
            size_t got = 0;
            const double t0 = now_s();
            if (z) {
                uint8_t *d = nullptr;
                hast_stream fill = nullptr;
                if (hast_rs_device_block(feed, &d, &fill) != HAST_OK) die(4, "the device ingest's block");
                if (hast_gz_read_device(z, d, rs_block, &got, fill) != HAST_OK) die(2, r + ": " + hast_last_error());
            } else if (plain) {
                uint8_t *h = host_block();
                while (got < rs_block) {
                    const ssize_t k = ::read(fd, h + got, rs_block - got);
                    if (k < 0 && errno == EINTR) continue;
                    if (k < 0) die(2, r + ": " + strerror(errno));
                    if (k == 0) break;
                    got += (size_t)k;
                }
            } else {
                constexpr size_t kPad = hast::BlockSource::kFrontPad;
                if (blk_at >= blk.size()) {
                    if (!blk.empty()) src.recycle(std::move(blk));
                    blk = src.next();
                    blk_at = kPad;
                    if (blk.empty() && !src.error().empty()) die(2, r + ": " + src.error());
                }
                uint8_t *h = host_block();
                got = blk.empty() ? 0 : std::min(rs_block, blk.size() - blk_at);
                if (got) memcpy(h, blk.data() + blk_at, got);
                blk_at += got;
            }
            st_read += now_s() - t0;
            ended = got == 0;                                    // (only a read that returns nothing ends the stream, include/hast.h)
            submit(got, ended);
        }
        if (!ended) {                                            // given up: the feed wants the file's last block all the same
            if (!z) (void)host_block();
            else {
                uint8_t *d = nullptr;
                if (hast_rs_device_block(feed, &d, nullptr) != HAST_OK) die(4, "the device ingest's block");
            }
            submit(0, true);
        }
        while (pending) step();                                  // (before the decoder goes: its kernels wrote the blocks still waiting)
        if (z) hast_gz_close(z);
        if (fd >= 0) close(fd);
        if (!verdict) st_records += framed_records;
        if (!verdict && fastq) {
            size_t n_tail = 0;
            rs_tail.resize(rs_block);
            if (hast_rs_take_tail(feed, rs_tail.data(), &n_tail) != HAST_OK) die(4, "the end of the input");
            Batch tb;
            if (!tail_batch(reinterpret_cast<const char *>(rs_tail.data()), n_tail, tb.names, tb.bases, tb.offsets)) verdict = 1;
            else {
                if (bin_reads && !tb.names.empty()) {
                    tb.raw.assign(reinterpret_cast<const char *>(rs_tail.data()), n_tail);
                    if (tb.raw.back() != '\n') tb.raw += '\n';
                    tb.ext.assign(1, hast::rb::Extent{0, tb.raw.size()});
                }
                run_batch(tb);
                if (!bg_error.empty()) die(4, bg_error);
            }
        }
        if (verdict == 1) fprintf(stderr, fastq ? "fasta detected . ERROR . please use \"--format fasta\". exit ... \n" : "fasta detected . ERROR . please use \"--format fastq\". exit ... \n");
        return verdict;
    };
    const double t_phase = now_s();
    // the format error: the input leaves no files, as it leaves no rows
    auto give_up = [&]() {
        if (bg.joinable()) bg.join();
        if (bin_reads) bins.discard();
        return 1;
    };
    for (size_t ri = 0; ri < read.size(); ++ri) {
        const std::string &r = read[ri];
        fprintf(stderr, "__process read: %s\n", r.c_str());
        if (bin_reads) bins.start(bin_dir, bin_base[ri], fastq ? "fastq" : "fasta", gz_out);
        const uint64_t bin_before[5] = {st_bin[0], st_bin[1], st_bin[2], st_bin_dev, st_bin_host};
        bool on_device = false;
        if (feed) {
            struct stat sb;
            if (stat(r.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) {
                fprintf(stderr, "classify_read: WARN: %s is not a regular file: host ingest for this input (fallback=not_a_regular_file)\n", r.c_str());
                st_fallback = "not_a_regular_file";
            } else {
                const int v = device_file(r);
                if (v == 1) return give_up();
                on_device = v == 0;
                if (v == 2) {
                    fprintf(stderr, "classify_read: WARN: a record of %s does not fit two blocks of %zu bytes: host ingest for this input (fallback=record_too_long)\n",
                            r.c_str(), rs_block);
                    st_fallback = "record_too_long";
                    if (bin_reads) {                             // the file is read again from its start: so are its bins
                        bins.discard();
                        bins.start(bin_dir, bin_base[ri], fastq ? "fastq" : "fasta", gz_out);
                        st_bin[0] = bin_before[0], st_bin[1] = bin_before[1], st_bin[2] = bin_before[2];
                        st_bin_dev = bin_before[3], st_bin_host = bin_before[4];
                    }
                }
            }
        }
        if (!on_device && host_file(r)) return give_up();
        wait_bg();
        if (bin_reads && (!bins.close_all() || bin_failed)) die(3, "writing the reads of " + r + " to " + bin_dir + " failed");
        if (fwrite(out_rows.data(), 1, out_rows.size(), stdout) != out_rows.size()) output_failed = true;
        fprintf(stderr, "__process read done__\n");
    }
    if (stats) {
        fprintf(stderr, "[stats] ingest %s: blocks_framed=%llu records=%llu gz_on_device=%llu fallback=%s\n", feed ? "device" : "host", (unsigned long long)st_blocks,
                (unsigned long long)st_records, (unsigned long long)st_gz, st_fallback.c_str());
        fprintf(stderr, "[stats] seconds: read=%.3f upload=%.3f kernels=%.3f rows=%.3f read_phase=%.3f\n", st_read, st_upload, st_kernels, st_rows, now_s() - t_phase);
        if (bin_reads)
            fprintf(stderr, "[stats] bins: haplotype0=%llu haplotype1=%llu ambiguous=%llu bytes_on_device=%llu bytes_on_host=%llu gz=%d\n", (unsigned long long)st_bin[0],
                    (unsigned long long)st_bin[1], (unsigned long long)st_bin[2], (unsigned long long)st_bin_dev, (unsigned long long)st_bin_host, gz_out ? 1 : 0);
    }
    if (feed) hast_rs_destroy(feed);
    // (mkoutput_by_fabulous2.0.sh redirects stdout into a file and goes on: a full disk or a closed pipe must not pass as exit 0)
    if (fflush(stdout) != 0) output_failed = true;
    if (output_failed) {
        fprintf(stderr, "classify: ERROR: writing the result to stdout failed (%s)\n", strerror(errno));
        return 2;
    }
    fprintf(stderr, "__END__\n");
    for (hast_ctx *c : ctxs) hast_ctx_destroy(c);
    return 0;
}
