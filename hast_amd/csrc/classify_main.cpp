// classify_main.cpp -- the drop-in `classify` executable for HAST stage 01 on MI355X.
//
// Same command line, same stdout rows and same stderr skeleton as the reference program
// (/root/reference/01.classify_stlfr_reads/classify.cpp:373-450), so
// 01.classify_stlfr_reads/classify_stlfr_reads.sh:148-149 runs unchanged against it.  All k-mer
// work (table build, adaptor scrub, read classification) happens on the GPU through the C ABI of
// include/hast.h; this file only does what the reference does on the host around it: flag parsing,
// FASTQ framing, barcode names -> dense ids, getHap + printing.
//
// Deliberate, documented deviations (all on inputs the reference does not survive either):
//   * unopenable k-mer/read file: error + exit 2 (the reference loops forever, classify.cpp:41);
//   * ragged k-mer line / read shorter than K: error + exit 3 (the reference assert-aborts,
//     kmer.h:154,171);
//   * K must be in [1,32] like the reference's correct range (it is silently wrong above 32).
// Additive flags: --device N (GPU ordinal, default 0), --devices A,B,... (several GPUs of this node: the table is built
// on the first one and copied to the others over xGMI; the BLOCKS of every input file are dealt to the GPUs in turn and framed
// there -- the reference spreads the reads of one file over all its workers, classify.cpp:211-219 -- (HAST_DEAL=files: whole
// files in turn, as round 2 did; --host-parse: host-framed batches in turn); the per-barcode counters are
// summed with ONE RCCL all-reduce at the end -- the thread merge of classify.cpp:226-229,276-277 across GPUs; integer sums,
// so stdout is byte-identical to a single-GPU run), --block-mb N (ingest block size), --batch-reads N
// (approximate records per GPU batch, for tests), --initial-barcodes N, --stats (timings on stderr), --host-parse (frame the
// FASTQ records on the host as round 1 did; default: raw file bytes go to the GPU and are framed there, hast_fq_*).
// -t/--thread N is honoured as the number of host parser threads.
//
// Layout: main(), at the end, is the list of the run's phases; each phase is a function above it, in that order.  What the command
// line asked for is an Options, what one phase leaves to the next is a Run.  One input file on its way to the GPU framer -- reader
// thread, queues, submit -- is fq_feed.h, which both passes over the inputs (classification, --phase-reads routing) use.
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <deque>
#include <future>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/hast.h"
#include "cli_common.h"
#include "fq_feed.h"
#include "ingest.h"
#include "quartering.h"

namespace {

using hast::now_s;
namespace sw = hast::sw;
using hast::parse_count;

void logtime() {                                  // classify.cpp:17-21
    time_t now = time(0);
    fprintf(stderr, "%s\n", ctime(&now));
}

void print_usage() {                              // same flags as the reference (classify.cpp:375-387); stderr is free-form
    fputs("\nclassify (MI355X) -- per-barcode haplotype votes for stLFR reads\n\n"
          "  classify --hap0 PATERNAL.mer --hap1 MATERNAL.mer --read READS.fq[.gz] [--read ...] [options]\n\n"
          "  -p, --hap0 FILE       parent-0 specific k-mers, one per line (K = length of the first line, K <= 32)\n"
          "  -m, --hap1 FILE       parent-1 specific k-mers\n"
          "  -r, --read FILE       child reads, 4-line FASTQ; gzip if the name ends in .gz; may be repeated\n"
          "  -t, --thread N        host parser threads (default 8)\n"
          "  -w, --weight0 F       weight of hap0 in the call (default 1.0)\n"
          "  -u, --weight1 F       weight of hap1 in the call (default 1.0)\n"
          "  -f, --adaptor_f SEQ   forward adaptor whose k-mers are removed from both sets\n"
          "  -q, --adaptor_r SEQ   reverse adaptor whose k-mers are removed from both sets\n"
          "      --device N        GPU ordinal (default 0)\n"
          "      --devices A,B,..  classify on several GPUs of this node (reads are dealt out, counts summed over RCCL)\n"
          "      --save-table FILE write the built k-mer table (after the adaptor scrub) as a binary key set\n"
          "      --load-table FILE use such a file instead of --hap0/--hap1\n"
          "      --stats           timings and set sizes on stderr\n"
          "      --stats-json FILE the same as one JSON object (- = stderr)\n"
          "      --phase-reads     also do the wrapper's steps 10-11: write the three barcode lists and route every record of every\n"
          "                        input to <name>.{paternal,maternal,homozygous,nobarcode}.fastq (HAST_PHASE_READS=1)\n"
          "      --gz-out          with --phase-reads: the four files are gzip, <name>.<class>.fastq.gz; records routed on the GPU are\n"
          "                        compressed there and only compressed bytes come back (HAST_PHASE_GZ=1)\n"
          "      --gz-format FMT   with --gz-out: gzip (default) | bgzf: every member written, on the GPU or by the host, is blocked gzip\n"
          "                        (BGZF, at most 48 KB of records a member) and every file ends with BGZF's end-of-file block: gzip -dc\n"
          "                        reads the files as before, bgzip / htslib readers and --bgzf device can split them (HAST_PHASE_GZ_FORMAT)\n"
          "      --route MODE      device (default): records routed on the GPU; host: parsed again by host threads\n"
          "      --inflate MODE    device (default) | host | zlib: who inflates .gz inputs (HAST_INFLATE)\n"
          "      --bgzf MODE       host (default) | device: who inflates blocked-gzip (BGZF) inputs (HAST_BGZF)\n"
          "      --gz-ring-bytes N compressed bytes of a .gz input kept on the device at a time (default: whole files up to 2 GB;\n"
          "                        HAST_GZ_RING_BYTES)\n"
          "      --park-gb X       device memory of closed streams kept for reuse instead of freed (default 32; HAST_PARK_GB)\n"
          "      --name-cache N    barcodes the device-side dictionary holds (default 16M; HAST_NAME_CACHE); what it cannot hold is\n"
          "                        numbered by the host\n"
          "                        (N: digits, optionally followed by K, M or G = 2^10, 2^20, 2^30; X: a decimal number such as 1.5)\n"
          "      --deal MODE       with --devices: blocks (default) | files (HAST_DEAL)\n"
          "      --rows MODE       host (default) | device: who sorts and formats the output table, and with --phase-reads the three\n"
          "                        barcode lists: host threads, or the GPU, from which only the finished text comes back (HAST_ROWS);\n"
          "                        a run the GPU cannot do this for says why (fallback=...) and does it on the host, same bytes\n"
          "  -h, --help            this text\n\n"
          "stdout: barcode <TAB> haplotype(0/1/-1) <TAB> hits_hap0 <TAB> hits_hap1, sorted by barcode\n\n",
          stderr);
}

[[noreturn]] void die(int code, const char *what) {
    fprintf(stderr, "classify: ERROR: %s", what);
    const char *e = hast_last_error();
    if (e && *e) fprintf(stderr, " (%s)", e);
    fputc('\n', stderr);
    // (no destructors: reader / inflate threads of the library may be at work, and nothing is left to save)
    fflush(stdout);
    fflush(stderr);
    _exit(code);
}
#define CK(call, what) do { if ((call) != HAST_OK) die(4, what); } while (0)
[[noreturn]] void die_output() {
    fprintf(stderr, "classify: ERROR: writing the result to stdout failed (%s)\n", strerror(errno));
    fflush(stderr);
    _exit(2);
}

// --stats: every "__stats_<section>__ key=value ..." line goes to stderr and is kept for --stats-json FILE, which writes the same
// numbers as ONE JSON object {"section": {"key": value, ...}, ...} (a section printed several times, e.g. one line per .gz input,
// becomes an array) -- SURVEY section 5's machine-readable summary.
struct StatLog {
    std::mutex mu;
    std::vector<std::string> lines;
};
StatLog &stat_log() {
    static StatLog *l = new StatLog();
    return *l;
}
void stat_line(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void stat_line(const char *fmt, ...) {
    char buf[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    fputs(buf, stderr);
    std::string l(buf);
    while (!l.empty() && l.back() == '\n') l.pop_back();
    std::lock_guard<std::mutex> g(stat_log().mu);
    stat_log().lines.push_back(std::move(l));
}
bool write_stats_json(const std::string &path) {
    std::vector<std::string> lines;
    {
        std::lock_guard<std::mutex> g(stat_log().mu);
        lines = stat_log().lines;
    }
    auto quote = [](const std::string &v) {
        std::string o = "\"";
        for (char c : v) {
            if (c == '"' || c == '\\') { o.push_back('\\'); o.push_back(c); }
            else if ((unsigned char)c < 0x20) { char t[8]; snprintf(t, sizeof(t), "\\u%04x", c); o += t; }
            else o.push_back(c);
        }
        return o + "\"";
    };
    auto is_number = [](const std::string &v) {
        if (v.empty()) return false;
        char *end = nullptr;
        (void)strtod(v.c_str(), &end);
        if (*end) return false;
        const char c0 = v[0] == '-' ? (v.size() > 1 ? v[1] : 'x') : v[0];        // (JSON numbers: no hex, inf, nan, leading '+' or '.')
        return c0 >= '0' && c0 <= '9' && v.find_first_of("xXnN") == std::string::npos && !(v.size() > 1 && v[0] == '0' && v[1] >= '0' && v[1] <= '9');
    };
    std::vector<std::pair<std::string, std::vector<std::string>>> sections;       // name -> one object per line, in order of appearance
    for (const std::string &l : lines) {
        size_t sp = l.find(' ');
        std::string name = l.substr(0, sp);
        while (!name.empty() && name.front() == '_') name.erase(name.begin());
        while (!name.empty() && name.back() == '_') name.pop_back();
        std::string obj = "{";
        bool first = true;
        while (sp != std::string::npos) {
            const size_t a = sp + 1, b = l.find(' ', a);
            const std::string tok = l.substr(a, b == std::string::npos ? std::string::npos : b - a);
            sp = b;
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || eq == 0) continue;                     // (free text inside a line)
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            obj += (first ? "" : ", ") + quote(k) + ": " + (is_number(v) ? v : quote(v));
            first = false;
        }
        obj += "}";
        size_t i = 0;
        while (i < sections.size() && sections[i].first != name) ++i;
        if (i == sections.size()) sections.push_back({name, {}});
        sections[i].second.push_back(obj);
    }
    std::string js = "{";
    for (size_t i = 0; i < sections.size(); i++) {
        js += (i ? ", " : "") + quote(sections[i].first) + ": ";
        if (sections[i].second.size() == 1) js += sections[i].second[0];
        else {
            js += "[";
            for (size_t j = 0; j < sections[i].second.size(); j++) js += (j ? ", " : "") + sections[i].second[j];
            js += "]";
        }
    }
    js += "}\n";
    if (path == "-") return fputs(js.c_str(), stderr) >= 0;
    FILE *f = fopen(path.c_str(), "wb");
    return f && fwrite(js.data(), 1, js.size(), f) == js.size() && fclose(f) == 0;
}

// the reference's startup self-test (TestAll, classify.cpp:341-367) on our host primitives
bool self_test() {
    size_t s, n;
    const char *h = "VSDSDS#XXX_xxx_s/1";
    hast_parse_barcode(h, strlen(h), &s, &n);
    if (std::string(h + s, n) != "XXX_xxx_s") return false;
    if (hast_canon_kmer("AGCTC", 5) != 0xD9 || hast_canon_kmer("GAGCT", 5) != 0xD9) return false;
    uint64_t km[2];
    if (hast_chop_read("GAGCTA", 6, 5, km) != 2 || km[0] != 0xD9 || km[1] != 0xD8) return false;
    char buf[8];
    hast_kmer_to_str(km[0], 5, buf);
    if (strcmp(buf, "AGCTC")) return false;
    hast_kmer_to_str(km[1], 5, buf);
    return strcmp(buf, "AGCTA") == 0;
}

struct Counts {                                    // host accumulators behind the device counters
    std::vector<uint64_t> c0, c1, neg;             // by device-dictionary id (one dictionary), by merged id (several), by host id (no device dictionary)
    std::vector<uint64_t> h0, h1, hneg;            // by host-dictionary id, for what a device dictionary left to the host
    size_t device_cap = 0;
    bool folded = false;                           // device counters have been read back and added to the sums above
};

// Who numbers the barcodes.  Round 6: the GPU's own dictionary (hast_names_create_dict) -- ids 0 .. limit-1 in the order in which its
// naming kernel meets new texts; the host's dictionary only names what the device leaves to it (texts longer than 15 bytes, and what
// arrives when every device id is out) in the range [host_base, ...) above.  One dictionary per GPU (contexts of one GPU share it): with
// several GPUs the dictionaries number independently and their counters are MERGED BY TEXT, on the GPUs: the texts another dictionary has
// learnt go through the FIRST dictionary's naming kernel (hast_names_merge: their ids there, new ones claimed), the counters of that
// dictionary's contexts are renumbered on their device (hast_counts_permute), then the one all-reduce runs over one id space.
struct Naming {
    bool device_dict = false;
    size_t host_base = 0;                          // ids of the host dictionary start here in the device counters
    std::vector<hast_names *> groups;              // the distinct dictionaries
    std::vector<int> group_of;                     // per context
    std::vector<std::vector<uint32_t>> perm;       // per dictionary but the first: its ids in the first one's numbering, as far as merged
    double merge_s = 0;
    size_t merged_to_host = 0;                     // texts of another dictionary that the first one had no id left for
};

inline void add_into(std::vector<uint64_t> &dst, const std::vector<uint64_t> &src, size_t n) {
    if (dst.size() < n) dst.resize(n);
    for (size_t i = 0; i < n; i++) dst[i] += src[i];       // (64-bit on the device and here: nothing wraps)
}

// What the command line asked for (and the environment variables that the flags replace).
struct Options {
    std::string hap0, hap1, save_table, load_table, stats_json, route_mode;
    std::string r1{"CTGTCTCTTATACACATCTTAGGAAGACAAGCACTGACGACATGA"};   // classify.cpp:312
    std::string r2{"TCTGCTGAGTCGAGAACGTCTCTGTGAGCCAAGGAGTTGCTCTGG"};   // classify.cpp:313
    std::vector<std::string> read;
    int t_num = 8;
    std::vector<int> devices;                      // the first one builds the table
    // (counters for 16M barcodes from the start: 512 MB of HBM and a fill -- a regrowth reads everything back and allocates anew, four
    // times on the way to BASELINE config 3's 10M barcodes)
    size_t batch_reads = 0, block_mb = 256, initial_barcodes = 1u << 24;
    bool stats = false, host_parse = false, phase_reads = false, gz_out = false;
    bool gz_bgzf = false;                          // --gz-format bgzf: what --gz-out writes is blocked gzip (BGZF) with an end-of-file block per file
    hast::quartering::GzFormat gz_format() const {
        return !gz_out ? hast::quartering::GzFormat::kNone : gz_bgzf ? hast::quartering::GzFormat::kBgzf : hast::quartering::GzFormat::kGzip;
    }
    bool rows_device = false;                      // --rows device: the table (and the lists) are sorted and formatted on the GPU (hast_rows_*)
    bool bgzf_device = false;                      // --bgzf device: blocked gzip is inflated on the GPU per member (hast_gz_open_blocked)
    double w0 = 1.0, w1 = 1.0;
    // worked out from the above
    size_t block_bytes = 0;                        // --host-parse: bytes per block of a file
    bool block_given = false;                      // --block-mb or --batch-reads said how large a block is
    // GPU framing: bytes per block of a file, blocks a file may have between its reader and the commit
    // (a multiple of 4 KB, as the library's blocks are: the blocks of a striped stream must be full)
    size_t fq_cap = 0;
    static constexpr int fq_bufs = 6;
};

// What a run holds from one phase of main() to the next.
struct Run {
    explicit Run(const Options &opt) : o(opt), dev_gz(opt.read.size(), 0), dev_bz(opt.read.size(), 0) {}
    const Options &o;
    size_t K = 0;
    hast_ctx *ctx = nullptr;                       // the first GPU's: the table is built there
    std::vector<hast_ctx *> ctxs;
    // several GPUs: the blocks of every file go to all of them in turn (a striped stream); HAST_DEAL=files deals whole files
    bool stripe = false;
    std::vector<char> dev_gz;                      // per input: inflated on the GPU
    std::vector<char> dev_bz;                      // ... as blocked gzip, member by member (--bgzf device; only with dev_gz)
    // the FASTQ streams (and .gz inputs) of the first files, opened by the set-up thread while the table is built
    std::vector<hast_fq *> pre_fq, done_fq;
    std::vector<hast_gz *> pre_gz;
    std::vector<hast_status> pre_gz_status;
    std::thread pre_thread;
    std::string pre_error;
    std::vector<std::thread> gz_closers;
    std::vector<hast_names *> name_caches, own_caches;     // per context / per GPU: device-side dictionary barcode text -> id
    std::vector<hast_names *> own_tabs;                    // per GPU: the routing pass's table barcode text -> class
    Naming naming;
    std::atomic<bool> hbm_stop{false};
    std::atomic<size_t> hbm_free_min{~(size_t)0}, hbm_total{0};
    std::thread hbm_thread;
    // reader thread -> blocks of raw bytes -> t_num workers index newlines / name barcodes in parallel
    std::unique_ptr<hast::WorkerPool> pool;                // (from the read phase on)
    hast::BarcodeDict dict;
    std::vector<hast::BarcodeDict::Cache> caches;
    Counts acc;
    uint64_t total_reads = 0, total_bases = 0, n_set[2] = {0, 0};
    // the rows: names by id (the device dictionary's, then the host's), and their sorted order
    std::vector<uint8_t> dev_texts;
    std::vector<std::string_view> names;
    std::vector<uint32_t> order;
    size_t n_dev_names = 0, n_host_names = 0, n_rows_summed = 0;
    size_t n_rows = 0;                             // rows of the table
    bool past_int = false;
    // --rows device: the table made on the GPU (null: made on the host, rows_fallback says why when the device was asked for)
    hast_rows *rows = nullptr;
    bool counts_summed = false;                    // the all-reduce has run and nothing was counted since
    const char *rows_fallback = "none";
    double rows_download_write_s = 0;
    double t_start = 0, t_ctx = 0, t_loaded = 0, t_scrubbed = 0, t_read_done = 0, t_classified = 0, t_printed = 0, t_pre_waited = 0;
};

// The counters of all contexts summed ON the devices, nothing read back: the dictionaries of several GPUs merged into the first one's
// numbering and their contexts' counters renumbered, then ONE all-reduce(sum,u64) over RCCL/xGMI, which leaves the totals on every
// device (collectBarcodes + data.Add, classify.cpp:226-229,277).  flush_counts reads them back behind it; --rows device goes on from
// them where they lie.
void sum_counts_on_devices(Run &rs) {
    std::vector<hast_ctx *> &ctxs = rs.ctxs;
    Counts &acc = rs.acc;
    Naming &nm = rs.naming;
    hast::BarcodeDict &dict = rs.dict;
    hast::BarcodeDict::Cache &dict_cache = rs.caches[0];
    {
        if (nm.device_dict && nm.groups.size() > 1) {
            // several dictionaries: what each has learnt since the last merge into the first one's numbering, its contexts' counters with it
            const double t0 = now_s();
            nm.perm.resize(nm.groups.size());
            for (size_t g = 1; g < nm.groups.size(); g++) {
                size_t n_g = 0;
                CK(hast_names_count(nm.groups[g], &n_g), "asking a dictionary for its size");
                const size_t have = nm.perm[g].size();
                if (n_g > have) {
                    nm.perm[g].resize(n_g);
                    const hast_status ms = hast_names_merge(nm.groups[0], nm.groups[g], have, n_g - have, nm.perm[g].data() + have);
                    if (ms == HAST_ERR_TABLE_FULL) {
                        // the first dictionary is out of ids: what it could not take (HAST_NAME_NONE, include/hast.h) is the host's, like
                        // everything a full dictionary leaves to it -- the text by id from the other dictionary, its counters to the host's id
                        std::vector<uint8_t> txt(16 * (n_g - have));
                        CK(hast_names_texts(nm.groups[g], have, n_g - have, txt.data()), "reading a dictionary's texts");
                        for (size_t i = have; i < n_g; i++) {
                            if (nm.perm[g][i] != HAST_NAME_NONE) continue;
                            const uint8_t *t = txt.data() + 16 * (i - have);
                            nm.perm[g][i] = (uint32_t)nm.host_base + dict.get(std::string_view(reinterpret_cast<const char *>(t) + 1, t[0]), dict_cache);
                            nm.merged_to_host++;
                        }
                    } else if (ms != HAST_OK)
                        die(4, "merging the GPUs' barcode dictionaries");
                }
            }
            // (the first dictionary may have grown past what the counters were sized for -- they follow the ids of each dictionary's own
            // blocks: every context's counters move into arrays that hold the merged numbering)
            size_t n_merged = 0;
            CK(hast_names_count(nm.groups[0], &n_merged), "asking the dictionary for its size");
            const size_t need_cap = std::max({acc.device_cap, n_merged, dict.size() ? nm.host_base + dict.size() : 0});
            for (size_t i = 0; i < ctxs.size(); i++) {
                const size_t g = (size_t)nm.group_of[i];
                if (g == 0 && need_cap == acc.device_cap) continue;
                const size_t n_perm = g ? std::min(nm.perm[g].size(), acc.device_cap) : 0;
                CK(hast_counts_permute(ctxs[i], g ? nm.perm[g].data() : nullptr, n_perm, need_cap), "renumbering the counters of a GPU");
            }
            acc.device_cap = need_cap;
            nm.merge_s += now_s() - t0;
        }
        if (ctxs.size() > 1) CK(hast_counts_allreduce(ctxs.data(), (int)ctxs.size()), "summing the counters of the GPUs");
    }
}

void flush_counts(Run &rs, size_t new_cap) {
    std::vector<hast_ctx *> &ctxs = rs.ctxs;
    Counts &acc = rs.acc;
    Naming &nm = rs.naming;
    hast::BarcodeDict &dict = rs.dict;
    // fold what the devices have counted so far into the host sums, then (re)size the device arrays
    hast_ctx *ctx = ctxs[0];
    if (acc.device_cap) {
        std::vector<uint64_t> a, b, c;
        auto read_range = [&](size_t first, size_t n, std::vector<uint64_t> &d0, std::vector<uint64_t> &d1, std::vector<uint64_t> &d2) {
            n = first < acc.device_cap ? std::min(n, acc.device_cap - first) : 0;
            a.assign(n, 0); b.assign(n, 0); c.assign(n, 0);
            if (n) CK(hast_counts_read_range(ctx, first, n, a.data(), b.data(), c.data()), "reading counters");
            add_into(d0, a, n); add_into(d1, b, n); add_into(d2, c, n);
        };
        if (!rs.counts_summed) sum_counts_on_devices(rs);           // (--rows device summed them and then had no room for its table)
        rs.counts_summed = false;
        acc.folded = true;
        const size_t n_host = dict.size();                                         // (after the merge: it may have named texts)
        if (!nm.device_dict) read_range(0, n_host, acc.c0, acc.c1, acc.neg);      // (only the barcodes that exist: the counters are sized ahead of the dictionary)
        else {
            size_t n_dev = 0;
            CK(hast_names_count(nm.groups[0], &n_dev), "asking the dictionary for its size");
            read_range(0, n_dev, acc.c0, acc.c1, acc.neg);
            read_range(nm.host_base, n_host, acc.h0, acc.h1, acc.hneg);
        }
    }
    for (hast_ctx *c : ctxs) CK(hast_counts_resize(c, new_cap), "allocating counters");
    acc.device_cap = new_cap;
}

// a plain non-negative decimal number, fractions allowed ("1.5"), nothing behind it
bool parse_amount(const char *text, double *out) {
    if (!text || !((*text >= '0' && *text <= '9') || *text == '.')) return false;
    errno = 0;
    char *end = nullptr;
    const double v = strtod(text, &end);
    if (errno || end == text || *end || !(v >= 0) || v > 1e12) return false;
    *out = v;
    return true;
}

// What changes what a production run allocates or writes is a FLAG; the environment variable each one replaces stays as an alias
// (a flag wins).  The library reads its switches from the environment, once: a flag is put there before the first library call.
// false: the usage text has been printed, the exit status is -1
bool parse_options(int argc, char **argv, Options &o) {
    static struct option long_options[] = {                       // classify.cpp:375-386 + additive
        {"hap0", required_argument, NULL, 'p'},      {"hap1", required_argument, NULL, 'm'},
        {"read", required_argument, NULL, 'r'},      {"thread", required_argument, NULL, 't'},
        {"weight0", required_argument, NULL, 'w'},   {"weight1", required_argument, NULL, 'u'},
        {"adaptor_f", required_argument, NULL, 'f'}, {"adaptor_r", required_argument, NULL, 'q'},
        {"help", no_argument, NULL, 'h'},            {"device", required_argument, NULL, 1001},
        {"batch-reads", required_argument, NULL, 1002}, {"stats", no_argument, NULL, 1003},
        {"block-mb", required_argument, NULL, 1004},    {"initial-barcodes", required_argument, NULL, 1005},
        {"save-table", required_argument, NULL, 1006},  {"load-table", required_argument, NULL, 1007},
        {"devices", required_argument, NULL, 1008},     {"host-parse", no_argument, NULL, 1009},
        {"phase-reads", no_argument, NULL, 1010},       {"inflate", required_argument, NULL, 1011},
        {"gz-ring-bytes", required_argument, NULL, 1012}, {"stats-json", required_argument, NULL, 1013},
        {"park-gb", required_argument, NULL, 1014},     {"name-cache", required_argument, NULL, 1015},
        {"deal", required_argument, NULL, 1016},        {"route", required_argument, NULL, 1017},
        {"gz-out", no_argument, NULL, 1018},            {"bgzf", required_argument, NULL, 1019},
        {"gz-format", required_argument, NULL, 1020},   {"rows", required_argument, NULL, 1021},
        {0, 0, 0, 0}};
    static char optstring[] = "p:m:l:r:t:w:u:f:q:h";             // classify.cpp:387
    bool gz_out_flag = false;
    int device = 0;
    // (the aliases for runs of the unchanged wrapper; a flag wins.  These three are held to the rule of their flag below: a wrong word
    // is the usage text, not a variable that is ignored)
    const char *bgzf = sw::text(sw::HAST_BGZF);
    const char *gz_format = sw::text(sw::HAST_PHASE_GZ_FORMAT);   // (ignored where nothing is written as gzip)
    const char *rows = sw::text(sw::HAST_ROWS);
    bool gz_format_flag = false;
    o.phase_reads = sw::flag(sw::HAST_PHASE_READS);
    o.gz_out = sw::flag(sw::HAST_PHASE_GZ);
    for (;;) {
        int c = getopt_long(argc, argv, optstring, long_options, NULL);
        if (c < 0) break;
        switch (c) {
        case 'f': o.r1 = optarg; break;
        case 'q': o.r2 = optarg; break;
        case 'p': o.hap0 = optarg; break;
        case 'm': o.hap1 = optarg; break;
        case 'r': o.read.push_back(optarg); break;
        case 't': o.t_num = atoi(optarg); break;
        case 'u': o.w1 = atof(optarg); break;
        case 'w': o.w0 = atof(optarg); break;
        case 1001: device = atoi(optarg); break;
        case 1002: o.batch_reads = (size_t)std::max(1L, atol(optarg)); break;
        case 1003: o.stats = true; break;
        case 1004: o.block_mb = (size_t)std::max(1L, atol(optarg)); break;
        case 1005: o.initial_barcodes = (size_t)std::max(1L, atol(optarg)); break;
        case 1006: o.save_table = optarg; break;
        case 1007: o.load_table = optarg; break;
        case 1009: o.host_parse = true; break;
        case 1010: o.phase_reads = true; break;
        case 1011:
            if (strcmp(optarg, "host") && strcmp(optarg, "device") && strcmp(optarg, "zlib")) { print_usage(); return false; }
            setenv("HAST_INFLATE", optarg, 1);
            break;
        case 1012: {                                     // (the library reads plain decimal digits from the environment: what a suffix meant is spelt out)
            uint64_t v;
            if (!parse_count(optarg, &v)) { print_usage(); return false; }
            setenv("HAST_GZ_RING_BYTES", std::to_string(v).c_str(), 1);
            break;
        }
        case 1013: o.stats_json = optarg; o.stats = true; break;
        case 1014: {
            double v;
            if (!parse_amount(optarg, &v)) { print_usage(); return false; }
            setenv("HAST_PARK_GB", optarg, 1);
            break;
        }
        case 1015: {
            uint64_t v;
            if (!parse_count(optarg, &v)) { print_usage(); return false; }
            setenv("HAST_NAME_CACHE", std::to_string(v).c_str(), 1);
            break;
        }
        case 1016:
            if (strcmp(optarg, "files") && strcmp(optarg, "blocks")) { print_usage(); return false; }
            setenv("HAST_DEAL", optarg, 1);
            break;
        case 1017:
            if (strcmp(optarg, "host") && strcmp(optarg, "device")) { print_usage(); return false; }
            o.route_mode = optarg;
            break;
        case 1018: o.gz_out = gz_out_flag = true; break;
        case 1019: bgzf = optarg; break;
        case 1020: gz_format = optarg; gz_format_flag = true; break;
        case 1021: rows = optarg; break;
        case 1008:
            if (!hast::parse_device_list(optarg, o.devices)) { print_usage(); return false; }
            break;
        case 'h':
        default: print_usage(); return false;
        }
    }
    if (((o.hap0.empty() || o.hap1.empty()) && o.load_table.empty()) || o.read.empty() || o.t_num < 1) {   // classify.cpp:425-428
        print_usage();
        return false;
    }
    // --gz-out says how the routed files are written: without --phase-reads there are none (HAST_PHASE_GZ alone is ignored: a wrapper
    // may export it for every stage)
    if (gz_out_flag && !o.phase_reads) {
        fputs("classify: --gz-out needs --phase-reads\n", stderr);
        print_usage();
        return false;
    }
    o.gz_out = o.gz_out && o.phase_reads;
    // --gz-format says how --gz-out writes: without it there is nothing to say (the variable alone is ignored then, as HAST_PHASE_GZ is)
    if (gz_format_flag && !o.gz_out) {
        fputs("classify: --gz-format needs --gz-out\n", stderr);
        print_usage();
        return false;
    }
    if (o.gz_out && gz_format && *gz_format) {
        if (strcmp(gz_format, "gzip") && strcmp(gz_format, "bgzf")) { print_usage(); return false; }
        o.gz_bgzf = !strcmp(gz_format, "bgzf");
    }
    if (bgzf && *bgzf) {
        if (strcmp(bgzf, "host") && strcmp(bgzf, "device")) { print_usage(); return false; }
        o.bgzf_device = !strcmp(bgzf, "device");
    }
    if (rows && *rows) {
        if (strcmp(rows, "host") && strcmp(rows, "device")) { print_usage(); return false; }
        o.rows_device = !strcmp(rows, "device");
    }
    if (o.devices.empty()) o.devices.push_back(device);
    // --batch-reads N (tests / small inputs): shrink the blocks so that a batch holds about N records
    o.block_bytes = o.block_mb << 20;
    if (o.batch_reads) o.block_bytes = std::max<size_t>(4096, std::min(o.block_bytes, o.batch_reads * 320));
    o.block_given = o.block_mb != 256 || o.batch_reads;
    o.fq_cap = (std::max<size_t>(4096, o.block_given ? std::min<size_t>(o.block_bytes, 256u << 20) : (16u << 20)) + 4095) & ~(size_t)4095;
    return true;
}

// ---- the inputs and their streams ---------------------------------------------------------------------------------------------
// the file name of an input without its directories and without a trailing ".gz" (the wrapper's ${name: -3} == ".gz"), and whether
// that was there
struct InputName {
    std::string base;
    bool gz = false;
};
InputName input_name(const std::string &path) {
    InputName n;
    n.base = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
    n.gz = hast::ends_gz(n.base, 0);
    if (n.gz) n.base.resize(n.base.size() - 3);
    return n;
}

// buffers of a FASTQ stream per context
int buffers_per_context(const Run &rs) {
    const int n_ctx = (int)rs.ctxs.size();
    return rs.stripe ? std::max(2, (Options::fq_bufs + n_ctx - 1) / n_ctx) : Options::fq_bufs;
}

// inputs open at a time.  same_prefix: inputs with one basename write the same four routed files -- the awk loop lets the later one
// overwrite the earlier: one at a time then
size_t inputs_open_at_once(const Run &rs, bool same_prefix) {
    return same_prefix ? 1 : rs.stripe ? 2 : std::max<size_t>(4, 2 * rs.ctxs.size());
}

// .gz inputs are inflated ON THE GPU (hast_gz_*: the compressed bytes cross PCIe, the framer reads the inflated bytes where they
// lie) when they are ordinary gzip files; blocked gzip (BGZF: thousands of one-block members, which the host inflates side by
// side), pipes and ".gz" files that are not gzip stay with the host decoders, as does everything under HAST_INFLATE=host|zlib.
// --bgzf device: a blocked-gzip input goes to the GPU too, inflated member by member (hast_gz_open_blocked) -- with one context or
// whole files dealt to the contexts; a striped run keeps it on the host.
void find_device_gz_inputs(Run &rs) {
    const int which = sw::word(sw::HAST_INFLATE);                 // (device 0, host 1, zlib 2; unset -1)
    const bool allow = !rs.o.host_parse && which <= 0;
    const bool blocked_ok = rs.o.bgzf_device && (rs.o.devices.size() <= 1 || sw::word_is(sw::HAST_DEAL, "files"));
    for (size_t i = 0; allow && i < rs.o.read.size(); i++) {
        const std::string &r = rs.o.read[i];
        struct stat sb;
        // (a file called just ".gz" is no gzip file to BlockSource either)
        if (r.size() <= 3 || !input_name(r).gz || stat(r.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) continue;
        FILE *fp = fopen(r.c_str(), "rb");
        if (!fp) continue;                                      // (reported where the file is opened for good)
        unsigned char magic[2] = {0, 0};
        const bool gzip_magic = fread(magic, 1, 2, fp) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        rewind(fp);
        const bool blocked = hast::BgzfReader::probe(fp);
        rs.dev_bz[i] = gzip_magic && blocked && blocked_ok;
        rs.dev_gz[i] = ((gzip_magic || sb.st_size == 0) && !blocked) || rs.dev_bz[i];
        fclose(fp);
    }
}

// Bytes per block of an input.  A block costs a dozen small kernels and two host round trips besides its bytes.  For a .gz input
// inflated on the GPU that is what bounds the read phase at BASELINE size (2 x 34 GB = 4 090 blocks of 16 MB): 64-MB blocks 1.70-1.82 s
// against 2.23-2.26 s, alternating on one box (profiles/round6_cli_c2_ab_blocks.txt) -- and such a stream has no block to pin on
// the host.  Plain files stay at 16 MB: their read phase is the PCIe upload whatever the block (1.43-1.48 s with 32 MB against
// 1.34-1.50 s), their blocks are pinned host memory (0.7 ms per MB, six buffers a stream), and small .gz inputs want their first
// block early.
size_t cap_of(const Run &rs, size_t file_index) {
    const Options &o = rs.o;
    if (o.block_given || o.host_parse || !rs.dev_gz[file_index]) return o.fq_cap;
    struct stat sb;
    if (stat(o.read[file_index].c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return o.fq_cap;
    return (uint64_t)sb.st_size >= (1ull << 30) ? (size_t)(64u << 20) : o.fq_cap;
}

hast_status make_fq(Run &rs, size_t file_index, hast_fq **out) {
    const size_t cap = cap_of(rs, file_index);
    const int device_blocks = rs.dev_gz[file_index] ? 1 : 0;
    // (a .gz file inflated on the GPUs: the passes of its one deflate stream go to the GPUs in turn, hast_gz_open_multi, and its
    // inflated blocks -- written on the device -- are dealt to the contexts like a plain file's)
    if (rs.stripe) return hast_fq_create_striped_ex(rs.ctxs.data(), (int)rs.ctxs.size(), cap, buffers_per_context(rs), rs.name_caches.data(), device_blocks, out);
    const size_t c = file_index % rs.ctxs.size();
    return hast_fq_create_ex(rs.ctxs[c], cap, buffers_per_context(rs), rs.name_caches[c], device_blocks, out);
}

// a .gz input on the device(s): its compressed bytes go there and its first passes are decoded at once
hast_status open_gz(Run &rs, size_t file_index, hast_gz **out) {
    const char *path = rs.o.read[file_index].c_str();
    if (rs.dev_bz[file_index]) return hast_gz_open_blocked(rs.ctxs[file_index % rs.ctxs.size()], path, out);
    return rs.stripe ? hast_gz_open_multi(rs.ctxs.data(), (int)rs.ctxs.size(), path, out) : hast_gz_open(rs.ctxs[file_index % rs.ctxs.size()], path, out);
}

// --stats: the device's free memory, sampled every 20 ms from here to the end (the HBM head-room line)
void start_hbm_sampler(Run &rs) {
    rs.hbm_thread = std::thread([&rs] {
        while (!rs.hbm_stop.load()) {
            size_t f = 0, t = 0;
            if (hast_dev_mem_info(rs.ctx, &f, &t, nullptr) == HAST_OK) {
                rs.hbm_total = t;
                if (f < rs.hbm_free_min.load()) rs.hbm_free_min = f;
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
        }
    });
}

// the first context exists: the other GPUs' at the same time (a context is a device's first HIP calls and a few streams, 50-100 ms each)
void create_other_contexts(Run &rs) {
    const std::vector<int> &devices = rs.o.devices;
    rs.ctxs.push_back(rs.ctx);
    std::vector<hast_ctx *> made(devices.size(), nullptr);
    std::vector<std::thread> makers;
    for (size_t i = 1; i < devices.size(); i++)
        makers.emplace_back([&, i] {
            if (hast_ctx_create(devices[i], (int)rs.K, &made[i]) != HAST_OK) made[i] = nullptr;
        });
    for (std::thread &t : makers) t.join();
    for (size_t i = 1; i < devices.size(); i++) {
        if (!made[i]) die(4, "cannot create GPU context");
        rs.ctxs.push_back(made[i]);
    }
}

// a dictionary barcode text -> id per GPU (contexts of one GPU share it)
void create_dictionaries(Run &rs) {
    const Options &o = rs.o;
    // (2 x 32 B per barcode it can hold + 16 B of text by id: 1.3 GB for 16M -- BASELINE config 3 has 10M barcodes; what does not fit
    // is named by the host, in an id range of its own)
    size_t name_cap = std::max<size_t>(o.initial_barcodes, 1u << 24);
    sw::size(sw::HAST_NAME_CACHE, &name_cap);
    // HAST_NAME_DICT=0: the table only caches what the host's dictionary names (up to round 5); HAST_NAME_DICT=context: a dictionary
    // per CONTEXT even where contexts share a GPU (tests: the merge by text of several GPUs' dictionaries, on one GPU)
    rs.naming.device_dict = name_cap && !sw::word_is(sw::HAST_NAME_DICT, "0");
    const bool per_context = sw::word_is(sw::HAST_NAME_DICT, "context");
    for (size_t i = 0; i < rs.ctxs.size(); i++) {
        // one per GPU: contexts that share a device (--devices 0,0) share it
        hast_names *nm = nullptr;
        int group = -1;
        for (size_t j = 0; j < i && !nm && !per_context; j++)
            if (o.devices[j] == o.devices[i]) { nm = rs.name_caches[j]; group = rs.naming.group_of[j]; }
        if (!nm && name_cap) {
            CK(rs.naming.device_dict ? hast_names_create_dict(rs.ctxs[i], name_cap, &nm) : hast_names_create(rs.ctxs[i], name_cap, &nm), "creating the barcode dictionary");
            rs.own_caches.push_back(nm);
            group = (int)rs.naming.groups.size();
            rs.naming.groups.push_back(nm);
        }
        rs.name_caches.push_back(nm);
        rs.naming.group_of.push_back(group);
    }
    if (rs.naming.device_dict) rs.naming.host_base = hast_names_limit(rs.naming.groups[0]);
}

// The first .gz files are opened NOW: their compressed bytes go to the device and their first passes are decoded while the
// k-mer files are loaded and the table is built (an inflated stream needs a GPU, not the table; the symbols wait in the
// stream's arenas) -- ~0.1 s of decode that used to start when the read phase did.  A thread per input: opening a stream and
// creating its FASTQ framer is mostly page pinning and device allocation, which the inputs need not queue up for.
void start_stream_setup(Run &rs) {
    rs.pre_fq.assign(std::min<size_t>(rs.o.read.size(), inputs_open_at_once(rs, false)), nullptr);
    rs.pre_gz.assign(rs.pre_fq.size(), nullptr);
    rs.pre_gz_status.assign(rs.pre_fq.size(), HAST_OK);
    rs.pre_thread = std::thread([&rs] {
        std::mutex err_mu;
        std::vector<std::thread> per_file;
        for (size_t i = 0; i < rs.pre_fq.size(); i++)
            per_file.emplace_back([&, i] {
                if (rs.dev_gz[i]) rs.pre_gz_status[i] = open_gz(rs, i, &rs.pre_gz[i]);        // (looked at where the read phase opens the input)
                if (make_fq(rs, i, &rs.pre_fq[i]) != HAST_OK) {
                    std::lock_guard<std::mutex> g(err_mu);
                    rs.pre_error = hast_last_error();
                }
            });
        for (std::thread &t : per_file) t.join();
    });
}

// The FASTQ streams of the first files (pinned staging + device buffers: ~0.1 s of page pinning) are set up by a thread
// of their own while the main thread reads the k-mer files and builds the table.
void contexts_ready(Run &rs) {
    if (rs.o.stats) start_hbm_sampler(rs);
    create_other_contexts(rs);
    if (rs.o.host_parse) return;
    // several GPUs: the blocks of every file go to all of them in turn (a striped stream); HAST_DEAL=files deals whole files
    rs.stripe = rs.ctxs.size() > 1 && !sw::word_is(sw::HAST_DEAL, "files");
    create_dictionaries(rs);
    start_stream_setup(rs);
}

// ---- load_kmers (classify.cpp:30-46): both files to memory, table built on the GPU --------
// binary key-set cache written by --save-table (both sets, after the adaptor scrub of that run)
void load_saved_table(Run &rs) {
    const Options &o = rs.o;
    int kk = 0;
    if (hast_table_file_info(o.load_table.c_str(), &kk, nullptr) != HAST_OK) die(2, "cannot use --load-table file");
    rs.K = (size_t)kk;
    if (hast_ctx_create(o.devices[0], kk, &rs.ctx) != HAST_OK) die(4, "cannot create GPU context");
    rs.t_ctx = now_s();
    contexts_ready(rs);
    fprintf(stderr, "__load kmer table %s__\n", o.load_table.c_str());
    CK(hast_table_load(rs.ctx, o.load_table.c_str(), 0.0), "loading the k-mer table");
    rs.t_loaded = now_s();
}

// returns 0, or the exit status of a K the reference does not have either
int build_table(Run &rs) {
    const Options &o = rs.o;
    // K = length of the first line of hap0 (classify.cpp:35-36); hast::KmerFiles has the rest
    hast::KmerFiles kf;
    std::string msg;
    if (int code = kf.open(o.hap0, o.hap1, &msg)) die(code, msg.c_str());
    rs.K = kf.K;
    if (rs.K < 1 || rs.K > 32) {
        fprintf(stderr, "classify: ERROR: K=%zu%s (length of the first line of %s) is outside [1,32]\n", rs.K, (!kf.head_has_newline && kf.head.size() == 4096) ? " or more" : "", o.hap0.c_str());
        return 3;
    }
    if (hast_ctx_create(o.devices[0], (int)rs.K, &rs.ctx) != HAST_OK) die(4, "cannot create GPU context");
    rs.t_ctx = now_s();
    contexts_ready(rs);
    CK(hast_table_reserve(rs.ctx, kf.capacity(), 0.0), "allocating the k-mer table");
    for (int h = 0; h < 2; h++) {
        fprintf(stderr, "__load hap%d kmers__\n", h);
        uint64_t lines = 0;
        if (int code = kf.insert(rs.ctx, h, false, false, &lines, &msg)) die(code, msg.empty() ? "k-mer file is not one K-mer per line" : msg.c_str());
        fprintf(stderr, "Recorded %llu haplotype %d specific %zu-mers\n", (unsigned long long)lines, h, rs.K);   // :45
    }
    rs.t_loaded = now_s();
    return 0;
}

// ---- InitAdaptor (classify.cpp:314-339), set sizes, --save-table, the other GPUs' copies ------
void scrub_and_clone(Run &rs) {
    const Options &o = rs.o;
    fprintf(stderr, "Adaptor forward :%s\n", o.r1.c_str());
    fprintf(stderr, "Adaptor reverse :%s\n", o.r2.c_str());
    {
        std::vector<uint64_t> keys;
        for (const std::string *ad : {&o.r1, &o.r2}) {
            if (ad->size() < rs.K) {
                fprintf(stderr, " WARN : adaptor shorter than K ignored\n");
                continue;
            }
            std::vector<uint64_t> km(ad->size() - rs.K + 1);
            size_t n = hast_chop_read(ad->data(), ad->size(), (int)rs.K, km.data());
            for (size_t i = 0; i < n; i++)
                if (std::find(keys.begin(), keys.end(), km[i]) == keys.end()) keys.push_back(km[i]);   // a repeat finds nothing the 2nd time
        }
        std::vector<uint8_t> hit(keys.size());
        CK(hast_table_erase(rs.ctx, keys.data(), keys.size(), hit.data()), "adaptor scrub");
        char buf[40];
        for (size_t i = 0; i < keys.size(); i++)
            for (int h = 0; h < 2; h++)
                if (hit[i] & (1 << h)) {
                    hast_kmer_to_str(keys[i], (int)rs.K, buf);
                    fprintf(stderr, " INFO : erase a adaptor kmer from hap %d ; kmer= %s\n", h, buf);   // :321,325
                }
    }
    CK(hast_table_sizes(rs.ctx, &rs.n_set[0], &rs.n_set[1]), "counting set sizes");
    if (!o.save_table.empty()) CK(hast_table_save(rs.ctx, o.save_table.c_str()), "writing --save-table file");
    // the other GPUs get a copy of the finished table (after the adaptor scrub), peer to peer
    // (all at once: every GPU pulls its copy over its own xGMI link from the first one -- one after the other, seven copies of the 50 GB
    // of BASELINE config 3's table and filter are seven times the one copy's time.  The source's filter is built first, once: the clones
    // only read the source then.)
    if (rs.ctxs.size() > 1) {
        CK(hast_filter_build(rs.ctx), "building the k-mer filter");
        std::vector<std::thread> cloners;
        std::vector<std::string> clone_err(rs.ctxs.size());
        for (size_t i = 1; i < rs.ctxs.size(); i++)
            cloners.emplace_back([&, i] {
                if (hast_table_clone(rs.ctxs[i], rs.ctx) != HAST_OK) clone_err[i] = std::string("copying the k-mer table to another GPU (") + hast_last_error() + ")";
            });
        for (std::thread &t : cloners) t.join();
        for (const std::string &e : clone_err)
            if (!e.empty()) {
                fprintf(stderr, "classify: ERROR: %s\n", e.c_str());
                fflush(stderr);
                _exit(4);
            }
    }
}

void wait_for_stream_setup(Run &rs) {
    const double t_pre_wait0 = now_s();
    if (rs.pre_thread.joinable()) {
        rs.pre_thread.join();
        if (!rs.pre_error.empty()) {
            fprintf(stderr, "classify: ERROR: creating the FASTQ stream (%s)\n", rs.pre_error.c_str());
            fflush(stderr);
            _exit(4);                                          // (threads of this program and of the library are at work: no destructors)
        }
    }
    rs.t_pre_waited = now_s() - t_pre_wait0;
}

// ---- processFastq (classify.cpp:238-278) for each --read, in order ------------------------
// --host-parse: reader thread -> blocks of raw bytes -> t_num workers index newlines and parse records in parallel
// -> pinned staging of the GPU library -> classify (asynchronous, double-buffered)
// Several --read files are streamed CONCURRENTLY (each has its own reader thread, so .gz files inflate in
// parallel -- zlib is the serial bottleneck of real inputs) and their blocks are parsed round-robin.  Counts are
// sums, so the interleaving cannot change the output; the reference handles the files one after the other.
struct FileState {
    std::string name;
    std::unique_ptr<hast::BlockSource> src;
    hast::BlockWork work;                          // (carries the bytes of an incomplete record at the end of a block)
};

struct HostParser {
    explicit HostParser(Run &run) : rs(run), T(run.pool->size()), part_bytes((size_t)T + 1), part_max((size_t)T), part_err((size_t)T) {}
    Run &rs;
    const int T;
    std::vector<uint64_t> part_bytes;
    std::vector<uint32_t> part_max, part_err;
    const std::string *cur_name = nullptr;
    size_t next_ctx = 0;

    // parse `n_rec` complete records whose newline positions are in allnl (4 per record) from `data`
    void parse_records(const char *data, const std::vector<uint32_t> &allnl, size_t n_rec) {
        if (n_rec == 0) return;
        uint8_t *hb;
        uint64_t *ho;
        uint32_t *hi;
        const size_t span = (size_t)allnl[4 * n_rec - 1] + 1;
        hast_ctx *bctx = rs.ctxs[next_ctx++ % rs.ctxs.size()];                               // batches are dealt round-robin to the GPUs
        CK(hast_batch_begin(bctx, span, n_rec, &hb, &ho, &hi), "staging a batch");
        auto rec_range = [&](int t, size_t &lo, size_t &hi_) { lo = n_rec * (size_t)t / T; hi_ = n_rec * (size_t)(t + 1) / T; };
        rs.pool->run([&](int t) {                          // pass 1: bytes of bases per worker
            size_t lo, hi_;
            rec_range(t, lo, hi_);
            uint64_t sum = 0;
            uint32_t mx = 0;
            for (size_t i = lo; i < hi_; i++) {
                uint32_t len = allnl[4 * i + 1] - allnl[4 * i] - 1;
                sum += len;
                mx = std::max(mx, len);
            }
            part_bytes[t + 1] = sum;
            part_max[t] = mx;
        });
        part_bytes[0] = 0;
        for (int t = 0; t < T; t++) part_bytes[t + 1] += part_bytes[t];
        rs.pool->run([&](int t) {                          // pass 2: barcode ids + bases into pinned staging
            size_t lo, hi_;
            rec_range(t, lo, hi_);
            uint64_t off = part_bytes[t];
            uint32_t err = 0;
            for (size_t i = lo; i < hi_; i++) {
                const size_t h0 = i ? (size_t)allnl[4 * i - 1] + 1 : 0, h1 = allnl[4 * i], s1 = allnl[4 * i + 1];
                size_t bs, bn;
                hast_parse_barcode(data + h0, h1 - h0, &bs, &bn);                          // classify.cpp:189
                hi[i] = rs.dict.get(std::string_view(data + h0 + bs, bn), rs.caches[t]);
                const size_t len = s1 - h1 - 1;
                ho[i] = off;
                memcpy(hb + off, data + h1 + 1, len);
                if (len < rs.K && !memchr(data + h1 + 1, 'N', len)) err = 1;                  // kmer.h:171
                off += len;
            }
            part_err[t] = err;
        });
        ho[n_rec] = part_bytes[T];
        uint32_t mx = 0;
        for (int t = 0; t < T; t++) {
            mx = std::max(mx, part_max[t]);
            if (part_err[t]) {
                fprintf(stderr, "classify: ERROR: read shorter than K=%zu in %s\n", rs.K, cur_name->c_str());
                fflush(stdout);                                                            // reference: assert abort.  _exit: the HBM sampler and the
                fflush(stderr);                                                            // library's threads are inside the HIP runtime -- exit() would take
                _exit(3);                                                                  // it down under them (seen: SIGSEGV instead of status 3)
            }
        }
        if (rs.dict.size() > rs.acc.device_cap) flush_counts(rs, std::max(rs.dict.size() * 2, rs.acc.device_cap * 2));
        CK(hast_batch_submit(bctx, n_rec, mx), "classifying a batch");
        rs.total_reads += n_rec;
        rs.total_bases += part_bytes[T];
    }
    // one block of one file; returns false when that file is finished
    bool process_block(FileState &fs) {
        cur_name = &fs.name;
        hast::BlockSource &src = *fs.src;
        hast::BlockWork &w = fs.work;
        // work area = carry (incomplete record of the previous block) + this block's data
        if (!w.next(src)) die(2, (fs.name + ": " + src.error()).c_str());
        const char *data = w.data;
        const size_t len = w.len;
        if (len == 0) return false;
        if (len >= (1ull << 32)) die(3, "a single FASTQ record spans more than 4 GB");
        w.index(*rs.pool);
        std::vector<uint32_t> &allnl = w.nl;
        const size_t n_rec = allnl.size() / 4;
        parse_records(data, allnl, n_rec);
        const size_t consumed = n_rec ? (size_t)allnl[4 * n_rec - 1] + 1 : 0;
        if (w.last) {
            // end of input: what is left holds < 4 newlines.  Reference framing (classify.cpp:257-268): the
            // header must be newline-terminated; bases are whatever follows up to the next newline or EOF.
            const char *p = data + consumed, *e = data + len;
            const char *h_end = (const char *)memchr(p, '\n', (size_t)(e - p));
            if (h_end) {
                const char *s0 = h_end + 1;
                const char *s_end = (const char *)memchr(s0, '\n', (size_t)(e - s0));
                if (!s_end) s_end = e;
                std::string tail(p, (size_t)(h_end - p));
                tail.push_back('\n');
                tail.append(s0, (size_t)(s_end - s0));
                tail.append("\n+\n\n");
                allnl.clear();
                for (size_t i = 0; i < tail.size(); i++)
                    if (tail[i] == '\n') allnl.push_back((uint32_t)i);
                parse_records(tail.data(), allnl, 1);
            }
            return false;
        }
        w.keep(src, consumed);                                                       // the incomplete record, for the next block
        return true;
    }
};

void read_phase_host(Run &rs) {
    const Options &o = rs.o;
    HostParser hp(rs);
    const size_t max_active = 4;                   // concurrent reader threads (3 prefetched blocks each)
    std::vector<FileState> active;
    size_t next_file = 0;
    auto open_next = [&]() {
        const std::string &r = o.read[next_file++];
        fprintf(stderr, "__process read: %s\n", r.c_str());
        FileState fs;
        fs.name = r;
        fs.src.reset(new hast::BlockSource());
        if (!fs.src->open(r, o.block_bytes)) die(2, ("cannot open " + r).c_str());
        active.push_back(std::move(fs));
    };
    while (next_file < o.read.size() && active.size() < max_active) open_next();
    while (!active.empty()) {
        for (size_t i = 0; i < active.size();) {
            if (hp.process_block(active[i])) {
                ++i;
                continue;
            }
            logtime();
            fprintf(stderr, "__process read done__\n");
            active.erase(active.begin() + (long)i);
            if (next_file < o.read.size()) open_next();
        }
    }
}

// ---- raw bytes to the GPU, records framed there (hast_fq_*, fq_kernels.hip) -------------------------------------
// Per file a feed (fq_feed.h): a reader thread fills the buffers the library hands out (pread / inflate straight into them), the main
// thread submits them.  Both passes over the inputs -- this one and the routing pass of --phase-reads -- run their feeds the same way;
// what they do with a block whose framing has arrived is theirs.
// (a blocked-gzip input on the device route -- the feed's handle answers hast_gz_get_blocked_stats: the library's message has the file and
// the offset; the way round it is named here)
[[noreturn]] void feed_die(const hast::FqFeed &f, hast::FeedStatus st, const std::string &what) {
    hast_gz_blocked_stats bs;
    const bool blocked = f.gz && hast_gz_get_blocked_stats(f.gz, &bs) == HAST_OK;
    die(st == hast::FeedStatus::input_failed ? 2 : 4, (blocked ? what + " -- classify --bgzf host inflates this input on the host" : what).c_str());
}

// steps 1 and 2 of a pass's loop: hand empty buffers to the reader, submit what it has filled
bool pump(hast::FqFeed &f) {
    hast::FeedStatus st = hast::FeedStatus::ok;
    std::string what;
    const bool moved = f.pump(st, what);
    if (st != hast::FeedStatus::ok) feed_die(f, st, what);
    return moved;
}

// the bytes of an input the host reads (f.gz is set: not this one)
void open_host_source(const Run &rs, hast::FqFeed &f, size_t cap) {
    if (f.gz) return;
    if (!f.src.open(f.name, cap, false)) die(2, ("cannot open " + f.name).c_str());
    f.src.set_readers(std::max(4, std::min(16, rs.o.t_num / (int)std::min<size_t>(rs.o.read.size(), 2))));
}

void start_feed(const Run &rs, hast::FqFeed &f, hast::FeedWake &wake, size_t cap) {
    std::string what;
    const hast::FeedStatus st = f.start(wake, cap, buffers_per_context(rs), what);
    if (st != hast::FeedStatus::ok) feed_die(f, st, what);
}

// (a GPU event may be what the loop waits for; a striped stream relays the newline count in front of EVERY block through the loop:
// count kernel -> host -> framing launch, so its wait is short)
double idle_wait(const Run &rs, hast::FeedWake &wake) {
    const double t0 = now_s();
    wake.wait(rs.stripe ? 10 : 100);
    return now_s() - t0;
}

// The classification pass: this thread maps the barcode text of every record the device could not name to its id (in parallel) and
// commits.  Files go to the GPUs round-robin; a file's blocks stay on one GPU (the unfinished record at the end of a block is carried
// on the device) unless the stream is striped.
struct ReadPhase {
    hast::FeedWake wake;
    std::vector<std::unique_ptr<hast::FqFeed>> active;
    size_t next_file = 0;
    std::vector<uint64_t> whole_file_records;              // records of files dealt whole, per context
    double t_create = 0, t_gpu_wait = 0, t_names = 0, t_commit = 0, t_idle = 0;
    uint64_t total_named = 0;
};

void open_next_classified(Run &rs, ReadPhase &ph) {
    const size_t fi = ph.next_file++;
    const std::string &r = rs.o.read[fi];
    fprintf(stderr, "__process read: %s\n", r.c_str());
    std::unique_ptr<hast::FqFeed> f(new hast::FqFeed());
    f->name = r;
    f->file_index = fi;
    const bool set_up_ahead = fi < rs.pre_fq.size();       // by the set-up thread, while the table was built
    if (rs.dev_gz[fi]) {
        hast_status gs;
        if (set_up_ahead) {
            gs = rs.pre_gz_status[fi];
            f->gz = rs.pre_gz[fi];
        } else
            gs = open_gz(rs, fi, &f->gz);
        if (gs == HAST_ERR_UNSUPPORTED) {                  // e.g. no room on the device: the host inflates
            f->gz = nullptr;
            rs.dev_gz[fi] = rs.dev_bz[fi] = 0;
            if (set_up_ahead && rs.pre_fq[fi]) {           // (a stream of device-side blocks was set up for it)
                hast_fq_destroy(rs.pre_fq[fi]);
                rs.pre_fq[fi] = nullptr;
            }
        } else if (gs != HAST_OK) die(2, ("cannot open " + r).c_str());
    }
    const size_t cap = cap_of(rs, fi);                     // (after a .gz input has gone to the host decoders, if it had to)
    open_host_source(rs, *f, cap);
    const double tc0 = now_s();
    if (set_up_ahead && rs.pre_fq[fi]) f->fq = rs.pre_fq[fi];
    else CK(make_fq(rs, fi, &f->fq), "creating the FASTQ stream");
    ph.t_create += now_s() - tc0;
    start_feed(rs, *f, ph.wake, cap);
    ph.active.push_back(std::move(f));
}

// names the barcodes of the oldest submitted block of a feed and commits it
void classify_block(Run &rs, ReadPhase &ph, hast::FqFeed &f) {
    const Naming &naming = rs.naming;
    const int T = rs.pool->size();
    hast_fq_block b;
    const double t0 = now_s();
    CK(hast_fq_next(f.fq, &b), "framing a block");
    const double t1 = now_s();
    ph.t_gpu_wait += t1 - t0;
    if (b.short_read) {
        fprintf(stderr, "classify: ERROR: read shorter than K=%zu in %s\n", rs.K, f.name.c_str());
        fflush(stdout);                                                            // reference: assert abort (kmer.h:171); _exit as in --host-parse
        fflush(stderr);
        _exit(3);
    }
    const size_t n = (size_t)b.n_records;
    if (hast_fq_lanes(f.fq) <= 1 || !rs.stripe) ph.whole_file_records[f.file_index % rs.ctxs.size()] += n;
    // records the device-side name cache did not know (all of them without a cache): text -> id in the job's dictionary
    const size_t nu = b.unknown ? (size_t)b.n_unknown : n;
    if (!b.bytes) {
        // a block that was filled on the device: the host copy is fetched only when a record's barcode text did not fit the
        // framer's 16-byte copy (longer than 15 bytes), or when there are no such copies (more records than they hold)
        bool need = !b.bc_text && nu > 0;
        for (size_t j = 0; !need && b.bc_text && j < nu; j++) need = b.bc_text[16 * (b.unknown ? b.unknown[j] : j)] == 0xFF;
        if (need) CK(hast_fq_block_host_bytes(f.fq, &b.bytes), "fetching a block");
    }
    auto name_range = [&](int t, size_t lo, size_t hi_) {
        for (size_t j = lo; j < hi_; j++) {
            const size_t i = b.unknown ? b.unknown[j] : j;
            const uint8_t *txt = b.bc_text ? b.bc_text + 16 * i : nullptr;      // the framer's compact copy of the barcode text
            b.ids[i] = (uint32_t)naming.host_base +
                       (txt && txt[0] != 0xFF
                            ? rs.dict.get(std::string_view(reinterpret_cast<const char *>(txt) + 1, txt[0]), rs.caches[(size_t)t])
                            : rs.dict.get(std::string_view(reinterpret_cast<const char *>(b.bytes) + b.bc_pos[i], b.bc_len[i]), rs.caches[(size_t)t]));
        }
    };
    if (nu < 4096) name_range(0, 0, nu);
    else rs.pool->run([&](int t) { name_range(t, nu * (size_t)t / T, nu * (size_t)(t + 1) / T); });
    ph.total_named += nu;
    const double t2 = now_s();
    ph.t_names += t2 - t1;
    // the counters must hold every id of this block: the device dictionary's (below dict_ids) and the host's (from host_base on)
    {
        const size_t n_host = rs.dict.size();
        const size_t need = std::max<size_t>(naming.device_dict ? (size_t)b.dict_ids : 0, n_host ? naming.host_base + n_host : 0);
        if (need > rs.acc.device_cap) flush_counts(rs, std::max(n_host ? naming.host_base + 2 * n_host + 4096 : 2 * need, rs.acc.device_cap * 2));
    }
    CK(hast_fq_commit(f.fq), "classifying a block");
    ph.t_commit += now_s() - t2;
    if (hast::feed_trace_blocks())
        fprintf(stderr, "trace %s open wait %.3f name %.3f commit %.3f ms at %.4f (sub %zu open %zu)\n", f.short_name(), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (now_s() - t2) * 1e3, now_s(),
                f.submitted, f.opened);
    f.opened++;
    f.held--;
    rs.total_reads += n;
    rs.total_bases += b.n_bases;
}

// a file whose every block is committed: its reader, its .gz stream and its line in the log
void retire_classified(Run &rs, hast::FqFeed &f) {
    f.stop_reader();
    if (f.gz) {
        hast_gz_stats gs;
        hast_gz_blocked_stats bs;
        if (rs.o.stats && rs.dev_bz[f.file_index] && hast_gz_get_blocked_stats(f.gz, &bs) == HAST_OK && hast_gz_get_stats(f.gz, &gs) == HAST_OK)
            stat_line("__stats_bgzf__ file=%s members=%llu batches=%llu read_s=%.3f upload_s=%.3f kernels_s=%.3f compressed_bytes=%llu inflated_bytes=%llu carried=%llu open_s=%.3f producer_waited_for_reader_s=%.3f\n",
                      f.name.c_str(), (unsigned long long)bs.members, (unsigned long long)bs.batches, bs.read_s, bs.upload_s, bs.kernels_s, (unsigned long long)gs.compressed_bytes,
                      (unsigned long long)gs.out_bytes, (unsigned long long)bs.carried, gs.open_s, bs.wait_reader_s);
        else if (rs.o.stats && hast_gz_get_stats(f.gz, &gs) == HAST_OK)
            stat_line("__stats_gz__ file=%s compressed_bytes=%llu inflated_bytes=%llu chunks=%llu accepted=%llu followup_jobs=%llu followup_rounds=%llu members=%llu "
                            "open_s=%.3f decode_s=%.3f windows_crc_s=%.3f chain_walk_s=%.3f producer_waited_for_upload_s=%.3f producer_waited_for_reader_s=%.3f reader_waited_for_decode_s=%.3f ring_bytes=%llu ring_laps=%llu upload_waited_for_ring=%llu\n",
                    f.name.c_str(), (unsigned long long)gs.compressed_bytes, (unsigned long long)gs.out_bytes, (unsigned long long)gs.chunks,
                    (unsigned long long)gs.accepted, (unsigned long long)gs.followup_jobs, (unsigned long long)gs.followup_rounds, (unsigned long long)gs.members,
                    gs.open_s, gs.decode_s, gs.windows_crc_s, gs.chain_walk_s, gs.wait_upload_s, gs.wait_consumer_s, gs.wait_decode_s, (unsigned long long)gs.ring_bytes,
                    (unsigned long long)gs.ring_laps, (unsigned long long)gs.upload_waited_for_ring);
        // its device memory (the compressed file, the symbol arenas, windows) goes back now, not at the end of the run: a
        // dozen finished .gz files would otherwise crowd the table out of HBM.  On a thread of its own: freeing synchronises.
        hast_gz *z = f.gz;
        rs.gz_closers.emplace_back([z] { hast_gz_close(z); });
    }
    rs.done_fq.push_back(f.fq);                            // (freed after the output: unpinning costs as much as pinning)
    logtime();
    fprintf(stderr, "__process read done__\n");
}

void read_phase_device(Run &rs) {
    ReadPhase ph;
    ph.whole_file_records.assign(rs.ctxs.size(), 0);
    const size_t max_active = inputs_open_at_once(rs, false);
    while (ph.next_file < rs.o.read.size() && ph.active.size() < max_active) open_next_classified(rs, ph);
    while (!ph.active.empty()) {
        bool progress = false;
        // 1. hand empty buffers to the readers, 2. submit what they have filled (copy + framing run on the GPU from there on)
        for (std::unique_ptr<hast::FqFeed> &f : ph.active)
            if (pump(*f)) progress = true;
        // 3. a block whose record table has arrived: name its barcodes, commit.  One block per round, so that what the
        //    readers have filled meanwhile is submitted between two blocks (the GPU must never run out of queued copies)
        for (size_t fi = 0; fi < ph.active.size();) {
            hast::FqFeed &f = *ph.active[fi];
            if (f.block_ready()) {
                classify_block(rs, ph, f);
                progress = true;
            }
            if (f.drained()) {
                retire_classified(rs, f);
                ph.active.erase(ph.active.begin() + (long)fi);
                if (ph.next_file < rs.o.read.size()) open_next_classified(rs, ph);
                progress = true;
                continue;
            }
            ++fi;
        }
        if (!progress) ph.t_idle += idle_wait(rs, ph.wake);       // everything waits for a reader thread
    }
    if (rs.o.stats && rs.stripe) {
        std::string per;
        for (size_t g = 0; g < rs.ctxs.size(); g++) {
            uint64_t n = ph.whole_file_records[g];               // (files dealt whole: HAST_DEAL=files)
            for (hast_fq *q : rs.done_fq) n += hast_fq_lane_records(q, (int)g);
            per += (g ? "," : "") + std::to_string(n);
        }
        stat_line("__stats_devices__ blocks_of_every_file_dealt_to=%zu records_per_context=%s\n", rs.ctxs.size(), per.c_str());
    }
    if (rs.o.stats)
        stat_line("__stats_read_phase__ waiting_for_file_bytes_s=%.3f waiting_for_gpu_framing_s=%.3f naming_barcodes_s=%.3f commit_s=%.3f stream_setup_s=%.3f records_named_on_host=%llu\n",
                ph.t_idle, ph.t_gpu_wait, ph.t_names, ph.t_commit, ph.t_create, (unsigned long long)ph.total_named);
}

// ---- the counters back, and the names by row: the device dictionary's texts by id (read once, now), then what the host named
void counters_back(Run &rs) {
    const int T = rs.pool->size();
    flush_counts(rs, 1);
    rs.t_classified = now_s();
    Naming &naming = rs.naming;
    Counts &acc = rs.acc;
    std::vector<uint8_t> &dev_texts = rs.dev_texts;
    std::vector<std::string_view> &names = rs.names;
    size_t n_dev_names = 0;
    if (naming.device_dict) {                       // (several dictionaries: the first one holds every text since the merge)
        CK(hast_names_count(naming.groups[0], &n_dev_names), "asking the dictionary for its size");
        dev_texts.resize(16 * n_dev_names);
        CK(hast_names_texts(naming.groups[0], 0, n_dev_names, dev_texts.data()), "reading the dictionary's texts");
    }
    const size_t n_host_names = rs.dict.size();
    names.assign(n_dev_names + n_host_names, std::string_view());
    if (naming.device_dict)
        rs.pool->run([&](int t) {
            for (size_t i = n_dev_names * (size_t)t / T, e = n_dev_names * (size_t)(t + 1) / T; i < e; i++)
                names[i] = std::string_view(reinterpret_cast<const char *>(dev_texts.data()) + 16 * i + 1, dev_texts[16 * i]);
        });
    {
        std::vector<std::string_view> hn(n_host_names);
        rs.pool->run([&](int t) { rs.dict.names_range(hn, hast::BarcodeDict::n_shards() * (size_t)t / T, hast::BarcodeDict::n_shards() * (size_t)(t + 1) / T); });
        std::copy(hn.begin(), hn.end(), names.begin() + (long)n_dev_names);
    }
    // one run of counters in the order of `names`
    if (naming.device_dict) {
        acc.c0.resize(n_dev_names); acc.c1.resize(n_dev_names); acc.neg.resize(n_dev_names);
        acc.h0.resize(n_host_names); acc.h1.resize(n_host_names);
        acc.c0.insert(acc.c0.end(), acc.h0.begin(), acc.h0.end());
        acc.c1.insert(acc.c1.end(), acc.h1.begin(), acc.h1.end());
    }
    // One row per TEXT, not per id.  A single dictionary never gives a text both a device id and leaves it to the host (name_claim.h).
    // Several do: one that has run out hands a text to the host which another, not yet full, numbers in its own blocks (or has numbered
    // long before), and nothing on the way merges the two ranges by text.  Only a host name of at most 15 bytes can have a device id as
    // well, and only once a dictionary has run out is there such a host name: then -- and only then -- the device's texts are looked up
    // among them, the host's row is added to the device's and dropped.
    size_t n_rows_summed = 0;
    if (naming.device_dict && n_dev_names && n_host_names) {
        std::unordered_map<std::string_view, uint32_t> short_host;
        for (size_t j = 0; j < n_host_names; j++)
            if (names[n_dev_names + j].size() <= 15) short_host.emplace(names[n_dev_names + j], (uint32_t)j);
        if (!short_host.empty()) {
            std::vector<char> drop(n_host_names, 0);
            for (size_t i = 0; i < n_dev_names; i++) {
                const auto it = short_host.find(names[i]);
                if (it == short_host.end()) continue;
                acc.c0[i] += acc.c0[n_dev_names + it->second];
                acc.c1[i] += acc.c1[n_dev_names + it->second];
                drop[it->second] = 1;
                n_rows_summed++;
            }
            if (n_rows_summed) {
                size_t to = n_dev_names;
                for (size_t j = 0; j < n_host_names; j++) {
                    if (drop[j]) continue;
                    names[to] = names[n_dev_names + j];
                    acc.c0[to] = acc.c0[n_dev_names + j];
                    acc.c1[to] = acc.c1[n_dev_names + j];
                    to++;
                }
                names.resize(to);
                acc.c0.resize(to);
                acc.c1.resize(to);
            }
        }
    }
    rs.n_dev_names = n_dev_names;
    rs.n_host_names = n_host_names;
    rs.n_rows_summed = n_rows_summed;
    rs.n_rows = names.size();
}

// ---- printBarcodeInfos (classify.cpp:93-102): byte-wise sorted rows ------------------------
// (the reference walks a std::map<std::string, ...>: byte-wise lexicographic order, a prefix in front of what it is a prefix of.
// BASELINE configs 2 / 3 have 1M / 10M barcodes: one std::sort of 10M names and one snprintf per row took seconds on one thread;
// the names are dealt into 65536 buckets by their first two bytes (bucket order = byte order), the buckets are sorted and the rows
// formatted by the parser threads)
void sort_rows(Run &rs) {
    const std::vector<std::string_view> &names = rs.names;
    std::vector<uint32_t> &order = rs.order;
    hast::WorkerPool &pool = *rs.pool;
    const int T = pool.size();
    fprintf(stderr, "__print result__\n");
    const size_t nb = names.size();
    order.assign(nb, 0);
    auto key16 = [&](uint32_t i) -> uint32_t {
        const std::string_view v = names[i];
        return (v.size() > 0 ? (uint32_t)(uint8_t)v[0] << 8 : 0u) | (v.size() > 1 ? (uint32_t)(uint8_t)v[1] : 0u);
    };
    if (nb < (1u << 16) || T == 1) {
        for (uint32_t i = 0; i < nb; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
    } else {
        constexpr size_t kB = 65536;
        std::vector<std::vector<uint32_t>> hist((size_t)T, std::vector<uint32_t>(kB, 0));
        pool.run([&](int t) {
            std::vector<uint32_t> &h = hist[(size_t)t];
            for (size_t i = nb * (size_t)t / T, e = nb * (size_t)(t + 1) / T; i < e; i++) h[key16((uint32_t)i)]++;
        });
        std::vector<size_t> bucket_at(kB + 1, 0);
        {
            size_t at = 0;
            for (size_t k = 0; k < kB; k++) {
                bucket_at[k] = at;
                for (int t = 0; t < T; t++) {
                    const uint32_t c = hist[(size_t)t][k];
                    hist[(size_t)t][k] = (uint32_t)at;              // (nb < 2^32: ids are 32-bit)
                    at += c;
                }
            }
            bucket_at[kB] = at;
        }
        pool.run([&](int t) {
            std::vector<uint32_t> &h = hist[(size_t)t];
            for (size_t i = nb * (size_t)t / T, e = nb * (size_t)(t + 1) / T; i < e; i++) order[h[key16((uint32_t)i)]++] = (uint32_t)i;
        });
        // the buckets, largest first, one at a time to whoever is free (stLFR barcodes are digits: a hundred buckets hold everything, and
        // ten of them sit next to each other -- dealt in runs of 64 keys, one thread got a tenth of the job); inside a bucket: by the next
        // byte, and the next (the ids are moved, the names are looked at once per level), std::sort below 2048 names
        std::vector<uint32_t> big;
        for (size_t k = 0; k < kB; k++)
            if (bucket_at[k + 1] - bucket_at[k] > 1) big.push_back((uint32_t)k);
        std::sort(big.begin(), big.end(), [&](uint32_t a, uint32_t b) { return bucket_at[a + 1] - bucket_at[a] > bucket_at[b + 1] - bucket_at[b]; });
        std::atomic<size_t> next_bucket{0};
        pool.run([&](int) {
            std::vector<uint32_t> tmp;
            struct Range { size_t lo, hi, depth; };
            std::vector<Range> todo;
            for (;;) {
                const size_t bi = next_bucket.fetch_add(1);
                if (bi >= big.size()) break;
                todo.push_back({bucket_at[big[bi]], bucket_at[big[bi] + 1], 2});
                while (!todo.empty()) {
                    const Range r = todo.back();
                    todo.pop_back();
                    const size_t n = r.hi - r.lo;
                    if (n < 2048 || r.depth > 64) {
                        std::sort(order.begin() + (long)r.lo, order.begin() + (long)r.hi, [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
                        continue;
                    }
                    // counting sort by the byte at r.depth; names that end here (shorter: a prefix of the others) come first
                    size_t cnt[257] = {0};
                    auto byte_at = [&](uint32_t id) -> size_t { const std::string_view v = names[id]; return v.size() > r.depth ? (size_t)(uint8_t)v[r.depth] + 1 : 0; };
                    for (size_t i = r.lo; i < r.hi; i++) cnt[byte_at(order[i])]++;
                    size_t at[258];
                    at[0] = 0;
                    for (int b = 0; b < 257; b++) at[b + 1] = at[b] + cnt[b];
                    tmp.resize(n);
                    {
                        size_t pos[257];
                        for (int b = 0; b < 257; b++) pos[b] = at[b];
                        for (size_t i = r.lo; i < r.hi; i++) tmp[pos[byte_at(order[i])]++] = order[i];
                    }
                    std::copy(tmp.begin(), tmp.begin() + (long)n, order.begin() + (long)r.lo);
                    for (int b = 1; b < 257; b++)                          // (slot 0: identical names cannot be, ids are one per name)
                        if (cnt[b] > 1) todo.push_back({r.lo + at[b], r.lo + at[b + 1], r.depth + 1});
                }
            }
        });
    }
}

void put_u64(std::string &out, uint64_t v) {
    char tmp[24];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) out.push_back(tmp[--n]);
}

// rows: formatted by all threads, each a contiguous share of the sorted order, written in that order
void print_rows(Run &rs) {
    const Options &o = rs.o;
    const std::vector<std::string_view> &names = rs.names;
    const std::vector<uint32_t> &order = rs.order;
    const Counts &acc = rs.acc;
    hast::WorkerPool &pool = *rs.pool;
    const int T = pool.size();
    const size_t nb = names.size();
    auto format_rows = [&](size_t lo, size_t hi, std::string &out, bool &past) {
        for (size_t r = lo; r < hi; r++) {
            const uint32_t i = order[r];
            const std::string_view bc = names[i];
            const uint64_t c0 = i < acc.c0.size() ? acc.c0[i] : 0, c1 = i < acc.c1.size() ? acc.c1[i] : 0;
            const int hap = hast_get_hap(bc.data(), bc.size(), c0, c1, rs.n_set[0], rs.n_set[1], o.w0, o.w1);
            out.append(bc.data(), bc.size());
            // the reference prints `int` counters (classify.cpp:51,98-100): the same digits up to INT_MAX; past it the reference's
            // counter has overflowed (undefined behaviour there) -- the exact count is printed and the run says so once
            past = past || c0 > 0x7FFFFFFFull || c1 > 0x7FFFFFFFull;
            out.push_back('\t');
            if (hap < 0) out.append("-1");
            else out.push_back((char)('0' + hap));
            out.push_back('\t');
            put_u64(out, c0);
            out.push_back('\t');
            put_u64(out, c1);
            out.push_back('\n');
        }
    };
    // (the wrapper redirects stdout into phased.barcodes and tests only the exit status, classify_stlfr_reads.sh:149: a full disk
    // or a closed pipe must not leave a truncated table behind exit 0)
    const size_t kRowsPerPiece = 1u << 16;
    for (size_t r0 = 0; r0 < nb; r0 += kRowsPerPiece * (size_t)T) {
        const size_t r1 = std::min(nb, r0 + kRowsPerPiece * (size_t)T);
        std::vector<std::string> piece((size_t)T);
        std::vector<char> past((size_t)T, 0);
        pool.run([&](int t) {
            const size_t lo = r0 + (r1 - r0) * (size_t)t / T, hi = r0 + (r1 - r0) * (size_t)(t + 1) / T;
            bool p = false;
            piece[(size_t)t].reserve((hi - lo) * 24);
            format_rows(lo, hi, piece[(size_t)t], p);
            past[(size_t)t] = p;
        });
        for (int t = 0; t < T; t++) {
            rs.past_int = rs.past_int || past[(size_t)t];
            if (fwrite(piece[(size_t)t].data(), 1, piece[(size_t)t].size(), stdout) != piece[(size_t)t].size()) die_output();
        }
    }
    if (fflush(stdout) != 0) die_output();
}

// ---- --rows device: the table keyed, called, sorted, sized and formatted in HBM (hast_rows_*, rows_kernels.hip) ---------------------
// The texts lie in the device dictionary and the counters in the context's arrays: 16 + 32 bytes a barcode that the host route reads
// back, sorts and formats with its threads.  Here only the finished text crosses PCIe.  What the device cannot do this for goes the
// host's way, whole, and says why: texts or counts that only the host holds would have to be merged into a table sorted elsewhere.
// Returns null when the table is in rs.rows, else the reason.
const char *rows_on_device(Run &rs) {
    const Options &o = rs.o;
    Naming &naming = rs.naming;
    if (!naming.device_dict) return "no_device_dictionary";
    if (naming.groups.size() != 1) return "several_dictionaries";
    if (rs.dict.size() != 0) return "host_names";                     // (texts the dictionary left to the host: their rows are not on the device)
    if (rs.acc.folded) return "counts_on_host";                       // (the counters were read back and sized anew on the way)
    size_t n = 0;
    CK(hast_names_count(naming.groups[0], &n), "asking the dictionary for its size");
    if (n > rs.acc.device_cap) return "counts_on_host";
    sum_counts_on_devices(rs);                                        // (several contexts of the one GPU: the totals, where they lie)
    rs.counts_summed = true;
    const hast_status st = hast_rows_build(rs.ctx, naming.groups[0], n, rs.n_set[0], rs.n_set[1], o.w0, o.w1, o.phase_reads ? 1 : 0, &rs.rows);
    if (st == HAST_ERR_OOM) return "no_room";
    if (st != HAST_OK) die(4, "making the table on the GPU");
    rs.t_classified = now_s();
    rs.n_dev_names = rs.n_rows = n;
    return nullptr;
}

// text `which` of the device's table to f: piece k is written while piece k + 1 comes down (the library stages through two pinned buffers)
bool write_rows_text(hast_rows *rows, int which, uint64_t total, FILE *f) {
    const size_t kPiece = 8u << 20;
    std::vector<uint8_t> buf[2];
    const uint64_t pieces = (total + kPiece - 1) / kPiece;
    auto fetch = [&](uint64_t k) {
        const size_t n = (size_t)std::min<uint64_t>(kPiece, total - k * kPiece);
        buf[k & 1].resize(n);
        return std::async(std::launch::async, [=, &buf] { return hast_rows_read(rows, which, k * kPiece, n, buf[k & 1].data()); });
    };
    std::future<hast_status> pending;
    if (pieces) pending = fetch(0);
    for (uint64_t k = 0; k < pieces; k++) {
        if (pending.get() != HAST_OK) die(4, "reading the table from the GPU");
        if (k + 1 < pieces) pending = fetch(k + 1);
        if (fwrite(buf[k & 1].data(), 1, buf[k & 1].size(), f) != buf[k & 1].size()) {
            if (pending.valid()) pending.wait();
            return false;
        }
    }
    return true;
}

void print_rows_from_device(Run &rs) {
    fprintf(stderr, "__print result__\n");
    hast_rows_info info;
    CK(hast_rows_get_info(rs.rows, &info), "asking for the table's sizes");
    const double t0 = now_s();
    // (as print_rows: a full disk or a closed pipe must not leave a truncated table behind exit 0)
    if (!write_rows_text(rs.rows, 0, info.table_bytes, stdout)) die_output();
    if (fflush(stdout) != 0) die_output();
    rs.rows_download_write_s = now_s() - t0;
    rs.past_int = info.past_int != 0;
}

void stat_rows(const Run &rs) {
    hast_rows_info info = {};
    if (rs.rows) (void)hast_rows_get_info(rs.rows, &info);
    stat_line("__stats_rows__ route=%s fallback=%s rows=%zu table_bytes=%llu list_bytes=%llu,%llu,%llu keys_s=%.3f sort_s=%.3f format_s=%.3f download_write_s=%.3f\n",
              rs.rows ? "device" : "host", rs.rows_fallback, rs.n_rows, (unsigned long long)info.table_bytes, (unsigned long long)info.list_bytes[0],
              (unsigned long long)info.list_bytes[1], (unsigned long long)info.list_bytes[2], info.keys_s, info.sort_s, info.format_s, rs.rows_download_write_s);
}

// ---- HAST_PHASE_READS=1: steps 10 and 11 of the wrapper (classify_stlfr_reads.sh:155-190) done here -------------------------
// The wrapper derives three barcode lists from the table above with awk and then routes every record of every input to
// <name>.{paternal,maternal,homozygous,nobarcode}.fastq with a single-threaded awk program, re-reading (and re-inflating) every
// input.  This program has the barcodes' classes in memory and a GPU that inflates .gz inputs: with HAST_PHASE_READS set it writes the
// lists, routes the records (quartering.h: the same bytes as the awk program's, incl. filter_reads.log and the ERROR lines) and
// leaves the marker files step_10_done / step_11_done, at which the UNCHANGED wrapper skips its own steps 10 and 11.
namespace hq = hast::quartering;

struct PhaseReads {
    std::vector<uint8_t> list_of;                  // per name: list 1 paternal (hap 0), 2 maternal (hap 1), 3 homozygous (-1)
    bool any_sep = false;                          // a barcode that itself holds '#' or '/'
    // awk's three arrays as one map: a list line's first field under -F '#|/', first list wins (awk :12-16,23-35).  10M insertions of
    // std::string take seconds: built only when the host has to route something
    hq::ClassMap cls_of;
    bool cls_ready = false;
    uint64_t blocks_routed = 0, blocks_host = 0, bytes_routed = 0;
    struct GzIn { hq::GzOutStats dev, host; };     // --gz-out, per input: into / out of the GPU's encoder and zlib, members written
    std::vector<GzIn> gz_in;
    double t_wait_write = 0, t_wait_gpu = 0;
};

// the call of every barcode once (getHap, classify.cpp:66-86), and the three lists
void write_lists(Run &rs, PhaseReads &pr) {
    const Options &o = rs.o;
    const std::vector<std::string_view> &names = rs.names;
    const std::vector<uint32_t> &order = rs.order;
    const Counts &acc = rs.acc;
    hast::WorkerPool &pool = *rs.pool;
    const int T = pool.size();
    const size_t nb = names.size();
    const char *list_name[3] = {"paternal.unique.barcodes", "maternal.unique.barcodes", "homozygous.unique.barcodes"};
    std::vector<uint8_t> &list_of = pr.list_of;
    list_of.assign(nb, 0);
    std::vector<char> has_sep((size_t)T, 0);
    pool.run([&](int t) {
        for (size_t i = nb * (size_t)t / T, e = nb * (size_t)(t + 1) / T; i < e; i++) {
            const std::string_view bc = names[i];
            const uint64_t c0 = i < acc.c0.size() ? acc.c0[i] : 0, c1 = i < acc.c1.size() ? acc.c1[i] : 0;
            const int hap = hast_get_hap(bc.data(), bc.size(), c0, c1, rs.n_set[0], rs.n_set[1], o.w0, o.w1);
            list_of[i] = hap == 0 ? 1 : hap == 1 ? 2 : 3;
            if (bc.find('#') != std::string_view::npos || bc.find('/') != std::string_view::npos) has_sep[(size_t)t] = 1;
        }
    });
    {
        // (one walk over the sorted rows, each thread a contiguous share: the three lists are the rows' first columns in row order)
        std::vector<std::string> part((size_t)T * 3);
        pool.run([&](int t) {
            for (size_t r = nb * (size_t)t / T, e = nb * (size_t)(t + 1) / T; r < e; r++) {
                const uint32_t i = order[r];
                std::string &text = part[(size_t)t * 3 + (size_t)(list_of[i] - 1)];
                text.append(names[i].data(), names[i].size());
                text.push_back('\n');
            }
        });
        for (int l = 0; l < 3; l++) {
            FILE *lf = fopen(list_name[l], "wb");
            bool ok = lf != nullptr;
            for (int t = 0; ok && t < T; t++) {
                const std::string &text = part[(size_t)t * 3 + (size_t)l];
                ok = fwrite(text.data(), 1, text.size(), lf) == text.size();
            }
            if (!ok || fclose(lf) != 0) die(2, (std::string("cannot write ") + list_name[l]).c_str());
        }
    }
    for (char c : has_sep) pr.any_sep = pr.any_sep || c;
}

// --rows device: the three lists as the GPU wrote them.  The router still goes by names, order and classes on the host (need_cls,
// host_class, build_routing_tables): downloads, no sort and no call is made here
void write_lists_from_device(Run &rs, PhaseReads &pr) {
    const char *list_name[3] = {"paternal.unique.barcodes", "maternal.unique.barcodes", "homozygous.unique.barcodes"};
    hast_rows_info info;
    CK(hast_rows_get_info(rs.rows, &info), "asking for the lists' sizes");
    for (int l = 0; l < 3; l++) {
        FILE *lf = fopen(list_name[l], "wb");                     // (a list with no line is created all the same)
        if (!lf || !write_rows_text(rs.rows, l + 1, info.list_bytes[l], lf) || fclose(lf) != 0) die(2, (std::string("cannot write ") + list_name[l]).c_str());
    }
    const size_t n = rs.n_rows;
    rs.dev_texts.resize(16 * n);
    CK(hast_names_texts(rs.naming.groups[0], 0, n, rs.dev_texts.data()), "reading the dictionary's texts");
    rs.names.assign(n, std::string_view());
    for (size_t i = 0; i < n; i++) rs.names[i] = std::string_view(reinterpret_cast<const char *>(rs.dev_texts.data()) + 16 * i + 1, rs.dev_texts[16 * i]);
    rs.order.assign(n, 0);
    CK(hast_rows_order(rs.rows, rs.order.data()), "reading the order of the rows");
    pr.list_of.assign(n, 0);
    CK(hast_rows_classes(rs.rows, pr.list_of.data()), "reading the barcodes' lists");
    pr.any_sep = info.any_sep != 0;
}

void need_cls(const Run &rs, PhaseReads &pr) {
    if (pr.cls_ready) return;
    for (int l = 0; l < 3; l++)
        for (size_t r = 0; r < rs.order.size(); r++) {
            const uint32_t i = rs.order[r];
            if (pr.list_of[i] == l + 1) pr.cls_of.emplace(std::string(hq::field(rs.names[i], 0)), (uint8_t)(l + 1));
        }
    pr.cls_ready = true;
}

// a record the device left to the host: its class by the host's rules (quartering.h's classify)
int host_class(const Run &rs, PhaseReads &pr, std::string_view head, std::string &err) {
    std::string_view f2 = hq::field(head, 1);
    if (f2.data() == nullptr || f2 == "0_0_0") return 0;
    need_cls(rs, pr);
    auto it = pr.cls_of.find(std::string(f2));
    if (it != pr.cls_of.end()) return it->second;
    err.append("ERROR : unclassify barcode : ").append(f2).append("\n");
    return -1;
}

// ---- the device router: the inputs go through the framer once more (.gz inputs inflated there again), a kernel sorts the records
// of every block into four runs by the class of their barcode, the runs come back over PCIe and are written as they are -- no
// host thread looks at a record.
struct WriteJob { const uint8_t *p[4]; size_t n[4]; std::shared_ptr<std::vector<std::string>> own; };

// a feed, and the four files its runs go to
struct RoutedFeed {
    hast::FqFeed feed;
    std::string prefix, log_name;
    std::thread wth[4];
    std::mutex wmu;
    std::condition_variable wcv;
    std::deque<WriteJob> wq[4];                             // per class: a writer thread per output file
    std::atomic<bool> write_failed{false};
    bool wstop = false, block_open = false;                 // block_open: its runs are being written, the commit waits for them
    size_t jobs = 0, written = 0;
    FILE *out[4] = {nullptr, nullptr, nullptr, nullptr};
    long long counts[5] = {0, 0, 0, 0, 0};
    bool any_input = false;
    std::string err_lines;
};

struct DeviceRouter {
    std::vector<hast_names *> tabs;                         // per context: the table text -> class of its GPU
    const char *const *suffix = nullptr;
    hast::FeedWake wake;
    std::vector<std::unique_ptr<RoutedFeed>> active, finished;
    size_t next_file = 0;
};

[[noreturn]] void die_routed_write(const RoutedFeed &f) {
    fprintf(stderr, "classify: cannot write %s.*.fastq\n", f.prefix.c_str());
    fflush(stderr);
    _exit(2);
}

// the table text -> class of every GPU
void build_routing_tables(Run &rs, const PhaseReads &pr, DeviceRouter &dr) {
    const std::vector<int> &devices = rs.o.devices;
    dr.tabs.assign(rs.ctxs.size(), nullptr);
    std::vector<uint8_t> text16;
    std::vector<uint32_t> cls;
    text16.reserve(rs.names.size() * 16);
    cls.reserve(rs.names.size());
    for (size_t i = 0; i < rs.names.size(); i++) {
        const std::string_view bc = rs.names[i];
        if (bc.size() > 15) continue;                    // (a field that long is the host's: the kernel hands the block over)
        uint8_t rec[16] = {0};
        rec[0] = (uint8_t)bc.size();
        memcpy(rec + 1, bc.data(), bc.size());
        text16.insert(text16.end(), rec, rec + 16);
        cls.push_back(pr.list_of[i]);
    }
    for (size_t i = 0; i < rs.ctxs.size(); i++) {
        for (size_t j = 0; j < i && !dr.tabs[i]; j++)
            if (devices[j] == devices[i]) dr.tabs[i] = dr.tabs[j];
        if (dr.tabs[i]) continue;
        CK(hast_names_create(rs.ctxs[i], std::max<size_t>(cls.size(), 1024), &dr.tabs[i]), "creating the routing table");
        rs.own_tabs.push_back(dr.tabs[i]);
        CK(hast_names_insert(dr.tabs[i], text16.data(), cls.data(), cls.size()), "filling the routing table");
    }
}

// the runs of class c to its file, in order (a thread per file: what bounds the routing is the write, 17 GB per file at BASELINE
// config 2)
void write_runs(RoutedFeed *fp, int c, const char *suffix, hast::FeedWake &wake) {
    for (;;) {
        WriteJob j;
        {
            std::unique_lock<std::mutex> g(fp->wmu);
            fp->wcv.wait(g, [fp, c] { return fp->wstop || !fp->wq[c].empty(); });
            if (fp->wq[c].empty()) return;
            j = std::move(fp->wq[c].front());
            fp->wq[c].pop_front();
        }
        if (j.n[c] && !fp->write_failed.load()) {
            if (!fp->out[c]) fp->out[c] = fopen((fp->prefix + suffix).c_str(), "wb");
            if (!fp->out[c] || fwrite(j.p[c], 1, j.n[c], fp->out[c]) != j.n[c]) fp->write_failed = true;
        }
        {
            std::lock_guard<std::mutex> g(fp->wmu);
            fp->written++;
        }
        wake.wake();
    }
}

void open_next_routed(Run &rs, DeviceRouter &dr) {
    const size_t fi = dr.next_file++;
    const std::string &x = rs.o.read[fi];
    std::unique_ptr<RoutedFeed> f(new RoutedFeed());
    f->feed.name = x;
    f->feed.file_index = fi;
    const InputName in = input_name(x);
    f->prefix = in.base;
    f->log_name = in.gz ? "-" : x;                          // (awk's FILENAME behind `gzip -dc` is "-")
    if (rs.dev_gz[fi]) {
        const hast_status gs = open_gz(rs, fi, &f->feed.gz);
        if (gs == HAST_ERR_UNSUPPORTED) {
            f->feed.gz = nullptr;
            rs.dev_gz[fi] = rs.dev_bz[fi] = 0;
        } else if (gs != HAST_OK) die(2, ("cannot open " + x).c_str());
    }
    const size_t cap = cap_of(rs, fi);
    open_host_source(rs, f->feed, cap);
    CK(make_fq(rs, fi, &f->feed.fq), "creating the FASTQ stream");
    std::vector<hast_names *> lane_tabs;
    if (rs.stripe) lane_tabs = dr.tabs;
    else lane_tabs.push_back(dr.tabs[fi % rs.ctxs.size()]);
    CK(hast_fq_set_route(f->feed.fq, lane_tabs.data(), (int)lane_tabs.size()), "switching the FASTQ stream to routing");
    CK(hast_fq_set_route_gz(f->feed.fq, rs.o.gz_out ? (rs.o.gz_bgzf ? 2 : 1) : 0), "switching the routed runs to gzip members");
    start_feed(rs, f->feed, dr.wake, cap);
    RoutedFeed *fp = f.get();
    for (int c = 0; c < 4; c++) f->wth[c] = std::thread(write_runs, fp, c, dr.suffix[c], std::ref(dr.wake));
    dr.active.push_back(std::move(f));
}

// the four runs of a block as the device sorted them
void runs_from_device(Run &rs, PhaseReads &pr, RoutedFeed &f, const hast_fq_routed &b, WriteJob &j) {
    const bool gz_out = rs.o.gz_out;
    for (int c = 0; c < 4; c++) {
        j.p[c] = b.run[c];
        j.n[c] = (size_t)b.run_bytes[c];
        f.counts[c] += (long long)b.count[c];
        if (!gz_out) pr.bytes_routed += b.run_bytes[c];
    }
    if (gz_out) {
        uint64_t raw[4];
        CK(hast_fq_routed_raw_bytes(f.feed.fq, raw), "asking for the runs' sizes");
        hq::GzOutStats &dev = pr.gz_in[f.feed.file_index].dev;
        for (int c = 0; c < 4; c++) {
            pr.bytes_routed += raw[c];                   // (the records' bytes, as without the flag; the members' sizes: __stats_route_gz__)
            dev.bytes_in += raw[c];
            dev.bytes_out += b.run_bytes[c];
            dev.members += rs.o.gz_bgzf ? hq::bgzf_member_count(raw[c]) : b.run_bytes[c] != 0;
        }
    }
    f.counts[4] += (long long)b.n_records;
    if (b.n_records) f.any_input = true;
    pr.blocks_routed++;
}

void point_at_own(WriteJob &j) {
    for (int c = 0; c < 4; c++) { j.p[c] = reinterpret_cast<const uint8_t *>((*j.own)[(size_t)c].data()); j.n[c] = (*j.own)[(size_t)c].size(); }
}

// n bytes of records as the host compresses them, appended to out: one gzip member, or the BGZF members of their slices
void host_members(Run &rs, const char *p, size_t n, std::string &out, hq::GzOutStats &host, const char *what) {
    const size_t before = out.size();
    if (!(rs.o.gz_bgzf ? hq::bgzf_members(p, n, out) : hq::gz_member(p, n, out))) die(2, what);
    host.bytes_in += n;
    host.bytes_out += out.size() - before;
    host.members += rs.o.gz_bgzf ? hq::bgzf_member_count(n) : 1;
}

// a block the device handed over: every record by the host's rules, in input order
void runs_from_host(Run &rs, PhaseReads &pr, RoutedFeed &f, const hast_fq_routed &b, WriteJob &j) {
    hq::GzOutStats &host = pr.gz_in[f.feed.file_index].host;
    j.own = std::make_shared<std::vector<std::string>>(4);
    for (uint64_t i = 0; i < b.n_slots; i++) {
        if (b.rec_class[i] == 0xFD) continue;
        const char *r0 = reinterpret_cast<const char *>(b.bytes) + b.rec_start[i];
        const size_t len = b.rec_len[i];
        int c = b.rec_class[i];
        if (c > 3) {
            const void *nlp = memchr(r0, '\n', len);
            c = host_class(rs, pr, std::string_view(r0, nlp ? (size_t)((const char *)nlp - r0) : len), f.err_lines);
        }
        f.counts[4]++;
        f.any_input = true;
        if (c >= 0) { (*j.own)[(size_t)c].append(r0, len); f.counts[c]++; }
    }
    if (rs.o.gz_out)                                        // the caller's block: its records compressed by zlib, a member per class
        for (int c = 0; c < 4; c++) {
            std::string &plain = (*j.own)[(size_t)c], z;
            if (plain.empty()) continue;
            host_members(rs, plain.data(), plain.size(), z, host, "cannot compress a block of routed records");
            plain.swap(z);
        }
    point_at_own(j);
    pr.blocks_host++;
}

// the end of the file inside a record: awk still takes every remaining line as the record's (:21,41-49)
void append_tail(Run &rs, PhaseReads &pr, RoutedFeed &f, const hast_fq_routed &b, WriteJob &j) {
    hq::GzOutStats &host = pr.gz_in[f.feed.file_index].host;
    if (!j.own) {
        j.own = std::make_shared<std::vector<std::string>>(4);
        for (int c = 0; c < 4; c++) (*j.own)[(size_t)c].assign(reinterpret_cast<const char *>(j.p[c]), j.n[c]);
    }
    std::string_view rest(reinterpret_cast<const char *>(b.tail), (size_t)b.tail_bytes);
    const size_t e = rest.find('\n');
    const int c = host_class(rs, pr, rest.substr(0, e == std::string_view::npos ? rest.size() : e), f.err_lines);
    f.counts[4]++;
    f.any_input = true;
    if (c >= 0) {
        std::string rec(rest);
        if (rec.back() != '\n') rec.push_back('\n');
        if (rs.o.gz_out) host_members(rs, rec.data(), rec.size(), (*j.own)[(size_t)c], host, "cannot compress the last record");      // a member of its own behind the block's
        else (*j.own)[(size_t)c].append(rec);
        f.counts[c]++;
    }
    point_at_own(j);
}

// the oldest submitted block of a feed: its runs to the four writers; the commit follows when they are through
void route_block(Run &rs, PhaseReads &pr, RoutedFeed &f) {
    hast_fq_routed b;
    const double t0 = now_s();
    CK(hast_fq_next_routed(f.feed.fq, &b), "routing a block");
    pr.t_wait_gpu += now_s() - t0;
    WriteJob j;
    for (int c = 0; c < 4; c++) { j.p[c] = nullptr; j.n[c] = 0; }
    if (!b.host_block) runs_from_device(rs, pr, f, b, j);
    else runs_from_host(rs, pr, f, b, j);
    if (b.tail_bytes) append_tail(rs, pr, f, b, j);
    {
        std::lock_guard<std::mutex> g(f.wmu);
        for (int c = 0; c < 4; c++) f.wq[c].push_back(j);
        f.jobs += 4;
    }
    f.wcv.notify_all();
    f.block_open = true;
    f.feed.opened++;
}

// the runs of the open block are written: the buffer goes back.  Returns whether they were
bool commit_when_written(RoutedFeed &f) {
    bool done;
    {
        std::lock_guard<std::mutex> g(f.wmu);
        done = f.written == f.jobs;
    }
    if (!done) return false;
    if (f.write_failed.load()) die_routed_write(f);
    CK(hast_fq_commit(f.feed.fq), "releasing a block");
    f.block_open = false;
    f.feed.held--;
    return true;
}

void retire_routed(Run &rs, PhaseReads &pr, RoutedFeed &f) {
    f.feed.stop_reader();
    {
        std::lock_guard<std::mutex> g(f.wmu);
        f.wstop = true;
    }
    f.wcv.notify_all();
    for (std::thread &w : f.wth) w.join();
    for (FILE *&o : f.out) {
        if (!o) continue;
        if (rs.o.gz_bgzf) {                                 // every BGZF file that exists ends with one end-of-file block
            if (fwrite(hq::kBgzfEof, 1, sizeof hq::kBgzfEof, o) != sizeof hq::kBgzfEof) die_routed_write(f);
            hq::GzOutStats &host = pr.gz_in[f.feed.file_index].host;
            host.bytes_out += sizeof hq::kBgzfEof;
            host.members++;
        }
        if (fclose(o) != 0) die_routed_write(f);
    }
    if (f.feed.gz) {
        hast_gz *z = f.feed.gz;
        rs.gz_closers.emplace_back([z] { hast_gz_close(z); });
    }
    rs.done_fq.push_back(f.feed.fq);
}

// stderr and filter_reads.log in the order of the inputs, as the wrapper's loop leaves them (awk :18-20,51-57)
void write_filter_log(const std::vector<std::unique_ptr<RoutedFeed>> &finished) {
    for (const std::unique_ptr<RoutedFeed> &fp : finished) {
        if (!fp) continue;
        fputs(fp->err_lines.c_str(), stderr);
        FILE *lg = fopen("filter_reads.log", "ab");
        if (lg) {
            if (fp->any_input) fprintf(lg, "%s\n", fp->log_name.c_str());
            fprintf(lg, "#Total reads                : %lld \n", fp->counts[4]);
            fprintf(lg, "#Reads without barcode      : %lld \n", fp->counts[0]);
            fprintf(lg, "#Paternal reads             : %lld \n", fp->counts[1]);
            fprintf(lg, "#Maternal reads             : %lld \n", fp->counts[2]);
            fprintf(lg, "#Homozygous reads           : %lld \n", fp->counts[3]);
            fclose(lg);
        }
    }
}

void route_on_device(Run &rs, PhaseReads &pr) {
    const std::vector<std::string> &read = rs.o.read;
    static const char *const suffix_plain[4] = {".nobarcode.fastq", ".paternal.fastq", ".maternal.fastq", ".homozygous.fastq"};
    static const char *const suffix_gz[4] = {".nobarcode.fastq.gz", ".paternal.fastq.gz", ".maternal.fastq.gz", ".homozygous.fastq.gz"};
    DeviceRouter dr;
    dr.suffix = rs.o.gz_out ? suffix_gz : suffix_plain;
    dr.finished.resize(read.size());
    build_routing_tables(rs, pr, dr);
    rs.done_fq.clear();                                     // (as before: the first pass's streams are left to the end of the process, also under HAST_TEARDOWN)
    // inputs with one basename write the same four files: the awk loop lets the later one overwrite the earlier -- one at a time then
    bool same_prefix = false;
    {
        std::vector<std::string> pf;
        for (const std::string &x : read) {
            const std::string nm = input_name(x).base;
            same_prefix = same_prefix || std::find(pf.begin(), pf.end(), nm) != pf.end();
            pf.push_back(nm);
        }
    }
    const size_t max_active = inputs_open_at_once(rs, same_prefix);
    while (dr.next_file < read.size() && dr.active.size() < max_active) open_next_routed(rs, dr);
    while (!dr.active.empty()) {
        bool progress = false;
        for (std::unique_ptr<RoutedFeed> &f : dr.active)
            if (pump(f->feed)) progress = true;
        for (size_t fi = 0; fi < dr.active.size();) {
            RoutedFeed &f = *dr.active[fi];
            if (f.block_open && commit_when_written(f)) progress = true;
            if (!f.block_open && f.feed.block_ready()) {
                route_block(rs, pr, f);
                progress = true;
            }
            if (f.feed.drained() && !f.block_open) {
                retire_routed(rs, pr, f);
                const size_t idx = f.feed.file_index;
                dr.finished[idx] = std::move(dr.active[fi]);
                dr.active.erase(dr.active.begin() + (long)fi);
                if (dr.next_file < read.size()) open_next_routed(rs, dr);
                progress = true;
                continue;
            }
            ++fi;
        }
        if (!progress) pr.t_wait_write += idle_wait(rs, dr.wake);
    }
    write_filter_log(dr.finished);
}

// ---- the host router: the inputs are parsed again by the worker threads, quartering.h
// a .gz input inflated on the GPU, as a block source for the router: the bytes come back over PCIe block by block
struct DevGzSource {
    static constexpr size_t kFrontPad = hast::BlockSource::kFrontPad;     // (room in front of a block's data: what route() expects)
    hast_ctx *ctx = nullptr;
    hast_gz *gz = nullptr;
    void *d_buf = nullptr;
    size_t cap = 0;
    std::string err;
    std::vector<std::vector<char>> spare;
    ~DevGzSource() {
        if (gz) hast_gz_close(gz);
        if (d_buf) hast_dev_free(ctx, d_buf);
    }
    std::vector<char> next() {
        if (!err.empty()) return {};
        std::vector<char> blk;
        if (!spare.empty()) { blk = std::move(spare.back()); spare.pop_back(); }
        blk.resize(kFrontPad + cap);
        size_t n = 0;
        if (hast_gz_read_device(gz, static_cast<uint8_t *>(d_buf), cap, &n, nullptr) != HAST_OK ||
            (n && hast_memcpy_d2h(ctx, blk.data() + kFrontPad, d_buf, n) != HAST_OK)) {
            err = hast_last_error();
            return {};
        }
        if (n == 0) return {};                       // (a short block is followed by another call: damage behind it is reported then)
        blk.resize(kFrontPad + n);
        return blk;
    }
    void recycle(std::vector<char> &&b) { spare.push_back(std::move(b)); }
    const std::string &error() const { return err; }
};

void route_on_host(Run &rs, PhaseReads &pr) {
    const Options &o = rs.o;
    hast_ctx *ctx = rs.ctx;
    need_cls(rs, pr);
    const hq::ClassMap &cls_of = pr.cls_of;
    for (size_t fi = 0; fi < o.read.size(); fi++) {
        const std::string &x = o.read[fi];
        const InputName in = input_name(x);
        const std::string &name = in.base;
        const bool gz_name = in.gz;
        int rc;
        if (gz_name && rs.dev_gz[fi]) {
            DevGzSource src;
            src.ctx = ctx;
            src.cap = 64u << 20;
            if ((rs.dev_bz[fi] ? hast_gz_open_blocked(ctx, x.c_str(), &src.gz) : hast_gz_open(ctx, x.c_str(), &src.gz)) != HAST_OK || hast_dev_alloc(ctx, src.cap, &src.d_buf) != HAST_OK) {
                src.gz = nullptr;                        // (no room on the device, ...: the host inflates)
                hast::BlockSource hsrc;
                if (!hsrc.open(x, 64u << 20)) die(2, ("cannot open " + x).c_str());
                rc = hq::route(name, cls_of, hsrc, "-", o.t_num, "classify", o.gz_format(), &pr.gz_in[fi].host);
            } else rc = hq::route(name, cls_of, src, "-", o.t_num, "classify", o.gz_format(), &pr.gz_in[fi].host);
        } else {
            hast::BlockSource hsrc;
            if (!hsrc.open(x, 64u << 20)) die(2, ("cannot open " + x).c_str());
            rc = hq::route(name, cls_of, hsrc, gz_name ? "-" : x, o.t_num, "classify", o.gz_format(), &pr.gz_in[fi].host);       // (awk's FILENAME behind `gzip -dc` is "-")
        }
        if (rc) {
            fprintf(stderr, "classify: ERROR: routing the reads of %s failed\n", x.c_str());
            fflush(stderr);
            _exit(rc);
        }
    }
}

void phase_reads(Run &rs) {
    const Options &o = rs.o;
    const double t_ph0 = now_s();
    PhaseReads pr;
    pr.gz_in.resize(o.read.size());
    if (rs.rows) write_lists_from_device(rs, pr);
    else write_lists(rs, pr);
    const double t_lists = now_s();
    // On the GPU (default).  On the host (--route host; --host-parse; a barcode that itself holds '#' or '/', whose list line awk cuts
    // short).
    const bool on_device = !o.host_parse && o.route_mode != "host" && !pr.any_sep;
    if (on_device) route_on_device(rs, pr);
    else route_on_host(rs, pr);
    for (const char *marker : {"step_10_done", "step_11_done"}) {
        FILE *mf = fopen(marker, "ab");                   // (the wrapper appends `date` to them and only tests that they exist)
        time_t now = time(0);
        if (!mf || fprintf(mf, "%s", ctime(&now)) < 0 || fclose(mf) != 0) die(2, (std::string("cannot write ") + marker).c_str());
    }
    if (o.stats)
        stat_line("__stats_phase_reads__ lists_and_routing_s=%.3f lists_s=%.3f routing_s=%.3f route=%s inputs=%zu blocks_routed_on_device=%llu blocks_routed_by_host=%llu "
                        "bytes_routed_on_device=%llu waiting_for_gpu_s=%.3f idle_s=%.3f\n",
                now_s() - t_ph0, t_lists - t_ph0, now_s() - t_lists, on_device ? "device" : "host", o.read.size(), (unsigned long long)pr.blocks_routed,
                (unsigned long long)pr.blocks_host, (unsigned long long)pr.bytes_routed, pr.t_wait_gpu, pr.t_wait_write);
    if (o.stats && o.gz_out)                                // one line per input, in the order of the inputs
        for (size_t i = 0; i < o.read.size(); i++) {
            const PhaseReads::GzIn &g = pr.gz_in[i];
            // (format=bgzf is said, gzip is not: the line of a run without --gz-format stays what it was, and what sums its fields still can)
            stat_line("__stats_route_gz__ file=%s%s device_bytes_in=%llu device_bytes_out=%llu device_members=%llu host_bytes_in=%llu host_bytes_out=%llu host_members=%llu\n",
                      o.read[i].c_str(), o.gz_bgzf ? " format=bgzf" : "", g.dev.bytes_in, g.dev.bytes_out, g.dev.members, g.host.bytes_in, g.host.bytes_out, g.host.members);
        }
}

// where a run's wall time goes, phase by phase (sums to the process's own lifetime from main() on).  teardown_s: null = skipped
void stat_phases(const Run &rs, const double *teardown_s) {
    char teardown[32] = "skipped";
    if (teardown_s) snprintf(teardown, sizeof(teardown), "%.3f", *teardown_s);
    stat_line("__stats_phases__ gpu_context_s=%.3f load_kmers_s=%.3f scrub_sizes_clone_s=%.3f read_phase_s=%.3f counters_back_s=%.3f sort_print_s=%.3f teardown_s=%s total_s=%.3f\n",
              rs.t_ctx - rs.t_start, rs.t_loaded - rs.t_ctx, rs.t_scrubbed - rs.t_loaded, rs.t_read_done - rs.t_scrubbed, rs.t_classified - rs.t_read_done,
              rs.t_printed - rs.t_classified, teardown, now_s() - rs.t_start);
}

void print_statistics(Run &rs) {
    const Options &o = rs.o;
    if (rs.past_int)
        fprintf(stderr, " WARN : a barcode has more than INT_MAX hits: the reference's `int` counters overflow on this input; the exact counts were printed\n");
    logtime();
    if (o.stats) {
        double dt = rs.t_classified - rs.t_loaded;
        stat_line("__stats__ K=%zu set0=%llu set1=%llu reads=%llu bases=%llu barcodes=%zu load_s=%.3f classify_s=%.3f Mbp_per_s=%.1f\n",
                rs.K, (unsigned long long)rs.n_set[0], (unsigned long long)rs.n_set[1], (unsigned long long)rs.total_reads,
                (unsigned long long)rs.total_bases, rs.n_rows, rs.t_loaded - rs.t_start, dt, dt > 0 ? rs.total_bases / dt / 1e6 : 0.0);
    }
    if (o.stats && o.rows_device) stat_rows(rs);
    if (o.stats && rs.naming.device_dict)
        stat_line("__stats_dictionary__ on=device dictionaries=%zu ids_limit=%zu ids_from_device=%zu ids_from_host=%zu merge_by_text_s=%.3f texts_merged_to_host=%zu rows_summed_by_text=%zu\n", rs.naming.groups.size(), rs.naming.host_base, rs.n_dev_names, rs.n_host_names, rs.naming.merge_s,
                  rs.naming.merged_to_host, rs.n_rows_summed);
    if (o.stats) {                                   // the sizes as the library reads them: what a flag with a suffix came to
        const char *nc = sw::text(sw::HAST_NAME_CACHE), *rb = sw::text(sw::HAST_GZ_RING_BYTES), *pg = sw::text(sw::HAST_PARK_GB);
        stat_line("__stats_sizes__ name_cache=%s gz_ring_bytes=%s park_gb=%s\n", nc ? nc : "default", rb ? rb : "default", pg ? pg : "default");
    }
    if (o.stats) stat_line("__stats_setup__ waited_for_stream_setup_s=%.3f (inside scrub_sizes_clone_s: .gz inputs opened, FASTQ streams created while the table was built)\n", rs.t_pre_waited);
    // a context that could not get room for its filter probes the table directly (the round-1 kernel: 1.6 x the HBM requests per read):
    // same results, never silently
    for (size_t i = 0; i < rs.ctxs.size(); i++) {
        char sw[512] = "";
        (void)hast_ctx_options(rs.ctxs[i], sw, sizeof(sw));
        if (strstr(sw, "filter_fallback"))
            fprintf(stderr, " WARN : GPU %d (context %zu) had no room for the k-mer filter and probed the table directly (%s)\n", o.devices[i], i, sw);
    }
    if (o.stats) {
        char sw[512] = "";
        (void)hast_ctx_options(rs.ctx, sw, sizeof(sw));          // measurement switches this context was created with (none by default)
        stat_line("__stats_switches__ %s\n", sw[0] ? sw : "none");
        int f_on = 0, f_m = 0, f_t = 0, f_kp = 0;
        uint64_t f_bytes = 0;
        (void)hast_filter_info(rs.ctx, &f_on, &f_m, &f_t, &f_kp, &f_bytes);
        stat_line("__stats_filter__ mode=%s m=%d t=%d kp=%d bytes=%llu\n", f_on == 2 ? "exact_entries" : f_on == 1 ? "prints" : "off_table_only", f_m, f_t, f_kp,
                  (unsigned long long)f_bytes);
        uint64_t lk = 0, lk_all = 0;                             // HAST_COUNT_LOOKUPS=1 only: windows the filter sent to the exact table
        bool counted = false;
        for (hast_ctx *cx : rs.ctxs)
            if (hast_filter_lookups(cx, &lk) == HAST_OK) { lk_all += lk; counted = true; }
        if (counted) stat_line("__stats_lookups__ windows_sent_to_table=%llu\n", (unsigned long long)lk_all);
    }
    if (rs.hbm_thread.joinable()) {
        rs.hbm_stop = true;
        rs.hbm_thread.join();
        size_t parked = 0;
        (void)hast_dev_mem_info(rs.ctx, nullptr, nullptr, &parked);
        const size_t fm = rs.hbm_free_min.load(), tot = rs.hbm_total.load();
        if (tot) stat_line("__stats_hbm__ total_bytes=%zu free_min_bytes=%zu in_use_peak_bytes=%zu parked_bytes_at_end=%zu\n", tot, fm, tot - std::min(fm, tot), parked);
    }
    fprintf(stderr, "__END__\n");
    rs.t_printed = now_s();
}

// The output is complete.  Unpinning and freeing hundreds of MB of staging memory, the table and the streams takes ~0.1 s that the
// operating system does anyway when the process ends: leave at once (HAST_TEARDOWN=1 runs the destructors, for leak checks) --
// unless a profiler is listening (rocprofv3 preloads its tool library and writes its files when the process ends in an orderly way).
int leave(Run &rs) {
    const Options &o = rs.o;
    if (!sw::flag(sw::HAST_TEARDOWN) && !sw::profiler_listening()) {
        if (o.stats) stat_phases(rs, nullptr);
        if (!o.stats_json.empty() && !write_stats_json(o.stats_json)) fprintf(stderr, "classify: cannot write %s\n", o.stats_json.c_str());
        if (fflush(stdout) != 0) die_output();
        fflush(stderr);
        _exit(0);
    }
    for (std::thread &t : rs.gz_closers) t.join();
    for (hast_fq *f : rs.done_fq) hast_fq_destroy(f);
    hast_rows_destroy(rs.rows);
    for (hast_names *nm : rs.own_caches) hast_names_destroy(nm);
    for (hast_names *nm : rs.own_tabs) hast_names_destroy(nm);       // (after the routing streams that refer to them)
    for (hast_ctx *c : rs.ctxs) hast_ctx_destroy(c);
    if (o.stats) {
        const double teardown_s = now_s() - rs.t_printed;
        stat_phases(rs, &teardown_s);
    }
    if (!o.stats_json.empty() && !write_stats_json(o.stats_json)) fprintf(stderr, "classify: cannot write %s\n", o.stats_json.c_str());
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (!self_test()) {
        fprintf(stderr, "classify: self-test failed\n");
        return 1;
    }
    // 1. options
    Options o;
    if (!parse_options(argc, argv, o)) return -1;
    fprintf(stderr, "__START__\n");
    fprintf(stderr, " use hap0 weight %g\n", o.w0);
    fprintf(stderr, " use hap1 weight %g\n", o.w1);
    logtime();
    const double t_start = now_s();
    Run rs(o);
    rs.t_start = t_start;
    // 2. contexts and dictionaries, with the set-up thread (contexts_ready, as soon as K is known), 3. the table: loaded or built,
    //    scrubbed, cloned to the other GPUs
    find_device_gz_inputs(rs);
    if (!o.load_table.empty()) load_saved_table(rs);
    else if (const int rc = build_table(rs)) return rc;
    scrub_and_clone(rs);
    wait_for_stream_setup(rs);
    logtime();
    rs.t_scrubbed = now_s();
    // 4. read phase
    rs.pool.reset(new hast::WorkerPool(o.t_num));
    rs.caches = std::vector<hast::BarcodeDict::Cache>((size_t)rs.pool->size());
    // (a device dictionary hands out ids below host_base; the first id the host has to give lies there: counters for both from the start,
    // unless --initial-barcodes asks for less, tests)
    flush_counts(rs, o.initial_barcodes == (1u << 24) && rs.naming.device_dict ? rs.naming.host_base + 4096 : o.initial_barcodes);
    if (o.host_parse) read_phase_host(rs);
    else read_phase_device(rs);
    rs.t_read_done = now_s();
    // 5. counters back, device and host names merged, 6. sort and print -- or, with --rows device, all of it where the counters lie
    if (o.rows_device) {
        if (const char *reason = rows_on_device(rs)) {
            rs.rows_fallback = reason;
            fprintf(stderr, " WARN : --rows device: the table is made on the host (fallback=%s)\n", reason);
        }
    }
    if (rs.rows) print_rows_from_device(rs);
    else {
        counters_back(rs);
        sort_rows(rs);
        print_rows(rs);
    }
    // 7. --phase-reads: the lists, then the device router or the host router
    if (o.phase_reads) phase_reads(rs);
    // 8. statistics and leaving
    print_statistics(rs);
    return leave(rs);
}
