// barcode_freq -- drop-in for the line of HAST's 02.assemble_by_supernova/assemble_by_supernova.sh that writes barcode_freq.txt: how
// many read-1 records carry each barcode.
//   barcode_freq [--count device|host] [--device N | --devices a,b,...] [--inflate device|host|zlib] [--block-mb N]
//                [--max-barcodes N] [--stats] [-t N] READS[.gz] ... > barcode_freq.txt
// The rule is bf_core.h's: of every line 4i + 1 of an input, split at '#' and '/', the second field is the key; one row
// "key \t count \n" per key, rows in byte-wise ascending key order (the script's rows come in awk's hash order, and its one reader
// puts them into a hash).  Every input is numbered on its own; the counts of all inputs are summed.
// --count device (default): the inputs go through the FASTQ streams of include/hast.h in tally mode, fed as classify feeds its passes
// (fq_feed.h: a reader thread per input, blocks submitted ahead; an ordinary .gz is inflated on the GPU, the host inflates what the
// GPU cannot take); keys are counted in a tally per lane on the GPU.  What a block leaves behind -- keys longer than 15 bytes, keys
// that arrive once a tally is full, the partial record at a file's end -- goes into the host model's map (bf_host.h).  At the end the
// tallies and the map are merged by key.  "-" is standard input and always the host model's.
// --count host: no GPU is touched; ingest.h and the host model.
// Exit codes: 0 done; 2 an input that cannot be opened, or is damaged; 3 a failed write; 4 no usable GPU, or a failing GPU call, on
// the device route; 5 the counts do not add up (a defect: nothing is printed); 255 usage.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hast.h"
#include "cli_common.h"
#include "bf_host.h"
#include "fq_feed.h"
#include "ingest.h"

namespace {

struct Options {
    std::vector<std::string> in;
    std::string count = "device", inflate = "device";
    std::vector<int> devices{0};
    size_t block = 16u << 20, max_barcodes = 1u << 24;
    bool block_given = false, stats = false;
    int t_num = 8;
};

struct Stats {
    uint64_t header_lines = 0, on_device = 0, on_host = 0, no_field = 0, distinct = 0, plain_in = 0, blocks = 0;
    int dictionary_full = 0;
    double setup_s = 0, read_s = 0, merge_s = 0, gpu_wait_s = 0;
};

using hast::now_s;
namespace sw = hast::sw;

int usage() {
    fprintf(stderr, "usage: barcode_freq [--count device|host] [--device N | --devices a,b,...] [--inflate device|host|zlib] [--block-mb N]\n"
                    "                    [--max-barcodes N] [--stats] [-t N] READS[.gz] ... > barcode_freq.txt\n");
    return 255;
}

using hast::ends_gz;
using hast::parse_count;

// ---- the host route (and "-" on either route): an input block by block through the model
int count_on_host(const Options &o, const std::string &path, hast::bf::Model &m, Stats &st) {
    hast::BlockSource src;
    if (!src.open(path, o.block, false)) {
        fprintf(stderr, "barcode_freq: cannot open %s\n", path.c_str());
        return 2;
    }
    src.set_readers(std::max(1, std::min(16, o.t_num)));
    std::vector<char> buf(o.block);
    std::string trouble;
    m.begin();
    for (;;) {
        const size_t n = src.read_into(buf.data(), o.block, trouble);
        m.feed(reinterpret_cast<const uint8_t *>(buf.data()), n);
        st.plain_in += n;
        if (!trouble.empty()) {
            fprintf(stderr, "barcode_freq: %s: %s\n", path.c_str(), trouble.c_str());
            return 2;
        }
        if (n < o.block) break;
    }
    m.finish();
    return 0;
}

// ---- the device route
struct Device {
    const Options &o;
    Stats &st;
    hast::bf::Model &model;                      // what the device leaves behind
    std::vector<hast_ctx *> ctxs;
    std::vector<hast_tally *> tallies;           // one per context: a lane of a striped stream, or the one stream's
    hast::FeedWake wake;
    std::vector<std::unique_ptr<hast::FqFeed>> active;
    std::vector<std::string> files;
    size_t next_file = 0;
    bool stripe() const { return ctxs.size() > 1; }
    int buffers() const { return stripe() ? std::max(2, (6 + (int)ctxs.size() - 1) / (int)ctxs.size()) : 6; }
    Device(const Options &oo, Stats &s, hast::bf::Model &m) : o(oo), st(s), model(m) {}
};

int fail_gpu(const char *what) {
    fprintf(stderr, "barcode_freq: %s: %s\n", what, hast_last_error());
    return 4;
}

// an ordinary gzip file goes to the GPU's inflate; BGZF, pipes and what only looks like .gz stay with the host decoders
bool wants_device_inflate(const Options &o, const std::string &path) {
    struct stat sb;
    if (o.inflate != "device" || !ends_gz(path) || stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    unsigned char magic[2] = {0, 0};
    const bool gzip_magic = fread(magic, 1, 2, fp) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    rewind(fp);
    const bool yes = (gzip_magic || sb.st_size == 0) && !hast::BgzfReader::probe(fp);
    fclose(fp);
    return yes;
}

int open_next(Device &d) {
    const std::string &path = d.files[d.next_file];
    std::unique_ptr<hast::FqFeed> f(new hast::FqFeed());
    f->name = path;
    f->file_index = d.next_file++;
    size_t cap = std::max<size_t>(d.o.block, 4096);
    if (wants_device_inflate(d.o, path)) {
        const hast_status gs = d.stripe() ? hast_gz_open_multi(d.ctxs.data(), (int)d.ctxs.size(), path.c_str(), &f->gz) : hast_gz_open(d.ctxs[0], path.c_str(), &f->gz);
        if (gs == HAST_ERR_UNSUPPORTED) f->gz = nullptr;               // (e.g. no room on the device: the host inflates)
        else if (gs != HAST_OK) {
            fprintf(stderr, "barcode_freq: cannot open %s: %s\n", path.c_str(), hast_last_error());
            return 2;
        }
        struct stat sb;
        // (a block costs a dozen small kernels and two round trips: large inflated inputs take larger ones, as in classify)
        if (f->gz && !d.o.block_given && stat(path.c_str(), &sb) == 0 && (uint64_t)sb.st_size >= (1ull << 30)) cap = 64u << 20;
    }
    if (!f->gz) {
        if (!f->src.open(path, cap, false)) {
            fprintf(stderr, "barcode_freq: cannot open %s\n", path.c_str());
            return 2;
        }
        f->src.set_readers(std::max(4, std::min(16, d.o.t_num)));
    }
    const hast_status cs = d.stripe() ? hast_fq_create_striped_ex(d.ctxs.data(), (int)d.ctxs.size(), cap, d.buffers(), nullptr, f->gz ? 1 : 0, &f->fq)
                                      : hast_fq_create_ex(d.ctxs[0], cap, d.buffers(), nullptr, f->gz ? 1 : 0, &f->fq);
    if (cs != HAST_OK) return fail_gpu("creating the FASTQ stream");
    if (hast_fq_set_tally(f->fq, d.tallies.data(), (int)d.tallies.size()) != HAST_OK) return fail_gpu("switching the FASTQ stream to tallying");
    std::string what;
    if (f->start(d.wake, hast_fq_block_bytes(f->fq), d.buffers(), what) != hast::FeedStatus::ok) {
        fprintf(stderr, "barcode_freq: %s\n", what.c_str());
        return 4;
    }
    d.active.push_back(std::move(f));
    return 0;
}

// the oldest submitted block of a feed: what the device counted is in its tally; what it left goes into the map
int tally_block(Device &d, hast::FqFeed &f) {
    hast_fq_tallied b;
    const double t0 = now_s();
    if (hast_fq_next_tallied(f.fq, &b) != HAST_OK) return fail_gpu("tallying a block");
    d.st.gpu_wait_s += now_s() - t0;
    f.opened++;
    d.st.blocks++;
    d.st.header_lines += b.n_records;
    d.st.on_device += b.n_counted;
    d.st.no_field += b.n_nofield;
    if (b.n_left) {
        const uint8_t *bytes = b.bytes;
        if (!bytes && hast_fq_block_host_bytes(f.fq, &bytes) != HAST_OK) return fail_gpu("fetching a block");
        for (uint64_t i = 0; i < b.n_left; ++i) d.model.add_key(bytes + b.left_pos[i], b.left_len[i]);
        d.st.on_host += b.n_left;
    }
    if (b.tail_bytes) d.model.whole(b.tail, (size_t)b.tail_bytes);     // (it starts at a record boundary: line 1 of a stream of its own)
    if (hast_fq_commit(f.fq) != HAST_OK) return fail_gpu("releasing a block");
    f.held--;
    return 0;
}

void retire(hast::FqFeed &f) {
    f.stop_reader();
    if (f.gz) hast_gz_close(f.gz);
    f.gz = nullptr;
    hast_fq_destroy(f.fq);
    f.fq = nullptr;
}

int run_device(Device &d) {
    const size_t max_active = d.stripe() ? 1 : 2;
    int rc = 0;
    while (!rc && d.next_file < d.files.size() && d.active.size() < max_active) rc = open_next(d);
    while (!rc && !d.active.empty()) {
        bool progress = false;
        for (std::unique_ptr<hast::FqFeed> &f : d.active) {
            hast::FeedStatus fs = hast::FeedStatus::ok;
            std::string what;
            if (f->pump(fs, what)) progress = true;
            if (fs != hast::FeedStatus::ok) {
                fprintf(stderr, "barcode_freq: %s%s%s\n", what.c_str(), fs == hast::FeedStatus::library_failed ? ": " : "", fs == hast::FeedStatus::library_failed ? hast_last_error() : "");
                rc = fs == hast::FeedStatus::input_failed ? 2 : 4;
                break;
            }
        }
        for (size_t fi = 0; !rc && fi < d.active.size();) {
            hast::FqFeed &f = *d.active[fi];
            if (f.block_ready()) {
                rc = tally_block(d, f);
                progress = true;
                if (rc) break;
            }
            if (f.drained()) {
                retire(f);
                d.active.erase(d.active.begin() + (long)fi);
                if (d.next_file < d.files.size()) rc = open_next(d);
                progress = true;
                continue;
            }
            ++fi;
        }
        if (!rc && !progress) d.wake.wait(d.stripe() ? 10 : 100);
    }
    for (std::unique_ptr<hast::FqFeed> &f : d.active) retire(*f);      // (after a failure)
    d.active.clear();
    return rc;
}

// every tally's keys and counts behind the rows
int read_tallies(Device &d, hast::bf::Rows &rows) {
    std::vector<uint8_t> text;
    std::vector<uint64_t> counts;
    for (hast_tally *t : d.tallies) {
        size_t n = 0;
        if (hast_tally_size(t, &n) != HAST_OK) return fail_gpu("reading a tally");
        if (n >= hast_tally_limit(t)) d.st.dictionary_full = 1;
        const size_t piece = 1u << 20;
        for (size_t at = 0; at < n; at += piece) {
            const size_t m = std::min(piece, n - at);
            text.resize(16 * m);
            counts.resize(m);
            if (hast_tally_read(t, at, m, text.data(), counts.data()) != HAST_OK) return fail_gpu("reading a tally");
            for (size_t i = 0; i < m; ++i) {
                const uint8_t *r = text.data() + 16 * i;
                if (r[0] > hast::bf::kMaxText) {
                    fprintf(stderr, "barcode_freq: a tally holds a text record of length %u\n", r[0]);
                    return 5;
                }
                rows.emplace_back(std::string(reinterpret_cast<const char *>(r + 1), r[0]), counts[i]);
            }
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto value = [&]() -> const char * { return i + 1 < argc ? argv[++i] : nullptr; };
        uint64_t v = 0;
        if (a == "--count") { const char *x = value(); if (!x || (strcmp(x, "host") && strcmp(x, "device"))) return usage(); o.count = x; }
        else if (a == "--inflate") { const char *x = value(); if (!x || (strcmp(x, "host") && strcmp(x, "device") && strcmp(x, "zlib"))) return usage(); o.inflate = x; }
        else if (a == "--device") { if (!parse_count(value(), &v) || v > 1023) return usage(); o.devices.assign(1, (int)v); }
        else if (a == "--devices") {
            const char *x = value();
            if (!x) return usage();
            o.devices.clear();
            for (const char *p = x; *p;) {
                char *end = nullptr;
                const long g = strtol(p, &end, 10);
                if (end == p || g < 0 || g > 1023 || (*end && *end != ',')) return usage();
                o.devices.push_back((int)g);
                p = *end ? end + 1 : end;
            }
            if (o.devices.empty() || o.devices.size() > 16) return usage();
        }
        else if (a == "--block-mb") { if (!parse_count(value(), &v) || v < 1 || v > 1024) return usage(); o.block = (size_t)v << 20; o.block_given = true; }
        else if (a == "--max-barcodes") { if (!parse_count(value(), &v) || v < 1 || v > (1ull << 30)) return usage(); o.max_barcodes = (size_t)v; }
        else if (a == "--stats") o.stats = true;
        else if (a == "-t") { if (!parse_count(value(), &v) || v < 1 || v > 1024) return usage(); o.t_num = (int)v; }
        else if (a.size() > 1 && a[0] == '-') return usage();
        else o.in.push_back(a);
    }
    if (o.in.empty()) return usage();
    if (!o.block_given) o.block_given = sw::size(sw::HAST_BF_BLOCK, &o.block);            // tests: blocks of a few hundred bytes
    if (o.inflate == "zlib") setenv("HAST_INFLATE", "zlib", 1);

    const double t_start = now_s();
    Stats st;
    hast::bf::Model model;
    hast::bf::Rows rows;
    int rc = 0;
    if (o.count == "host") {
        const double t0 = now_s();
        for (size_t i = 0; i < o.in.size() && !rc; ++i) rc = count_on_host(o, o.in[i], model, st);
        st.read_s = now_s() - t0;
    } else {
        Device d(o, st, model);
        for (const std::string &p : o.in)
            if (p != "-") d.files.push_back(p);
        const double t0 = now_s();
        if (!d.files.empty()) {
            for (size_t i = 0; i < o.devices.size() && !rc; ++i) {
                hast_ctx *c = nullptr;
                hast_tally *t = nullptr;
                if (hast_ctx_create(o.devices[i], 21, &c) != HAST_OK) { rc = fail_gpu("no usable GPU"); break; }
                d.ctxs.push_back(c);
                if (hast_tally_create(c, o.max_barcodes, &t) != HAST_OK) { rc = fail_gpu("creating a tally"); break; }
                d.tallies.push_back(t);
            }
        }
        st.setup_s = now_s() - t0;
        const double t1 = now_s();
        if (!rc && !d.files.empty()) rc = run_device(d);
        for (size_t i = 0; i < o.in.size() && !rc; ++i)
            if (o.in[i] == "-") rc = count_on_host(o, o.in[i], model, st);
        st.read_s = now_s() - t1;
        const double t2 = now_s();
        if (!rc) rc = read_tallies(d, rows);
        st.merge_s = now_s() - t2;
        for (hast_tally *t : d.tallies) hast_tally_destroy(t);
        for (hast_ctx *c : d.ctxs) hast_ctx_destroy(c);
    }
    if (rc) return rc;
    const double t2 = now_s();
    for (auto &kv : model.counts) rows.emplace_back(kv.first, kv.second);
    hast::bf::merge_rows(rows);
    st.header_lines += model.header_lines;
    st.on_host += model.counted;
    st.no_field += model.no_field;
    st.distinct = rows.size();
    uint64_t sum = 0;
    for (const auto &r : rows) sum += r.second;
    if (st.on_device + st.on_host + st.no_field != st.header_lines || sum != st.on_device + st.on_host) {
        fprintf(stderr, "barcode_freq: the counts do not add up: %llu on the device + %llu on the host + %llu without a field, %llu header lines, rows sum to %llu\n",
                (unsigned long long)st.on_device, (unsigned long long)st.on_host, (unsigned long long)st.no_field, (unsigned long long)st.header_lines, (unsigned long long)sum);
        return 5;
    }
    std::string out;
    hast::bf::print_rows(rows, out);
    st.merge_s += now_s() - t2;
    if ((out.size() && fwrite(out.data(), 1, out.size(), stdout) != out.size()) || fflush(stdout) != 0) {
        fprintf(stderr, "barcode_freq: cannot write the rows\n");
        return 3;
    }
    if (o.stats) {
        fprintf(stderr, "[stats] tally %s: header_lines=%llu counted_on_device=%llu counted_on_host=%llu no_field=%llu distinct=%llu dictionary_full=%d\n", o.count.c_str(),
                (unsigned long long)st.header_lines, (unsigned long long)st.on_device, (unsigned long long)st.on_host, (unsigned long long)st.no_field,
                (unsigned long long)st.distinct, st.dictionary_full);
        fprintf(stderr, "[stats] seconds: setup=%.3f read_phase=%.3f gpu_wait=%.3f merge=%.3f total=%.3f blocks=%llu plain_in_bytes=%llu\n", st.setup_s, st.read_s, st.gpu_wait_s,
                st.merge_s, now_s() - t_start, (unsigned long long)st.blocks, (unsigned long long)st.plain_in);
    }
    return 0;
}
