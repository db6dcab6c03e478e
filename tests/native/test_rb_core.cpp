// Host driver of the read bins (hast_amd/csrc/rb_core.h through the model of rb_host.h).
//   test_rb_core -c
//       the class rule: "v0 v1 t0 t1" per line on stdin, the class of each on stdout
//   test_rb_core -f fasta|fastq -b BLOCK -t T0,T1 file...
//       reads every file in views the way the feed of rs_api.cpp cuts them -- what the view before left unframed plus up to BLOCK new
//       bytes, the file's end a last view; a view grows as far as a record needs, so no file is refused -- with the votes of its records
//       from <file>.votes (uint32 pairs, in record order, the FASTQ tail's last), and writes the three runs to <file>.bin0 .. .bin2.
//       One status line per file on stdout:  <status> <count0> <count1> <count2> <records> <views> : <file>     status: ok | format_error
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/rb_host.h"

using namespace hast;

static bool slurp(const std::string &path, std::vector<uint8_t> *out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out->clear();
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

static bool run(int format, size_t block, uint32_t t0, uint32_t t1, const char *path) {
    std::vector<uint8_t> data, vraw;
    if (!slurp(path, &data) || !slurp(std::string(path) + ".votes", &vraw)) return false;
    std::vector<uint32_t> votes(vraw.size() / 4);
    if (!votes.empty()) memcpy(votes.data(), vraw.data(), votes.size() * 4);
    rb::Runs runs;
    std::vector<uint8_t> view;                        // [carried bytes | new bytes]
    std::vector<rb::Extent> ext;
    size_t at = 0, rec = 0;
    unsigned long long views = 0;
    bool seen_header = false;
    const char *status = "ok";
    for (bool last = false; !last;) {
        const size_t n_new = data.size() - at < block ? data.size() - at : block;
        last = n_new == 0;
        view.insert(view.end(), data.begin() + (long)at, data.begin() + (long)(at + n_new));
        at += n_new;
        rs::Framed fr;
        rs::frame(format, view.data(), view.size(), last, seen_header, &fr);
        ++views;
        if (fr.flags & RS_FORMAT_ERROR) { status = "format_error"; break; }
        rb::extents(format, view.data(), view.size(), last, &ext);
        if (ext.size() != fr.recs.size() || fr.consumed > view.size()) { status = "model_error"; break; }
        for (const rb::Extent &e : ext)
            if (e.lo >= e.hi || e.hi > fr.consumed) status = "model_error";
        if (2 * (rec + ext.size()) > votes.size()) { status = "votes_short"; break; }
        rb::append_runs(view.data(), ext.data(), votes.data() + 2 * rec, ext.size(), t0, t1, &runs);
        rec += ext.size();
        seen_header = seen_header || fr.headers > 0;
        view.erase(view.begin(), view.begin() + (long)fr.consumed);
        if (last && format == RS_FASTQ) {
            rs::Tail t;
            if (!rs::fq_tail(view.data(), view.size(), &t)) { status = "format_error"; break; }
            if (t.record) {
                if (2 * (rec + 1) > votes.size()) { status = "votes_short"; break; }
                if (!rb::append_tail(view.data(), view.size(), votes.data() + 2 * rec, t0, t1, &runs)) { status = "model_error"; break; }
                ++rec;
            }
        }
    }
    if (strcmp(status, "ok") != 0) runs.clear(), rec = 0;
    for (uint32_t c = 0; c < rb::kClasses; ++c) {
        const std::string out_path = std::string(path) + ".bin" + std::to_string(c);
        FILE *out = fopen(out_path.c_str(), "wb");
        if (!out || fwrite(runs.run[c].data(), 1, runs.run[c].size(), out) != runs.run[c].size() || fclose(out) != 0) return false;
    }
    printf("%s %llu %llu %llu %llu %llu : %s\n", status, (unsigned long long)runs.count[0], (unsigned long long)runs.count[1], (unsigned long long)runs.count[2],
           (unsigned long long)rec, views, path);
    return true;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "-c")) {
        unsigned long long v0, v1, t0, t1;
        while (scanf("%llu %llu %llu %llu", &v0, &v1, &t0, &t1) == 4) printf("%u\n", rb::read_class((uint32_t)v0, (uint32_t)v1, (uint32_t)t0, (uint32_t)t1));
        return 0;
    }
    size_t block = 65536;
    unsigned t0 = 0, t1 = 0;
    int format = -1, i = 1;
    bool have_t = false;
    for (; i + 1 < argc && argv[i][0] == '-'; i += 2) {
        if (!strcmp(argv[i], "-b")) block = (size_t)strtoull(argv[i + 1], nullptr, 10);
        else if (!strcmp(argv[i], "-f")) format = !strcmp(argv[i + 1], "fastq") ? RS_FASTQ : !strcmp(argv[i + 1], "fasta") ? RS_FASTA : -1;
        else if (!strcmp(argv[i], "-t")) have_t = sscanf(argv[i + 1], "%u,%u", &t0, &t1) == 2;
        else break;
    }
    if (format < 0 || block < 1 || !have_t || i >= argc) {
        fprintf(stderr, "usage: test_rb_core -c | -f fasta|fastq -b BLOCK -t T0,T1 file...\n");
        return 2;
    }
    for (; i < argc; ++i)
        if (!run(format, block, t0, t1, argv[i])) {
            fprintf(stderr, "test_rb_core: cannot read %s and its .votes, or write its .bin files\n", argv[i]);
            return 1;
        }
    return 0;
}
