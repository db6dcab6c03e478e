// Host driver of the read-stream rules (hast_amd/csrc/rs_core.h through the model of rs_host.h): reads every file in blocks of -b
// bytes the way the feed of rs_api.cpp does -- a view is what the view before left unframed plus up to one block of new bytes, the
// file's end is a last view -- and writes "name \t sequence \n" per record to <file>.rs.  One status line per file on stdout:
//   <status> <records> <bases> <bytes> <views>      status: ok | format_error | too_long
//   usage: test_rs_core -f fasta|fastq -b BLOCK file...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/rs_host.h"

using namespace hast;

static bool run(int format, size_t block, const char *path) {
    FILE *in = fopen(path, "rb");
    if (!in) return false;
    const std::string out_path = std::string(path) + ".rs";
    std::string rows;
    std::vector<uint8_t> view(2 * block);             // [carried bytes | new bytes], the new bytes at offset `block`
    size_t tail = 0;
    unsigned long long records = 0, bases = 0, bytes = 0, views = 0;
    bool seen_header = false;
    const char *status = "ok";
    for (bool last = false; !last;) {
        const size_t n_new = fread(view.data() + block, 1, block, in);
        last = n_new == 0;
        bytes += n_new;
        const uint8_t *v = view.data() + block - tail;
        const size_t n = tail + n_new;
        rs::Framed fr;
        rs::frame(format, v, n, last, seen_header, &fr);
        ++views;
        if (fr.flags & RS_FORMAT_ERROR) { status = "format_error"; break; }
        if (fr.consumed > n) { status = "model_error"; break; }
        const size_t left = n - (size_t)fr.consumed;
        if (left > block) { status = "too_long"; break; }
        for (const rs::Record &r : fr.recs) {
            rows.append(reinterpret_cast<const char *>(v) + r.name_pos, r.name_len);
            rows += '\t';
            rows += r.seq;
            rows += '\n';
        }
        records += fr.recs.size();
        bases += fr.bases;
        seen_header = seen_header || fr.headers > 0;
        if (last && format == RS_FASTQ) {
            rs::Tail t;
            if (!rs::fq_tail(v + fr.consumed, left, &t)) { status = "format_error"; break; }
            if (t.record) {
                rows += t.name + '\t' + t.seq + '\n';
                ++records;
                bases += t.seq.size();
            }
        }
        std::vector<uint8_t> keep(v + fr.consumed, v + n);       // (the feed copies into the other buffer: no overlap there)
        if (left) memcpy(view.data() + block - left, keep.data(), left);
        tail = left;
    }
    fclose(in);
    if (strcmp(status, "ok") != 0) rows.clear(), records = bases = 0;
    FILE *out = fopen(out_path.c_str(), "wb");
    if (!out || fwrite(rows.data(), 1, rows.size(), out) != rows.size() || fclose(out) != 0) return false;
    printf("%s %llu %llu %llu %llu : %s\n", status, records, bases, bytes, views, path);
    return true;
}

int main(int argc, char **argv) {
    size_t block = 65536;
    int format = -1, i = 1;
    for (; i + 1 < argc && argv[i][0] == '-'; i += 2) {
        if (!strcmp(argv[i], "-b")) block = (size_t)strtoull(argv[i + 1], nullptr, 10);
        else if (!strcmp(argv[i], "-f")) format = !strcmp(argv[i + 1], "fastq") ? RS_FASTQ : !strcmp(argv[i + 1], "fasta") ? RS_FASTA : -1;
        else break;
    }
    if (format < 0 || block < 64 || i >= argc) {
        fprintf(stderr, "usage: test_rs_core -f fasta|fastq -b BLOCK file...\n");
        return 2;
    }
    for (; i < argc; ++i)
        if (!run(format, block, argv[i])) {
            fprintf(stderr, "test_rs_core: cannot read %s or write its .rs\n", argv[i]);
            return 1;
        }
    return 0;
}
