// cli_common.h -- what the programs (classify, classify_read, unshared_kmers, fake_10x, barcode_freq) would each write again.  Host only.
// Nothing here ends the process: a caller gets a status and calls its own die().
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hast.h"
#include "switches.h"

namespace hast {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the whole input, front to back (also from a pipe, which has no size to ask for)
inline bool slurp(const std::string &path, std::vector<char> &out) {
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

// the name says gzip: it ends in ".gz" behind at least `stem` other bytes (1: a file called just ".gz" is none, as for BlockSource;
// 0: stage 00's script looks at the last three bytes alone, s00:169)
inline bool ends_gz(const std::string &s, size_t stem = 1) { return s.size() >= 3 + stem && s.compare(s.size() - 3, 3, ".gz") == 0; }

// (parse_count, the grammar of a count or a size on the command line, is switches.h's: the environment takes the same)

// --devices A,B,...: non-negative numbers with commas between them, appended to out; false: not such a list
inline bool parse_device_list(const char *text, std::vector<int> &out) {
    for (const char *q = text; *q;) {
        char *end;
        const long v = strtol(q, &end, 10);
        if (end == q || v < 0 || (*end && *end != ',')) return false;
        out.push_back((int)v);
        q = *end == ',' ? end + 1 : end;
    }
    return true;
}

// ---- the two k-mer files of classify and classify_read into the table (classify.cpp:30-46, s03:51-70) ----
// K = length of the first line of the first file; a regular file is streamed into the table by the library, anything else is read into
// memory first (a pipe can be read only once: it is read whole in open() and its first bytes serve as the head).  Between open() and
// insert() the caller looks at K, creates the context and reserves capacity() keys.  Both return 0 or the exit status the two programs
// share, with *msg -- left empty where the words are the caller's (status 3: the library found a line that is no K-mer).
struct KmerFiles {
    std::string path[2];
    std::vector<char> txt[2], head;              // txt: a file that is not streamed; head: the first 4096 bytes of file 0
    bool streamed[2] = {false, false}, head_has_newline = false;
    size_t text_bytes[2] = {0, 0}, K = 0;

    int open(const std::string &hap0, const std::string &hap1, std::string *msg) {
        path[0] = hap0;
        path[1] = hap1;
        for (int h = 0; h < 2; h++) {
            struct stat sb;
            streamed[h] = stat(path[h].c_str(), &sb) == 0 && S_ISREG(sb.st_mode);
            if (!streamed[h] && !slurp(path[h], txt[h])) return *msg = "cannot read " + path[h], 2;
            text_bytes[h] = streamed[h] ? (size_t)sb.st_size : txt[h].size();
        }
        if (streamed[0]) {
            FILE *f = fopen(path[0].c_str(), "rb");
            if (!f) return *msg = "cannot read " + path[0], 2;
            head.resize(4096);
            head.resize(fread(head.data(), 1, head.size(), f));
            fclose(f);
        } else head.assign(txt[0].begin(), txt[0].begin() + (long)std::min<size_t>(txt[0].size(), 4096));
        const void *nl0 = memchr(head.data(), '\n', head.size());
        head_has_newline = nl0 != nullptr;
        K = nl0 ? (size_t)((const char *)nl0 - head.data()) : head.size();
        return 0;
    }
    size_t capacity() const { return text_bytes[0] / (K + 1) + text_bytes[1] / (K + 1) + 2; }
    // File h into the table as haplotype h, *lines: the k-mers it gave; its memory is let go.  complete_lines_only: a trailing piece
    // without '\n' of a file read into memory is dropped (s03:63).  A lone unterminated first line of file 0 is a k-mer all the same
    // (classify.cpp:35-39); check_lone_line: only if it is A/C/G/T.
    int insert(hast_ctx *ctx, int h, bool complete_lines_only, bool check_lone_line, uint64_t *lines, std::string *msg) {
        size_t usable = txt[h].size();
        while (complete_lines_only && usable && txt[h][usable - 1] != '\n') usable--;
        const hast_status st = streamed[h] ? hast_table_insert_text_file(ctx, h, path[h].c_str(), lines) : hast_table_insert_text(ctx, h, txt[h].data(), usable, lines);
        if (st == HAST_ERR_FORMAT) return 3;
        if (st == HAST_ERR_IO) return *msg = "cannot read " + path[h], 2;
        if (st != HAST_OK) return *msg = "building the k-mer table", 4;
        if (h == 0 && !head_has_newline && text_bytes[0] == K) {
            for (size_t i = 0; check_lone_line && i < K; i++)
                if (!strchr("ACGT", head[i])) return *msg = "k-mer files must hold upper-case A/C/G/T lines only", 3;
            const uint64_t key = hast_canon_kmer(head.data(), (int)K);
            if (hast_table_insert_keys(ctx, 0, &key, 1) != HAST_OK) return *msg = "building the k-mer table", 4;
            *lines = 1;
        }
        std::vector<char>().swap(txt[h]);
        return 0;
    }
};

}  // namespace hast
