// Host-only test of hast::KmerFiles (hast_amd/csrc/cli_common.h; no GPU, no libhast.so): the head logic of loading the two k-mer files
// of classify and classify_read, against a fake table that records what it is handed.  Built with -fsanitize=address,undefined by
// tests/test_block_work_cpu.py.
//   test_kmer_files SCRATCH_DIR        (an empty directory for the input files)
// Held: K is the length of the first line of the first file, or of the whole head where that holds no newline; regular files are
// streamed, a pipe is read into memory and handed over whole or, with complete_lines_only, without its trailing piece; a lone
// unterminated first line (text_bytes == K) is inserted as a key, after the A/C/G/T check where that is on; the statuses and messages.
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "../../hast_amd/csrc/cli_common.h"

namespace {

[[noreturn]] void fail(const std::string &what) {
    fprintf(stderr, "test_kmer_files: %s\n", what.c_str());
    fflush(stderr);
    _exit(1);
}

struct Call { std::string what; int hap; std::string arg; };
std::vector<Call> g_calls;
hast_status g_status = HAST_OK;                     // what the fake text inserts answer

}  // namespace

struct hast_ctx {};

extern "C" {
const char *hast_last_error(void) { return "the fake table's word"; }
uint64_t hast_canon_kmer(const char *s, int k) { return 1000u + (uint64_t)k * 16 + (uint64_t)(s[0] & 15); }
hast_status hast_table_insert_text(hast_ctx *, int hap, const char *text, size_t nbytes, uint64_t *lines_out) {
    g_calls.push_back({"text", hap, std::string(text, nbytes)});
    *lines_out = 7;
    return g_status;
}
hast_status hast_table_insert_text_file(hast_ctx *, int hap, const char *path, uint64_t *lines_out) {
    g_calls.push_back({"file", hap, path});
    *lines_out = 9;
    return g_status;
}
hast_status hast_table_insert_keys(hast_ctx *, int hap, const uint64_t *canon_keys, size_t n) {
    g_calls.push_back({"keys", hap, std::to_string(n) + ":" + std::to_string(canon_keys[0])});
    return HAST_OK;
}
}

namespace {

std::string g_dir;
int g_pipes = 0;

std::string regular(const std::string &name, const std::string &bytes) {
    const std::string path = g_dir + "/" + name;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) fail("cannot write " + path);
    return path;
}

// open() + insert() of both files; file 0 through a pipe if asked.  Returns the first non-zero status (0: none)
struct Loaded {
    hast::KmerFiles kf;
    int code = 0;
    std::string msg;
    uint64_t lines[2] = {0, 0};
};
void load(Loaded &L, const std::string &text0, bool pipe0, bool complete_lines_only, bool check_lone_line) {
    g_calls.clear();
    std::string p0;
    std::thread writer;
    if (pipe0) {
        p0 = g_dir + "/pipe" + std::to_string(g_pipes++);
        if (mkfifo(p0.c_str(), 0600) != 0) fail("mkfifo");
        writer = std::thread([p0, text0] {
            FILE *f = fopen(p0.c_str(), "wb");
            if (!f || fwrite(text0.data(), 1, text0.size(), f) != text0.size() || fclose(f) != 0) fail("cannot write the pipe");
        });
    } else p0 = regular("hap0_" + std::to_string(g_pipes++) + ".mer", text0);
    const std::string p1 = regular("hap1.mer", "TTTTT\nGGGGG\n");
    hast_ctx ctx;
    L.code = L.kf.open(p0, p1, &L.msg);
    if (writer.joinable()) writer.join();
    for (int h = 0; h < 2 && !L.code; h++) L.code = L.kf.insert(&ctx, h, complete_lines_only, check_lone_line, &L.lines[h], &L.msg);
}

void expect(bool ok, const std::string &what) {
    if (!ok) fail(what);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) fail("usage: test_kmer_files SCRATCH_DIR");
    g_dir = argv[1];
    size_t cases = 0;
    {   // K from the first line; regular files are streamed; capacity from the sizes
        Loaded L;
        load(L, "ACGTA\nCCCCC\n", false, true, true);
        expect(L.code == 0 && L.kf.K == 5 && L.kf.head_has_newline && L.kf.streamed[0] && L.kf.streamed[1], "K from the first line");
        expect(L.kf.capacity() == 12 / 6 + 12 / 6 + 2, "capacity");
        expect(g_calls.size() == 2 && g_calls[0].what == "file" && g_calls[0].hap == 0 && g_calls[1].what == "file" && g_calls[1].hap == 1, "two streamed files");
        expect(L.lines[0] == 9 && L.lines[1] == 9, "lines of streamed files");
        cases++;
    }
    {   // a head without a newline: K is all of it, and 4096 of a longer one
        Loaded L;
        load(L, std::string(5000, 'A'), false, true, true);
        expect(L.code == 0 && L.kf.K == 4096 && !L.kf.head_has_newline && L.kf.head.size() == 4096, "a full head without a newline");
        expect(g_calls.size() == 2, "no lone line when the file is longer than K");
        cases++;
    }
    {   // the lone unterminated line: text_bytes == K
        Loaded L;
        load(L, "ACGTA", false, true, true);
        expect(L.code == 0 && L.kf.K == 5 && L.lines[0] == 1, "a lone line is one k-mer");
        expect(g_calls.size() == 3 && g_calls[1].what == "keys" && g_calls[1].hap == 0 && g_calls[1].arg == "1:" + std::to_string(hast_canon_kmer("ACGTA", 5)), "a lone line's key");
        cases++;
    }
    {   // ... checked for A/C/G/T where that is on
        Loaded L;
        load(L, "ACGXA", false, true, true);
        expect(L.code == 3 && L.msg == "k-mer files must hold upper-case A/C/G/T lines only" && g_calls.size() == 1, "a lone line that is no k-mer");
        Loaded M;
        load(M, "ACGXA", false, false, false);
        expect(M.code == 0 && M.lines[0] == 1 && g_calls.size() == 3, "a lone line, unchecked");
        cases += 2;
    }
    for (int trim = 0; trim < 2; trim++) {   // a pipe is read into memory; the trailing piece stays or goes
        Loaded L;
        load(L, "ACGTA\nCCCCC\nGG", true, trim != 0, true);
        expect(L.code == 0 && L.kf.K == 5 && !L.kf.streamed[0] && L.kf.text_bytes[0] == 14, "a pipe's K and size");
        expect(g_calls.size() == 2 && g_calls[0].what == "text" && g_calls[0].arg == (trim ? "ACGTA\nCCCCC\n" : "ACGTA\nCCCCC\nGG"), "the trailing piece");
        expect(L.lines[0] == 7 && L.kf.txt[0].empty(), "a pipe's lines, its memory let go");
        cases++;
    }
    {   // a lone line through a pipe: nothing complete to insert as text, the key all the same
        Loaded L;
        load(L, "ACGTA", true, true, true);
        expect(L.code == 0 && g_calls.size() == 3 && g_calls[0].what == "text" && g_calls[0].arg.empty() && g_calls[1].what == "keys" && L.lines[0] == 1, "a lone line through a pipe");
        cases++;
    }
    {   // what cannot be read, and the library's statuses
        hast::KmerFiles kf;
        std::string msg;
        expect(kf.open(g_dir + "/missing.mer", g_dir + "/hap1.mer", &msg) == 2 && msg == "cannot read " + g_dir + "/missing.mer", "a missing file");
        const hast_status st[3] = {HAST_ERR_FORMAT, HAST_ERR_IO, HAST_ERR_HIP};
        const int code[3] = {3, 2, 4};
        for (int i = 0; i < 3; i++) {
            Loaded L;
            g_status = st[i];
            load(L, "ACGTA\n", false, true, true);
            g_status = HAST_OK;
            expect(L.code == code[i] && g_calls.size() == 1, "a status of the library's");
            expect(i == 0 ? L.msg.empty() : i == 1 ? L.msg == "cannot read " + L.kf.path[0] : L.msg == "building the k-mer table", "its message");
            cases++;
        }
        cases++;
    }
    printf("ok cases=%zu\n", cases);
    return 0;
}
