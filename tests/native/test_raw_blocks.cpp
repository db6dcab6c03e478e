// Host-only test of hast::RawBlocks (hast_amd/csrc/raw_blocks.h; no GPU, no libhast.so): one input's raw bytes, a feed's block at a
// time, by its three routes, against a fake hast_gz in ordinary memory.  Built with -fsanitize=address,undefined by
// tests/test_raw_blocks_cpu.py.
//   test_raw_blocks SCRATCH_DIR        (an empty directory for the input files)
// Inputs: a plain file and its .gz (made with zlib) of 0 bytes, exactly two blocks, two blocks + 1 byte; the block is 4096 bytes.
// Held: every byte is delivered once and in order; the sizes of the reads (full blocks, the short one, then nothing -- and on the
// device route exactly what the decoder gave: a short read does not end the stream, only an empty one does); the kind open() settles on
// (a decoder that refuses the file leaves it to the host decoders); one hast_gz_close per hast_gz_open, and none before close().
#include <unistd.h>
#include <zlib.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/raw_blocks.h"

namespace {

constexpr size_t kBlock = 4096;

[[noreturn]] void fail(const std::string &what) {
    fprintf(stderr, "test_raw_blocks: %s\n", what.c_str());
    fflush(stderr);
    _exit(1);                                      // (a reader thread may be at work: no destructors)
}

std::string pattern(size_t n, unsigned seed) {
    std::string s(n, '\0');
    uint32_t x = 2463534242u + seed;
    for (size_t i = 0; i < n; i++) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        s[i] = i % 61 == 60 ? '\n' : (char)('A' + x % 26);
    }
    return s;
}

std::string g_last_error;
bool g_refuse_open = false;                        // hast_gz_open: "not for the GPU"
std::vector<size_t> g_short_reads;                 // hast_gz_read_device: the sizes of the first reads, then whole blocks
int g_opened = 0, g_closed = 0;

}  // namespace

// ---- the fake decoder: what raw_blocks.h calls of include/hast.h; "device" blocks are ordinary memory ----
struct hast_gz {
    std::string data;
    size_t pos = 0, calls = 0;
};
struct hast_ctx {};

extern "C" {
const char *hast_last_error(void) { return g_last_error.c_str(); }
hast_status hast_gz_open(hast_ctx *, const char *path, hast_gz **out) {
    if (g_refuse_open) return HAST_ERR_UNSUPPORTED;
    gzFile f = gzopen(path, "rb");
    if (!f) return HAST_ERR_IO;
    hast_gz *z = new hast_gz();
    char buf[1 << 15];
    for (int n; (n = gzread(f, buf, sizeof buf)) > 0;) z->data.append(buf, (size_t)n);
    gzclose(f);
    *out = z;
    g_opened++;
    return HAST_OK;
}
hast_status hast_gz_read_device(hast_gz *z, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream) {
    size_t n = std::min(cap, z->data.size() - z->pos);
    if (z->calls < g_short_reads.size()) n = std::min(n, g_short_reads[z->calls]);
    z->calls++;
    if (n) memcpy(d_dst, z->data.data() + z->pos, n);
    z->pos += n;
    *n_out = n;
    return HAST_OK;
}
void hast_gz_close(hast_gz *z) {
    g_closed++;
    delete z;
}
}

namespace {

std::string write_file(const std::string &dir, const std::string &name, const std::string &bytes, bool gz) {
    const std::string path = dir + "/" + name;
    if (gz) {
        gzFile f = gzopen(path.c_str(), "wb");
        if (!f || (!bytes.empty() && gzwrite(f, bytes.data(), (unsigned)bytes.size()) != (int)bytes.size()) || gzclose(f) != Z_OK) fail("cannot write " + path);
    } else {
        FILE *f = fopen(path.c_str(), "wb");
        if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) fail("cannot write " + path);
    }
    return path;
}

// the file through RawBlocks, the way the programs' loops read it: until a read gives nothing; returns the reads' sizes
std::vector<size_t> read_all(const std::string &path, bool gz, hast_ctx *ctx, hast::RawBlocks::Kind want_kind, const std::string &expect) {
    hast::RawBlocks raw;
    std::string err, got_bytes;
    const int closed_before = g_closed;
    if (!raw.open(path, gz, ctx, kBlock, &err)) fail("open: " + err);
    if (raw.kind() != want_kind) fail(path + ": kind " + std::to_string(raw.kind()) + ", not " + std::to_string(want_kind));
    std::vector<uint8_t> block(kBlock);                  // (exactly a block: a read past it is the sanitizer's to find)
    std::vector<size_t> sizes;
    for (;;) {
        size_t got = ~(size_t)0;
        if (!(raw.kind() == hast::RawBlocks::gz_on_device ? raw.read_device(block.data(), nullptr, &got) : raw.read_host(block.data(), &got, &err))) fail(path + ": read: " + err);
        if (got > kBlock) fail(path + ": a read larger than a block");
        sizes.push_back(got);
        if (got == 0) break;
        got_bytes.append(reinterpret_cast<const char *>(block.data()), got);
    }
    if (got_bytes != expect) fail(path + ": the bytes differ (" + std::to_string(got_bytes.size()) + " of " + std::to_string(expect.size()) + ")");
    if (g_closed != closed_before) fail(path + ": the decoder was closed before close()");
    raw.close();
    if (g_closed != closed_before + (want_kind == hast::RawBlocks::gz_on_device)) fail(path + ": hast_gz_close calls");
    if (raw.kind() != hast::RawBlocks::closed) fail(path + ": not closed");
    return sizes;
}

void expect_sizes(const std::string &what, const std::vector<size_t> &got, const std::vector<size_t> &want) {
    if (got == want) return;
    std::string s;
    for (size_t x : got) s += " " + std::to_string(x);
    fail(what + ": the reads' sizes are" + s);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) fail("usage: test_raw_blocks SCRATCH_DIR");
    const std::string dir = argv[1];
    hast_ctx ctx;
    using K = hast::RawBlocks;
    size_t cases = 0;
    std::string packed;
    const size_t sizes[3] = {0, 2 * kBlock, 2 * kBlock + 1};
    for (size_t si = 0; si < 3; si++) {
        const size_t n = sizes[si];
        const std::string bytes = pattern(n, (unsigned)si), tag = std::to_string(n);
        const std::string plain = write_file(dir, "in" + tag + ".fq", bytes, false), gz = write_file(dir, "in" + tag + ".fq.gz", bytes, true);
        std::vector<size_t> whole;                                  // full blocks, the short one, nothing
        for (size_t at = 0; at < n; at += kBlock) whole.push_back(std::min(kBlock, n - at));
        whole.push_back(0);
        expect_sizes("plain " + tag, read_all(plain, false, &ctx, K::plain, bytes), whole), cases++;
        g_refuse_open = false;
        g_short_reads.clear();
        expect_sizes("device " + tag, read_all(gz, true, &ctx, K::gz_on_device, bytes), whole), cases++;
        expect_sizes("host gz " + tag, read_all(gz, true, nullptr, K::gz_on_host, bytes), whole), cases++;
        g_refuse_open = true;
        expect_sizes("refused " + tag, read_all(gz, true, &ctx, K::gz_on_host, bytes), whole), cases++;
        g_refuse_open = false;
        if (n) {                                                     // short device reads: got < block, followed by more, then 0
            g_short_reads = {100, 1, kBlock - 1};
            std::vector<size_t> want = {100, 1, kBlock - 1};
            for (size_t at = kBlock + 100; at < n; at += kBlock) want.push_back(std::min(kBlock, n - at));
            want.push_back(0);
            expect_sizes("short device reads " + tag, read_all(gz, true, &ctx, K::gz_on_device, bytes), want), cases++;
            g_short_reads.clear();
        }
        // the caller's rule decides what is gzip, not the name: the .gz file's own bytes
        packed.clear();
        FILE *f = fopen(gz.c_str(), "rb");
        char buf[4096];
        for (size_t k; f && (k = fread(buf, 1, sizeof buf, f)) > 0;) packed.append(buf, k);
        if (!f || fclose(f) != 0) fail("cannot read " + gz);
        (void)read_all(gz, false, &ctx, K::plain, packed), cases++;
    }
    if (g_opened != g_closed || g_opened == 0) fail("hast_gz_open and hast_gz_close calls differ");
    hast::RawBlocks raw;
    std::string err;
    if (raw.open(dir + "/missing.fq", false, &ctx, kBlock, &err) || err != "cannot open " + dir + "/missing.fq") fail("a missing plain file");
    g_refuse_open = true;
    if (raw.open(dir + "/missing.fq.gz", true, &ctx, kBlock, &err) || err != "cannot open " + dir + "/missing.fq.gz") fail("a missing gz file");
    // a gzip file cut short: the host decoders' error, in their words
    const std::string junk = write_file(dir, "cut.fq.gz", packed.substr(0, packed.size() / 2), false);
    if (!raw.open(junk, true, nullptr, kBlock, &err)) fail("open: " + err);
    std::vector<uint8_t> block(kBlock);
    size_t got = 0;
    err.clear();
    while (raw.read_host(block.data(), &got, &err) && got) {}
    if (err.empty()) fail("a damaged gz input read to its end without a word");
    printf("ok cases=%zu\n", cases);
    return 0;
}
