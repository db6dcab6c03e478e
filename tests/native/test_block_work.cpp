// Host-only test of hast::BlockWork (hast_amd/csrc/ingest.h): the work area of the host parsers -- the carry in front of the next
// block, the newline index, the cut at `consumed` -- against a serial model: concatenate, scan for '\n', cut.  Built with
// -fsanitize=address,undefined by tests/test_block_work_cpu.py.
//   test_block_work SCRATCH_DIR        (an empty directory for the input files)
// The text: about 3 MB of random lines of 0..300 bytes with runs of empty lines and one line of 10000 bytes (a 4096-byte block without
// a newline).  Blocks of 4096 bytes and of 1 MiB read all of it, and `consumed` is chosen so that the carry goes through 0, 1,
// kFrontPad - 1, kFrontPad, kFrontPad + 1 (the slow path) and back to 0, then through random sizes (the text is four blocks of 1 MiB:
// there the carry goes through kFrontPad, kFrontPad + 1 and 0).  Blocks of 1 and 7 bytes read its
// first 20000 bytes with carries of 0, 1, 2, 5, 300 and 0: a carry of kFrontPad would take a million blocks to build there, each copied
// again by every keep(), and the paths it takes do not depend on the block size.  Every case runs with 1 and with 3 workers (areas of 0,
// 1 and 2 bytes are shorter than that), and with an input whose final area -- the carry alone -- is empty and one whose is not.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/ingest.h"

namespace {

[[noreturn]] void fail(const std::string &what) {
    fprintf(stderr, "test_block_work: %s\n", what.c_str());
    fflush(stderr);
    _exit(1);                                      // (a reader thread may be at work: no destructors)
}

uint32_t g_x = 2463534242u;
uint32_t rnd() {
    g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5;
    return g_x;
}

std::string make_text(size_t about) {
    std::string s;
    while (s.size() < about) {
        if (rnd() % 50 == 0)
            s.append(1 + rnd() % 9, '\n');         // a run of empty lines
        else {
            const size_t n = rnd() % 301;
            for (size_t i = 0; i < n; i++) s.push_back((char)('A' + rnd() % 26));
            s.push_back('\n');
        }
        if (s.size() > about / 2 && s.size() < about / 2 + 400) s.append(std::string(10000, 'N') + "\n");
    }
    return s;
}

struct Totals { size_t areas = 0, slow_path = 0, tiny = 0, no_newline = 0; };

// one pass over `text` in blocks of `block` bytes; targets: the carry sizes to go through, in order (then random ones up to 600);
// final_carry: what the last block's area leaves for the final one
void run_case(const std::string &path, const std::string &text, size_t block, int workers, const std::vector<size_t> &targets, size_t final_carry, Totals &tot) {
    hast::BlockSource src;
    if (!src.open(path, block)) fail("cannot open " + path);
    hast::WorkerPool pool(workers);
    hast::BlockWork w;
    std::string carry;                             // the model's
    size_t pos = 0, ti = 0, lasts = 0;
    for (;;) {
        if (!w.next(src)) fail("the source failed: " + src.error());
        const bool model_last = pos >= text.size();
        const std::string area = carry + text.substr(pos, block);
        pos += std::min(block, text.size() - pos);
        if (w.last != model_last) fail("last is wrong at offset " + std::to_string(pos));
        if (w.len != area.size() || (w.len && memcmp(w.data, area.data(), w.len) != 0)) fail("the area's bytes differ at offset " + std::to_string(pos));
        w.index(pool);
        std::vector<uint32_t> nl;
        for (const char *p = area.data(), *e = p + area.size(); p < e && (p = (const char *)memchr(p, '\n', (size_t)(e - p))); ++p) nl.push_back((uint32_t)(p - area.data()));
        if (w.nl != nl) fail("the newline index differs at offset " + std::to_string(pos));
        for (size_t i = 1; i < w.nl.size(); i++)
            if (w.nl[i] <= w.nl[i - 1]) fail("the newline index does not ascend");
        tot.areas++;
        tot.tiny += area.size() <= 2;
        tot.no_newline += !model_last && area.find('\n', carry.size()) == std::string::npos;
        tot.slow_path += !model_last && carry.size() > hast::BlockSource::kFrontPad;
        if (w.last) {
            lasts++;
            if (area.empty() != (text.empty() || final_carry == 0)) fail("the final area is not the carry it should be");
            break;
        }
        // the carry this area leaves: the target at hand once the area is long enough for it, everything until then
        size_t want = pos >= text.size() ? final_carry : ti < targets.size() ? targets[ti] : rnd() % 600;
        if (want <= area.size() && pos < text.size()) ti++;
        want = std::min(want, area.size());
        w.keep(src, area.size() - want);
        carry = area.substr(area.size() - want);
    }
    if (lasts != 1) fail("last was flagged " + std::to_string(lasts) + " times");
    if (ti < targets.size()) fail("a carry size was never reached with blocks of " + std::to_string(block));
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) fail("usage: test_block_work SCRATCH_DIR");
    const std::string text = make_text(3u << 20), head = text.substr(0, 20000);
    const std::string big = std::string(argv[1]) + "/big.txt", small = std::string(argv[1]) + "/small.txt", none = std::string(argv[1]) + "/empty.txt";
    const std::pair<const std::string *, const std::string *> files[3] = {{&big, &text}, {&small, &head}, {&none, nullptr}};
    for (const auto &f : files) {
        FILE *fp = fopen(f.first->c_str(), "wb");
        if (!fp || (f.second && fwrite(f.second->data(), 1, f.second->size(), fp) != f.second->size()) || fclose(fp) != 0) fail("cannot write " + *f.first);
    }
    constexpr size_t kPad = hast::BlockSource::kFrontPad;
    // (blocks of 1 MiB: the text has three of them and a short one, the carries that matter are gone through at once)
    const std::vector<size_t> wide = {0, 1, kPad - 1, kPad, kPad + 1, kPad + 1, 0}, few = {kPad, kPad + 1, 0}, narrow = {0, 1, 2, 5, 300, 0};
    Totals tot;
    size_t cases = 0;
    for (int workers : {1, 3})
        for (size_t final_carry : {(size_t)0, (size_t)3}) {
            run_case(big, text, 4096, workers, wide, final_carry, tot), cases++;
            run_case(big, text, (size_t)1 << 20, workers, few, final_carry, tot), cases++;
            for (size_t block : {(size_t)1, (size_t)7}) run_case(small, head, block, workers, narrow, final_carry, tot), cases++;
            run_case(none, std::string(), 4096, workers, {}, 0, tot), cases++;
        }
    if (!tot.slow_path || !tot.tiny || !tot.no_newline) fail("a path was not taken");
    printf("ok cases=%zu areas=%zu slow_path=%zu tiny=%zu no_newline=%zu\n", cases, tot.areas, tot.slow_path, tot.tiny, tot.no_newline);
    return 0;
}
