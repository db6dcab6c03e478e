// test_tx_feed_plan.cpp -- the paired feed of `fake_10x --inflate device` (hast_amd/csrc/tx_feed.cpp) as a sequential model: who
// reads, which mode a step has and when the feed hands over to the host come from hast_amd/csrc/tx_feed_plan.h alone, i.e. from the
// counts a step leaves behind (newlines, pairs, consumed bytes) and never from the bytes; the conversion is tx::pair_host.  It is
// compared, step by step, with a direct re-implementation of fake_10x_main.cpp's loop over have[] byte vectors.
//   test_tx_feed_plan SEED CASES   CASES random record streams of 200-2000 pairs, blocks of 64 B - 8 KB, the two sides of unequal
//       record length and unequal record count (sometimes ending inside a record); every fourth case has one record longer than
//       the feed's room.  Per case both routes must give the same sequence of (who read, mode, consumed, carried bytes), the same
//       outputs and the same state; a side of the model that has to read must fit its room unless one of its records does not.
// Exit 0: all equal (one summary line on stderr); 1: a difference (said on stderr); 2: usage.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../hast_amd/csrc/tx_feed_plan.h"
#include "../../hast_amd/csrc/tx_host.h"

using namespace hast;

namespace {

uint64_t g_rng = 1;
uint64_t rnd() {                   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t between(uint64_t lo, uint64_t hi) { return lo + rnd() % (hi - lo + 1); }

struct Step {
    bool read[2];
    int mode;
    uint64_t consumed[2];
    size_t carry[2];
    bool operator==(const Step &o) const {
        return read[0] == o.read[0] && read[1] == o.read[1] && mode == o.mode && consumed[0] == o.consumed[0] && consumed[1] == o.consumed[1] &&
               carry[0] == o.carry[0] && carry[1] == o.carry[1];
    }
};

struct Route {
    std::vector<Step> steps;
    std::string out[2];
    tx::State st;
};

struct Source {
    const std::vector<uint8_t> *bytes;
    size_t at = 0;
    bool eof = false;
    size_t read(std::vector<uint8_t> &to, size_t block) {           // as the program: a read short of a block is the input's end
        const size_t n = bytes->size() - at < block ? bytes->size() - at : block;
        to.insert(to.end(), bytes->begin() + (long)at, bytes->begin() + (long)(at + n));
        at += n;
        if (n < block) eof = true;
        return n;
    }
};

bool has_record(const std::vector<uint8_t> &v) {
    uint64_t rec;
    tx::whole_records(v.data(), v.size(), 1, &rec);
    return rec > 0;
}

// fake_10x_main.cpp's loop, from any point of it: have[] and the sources as they are, read_done as host_loop takes it
void program_loop(const tx::Map &map, Source src[2], std::vector<uint8_t> have[2], size_t block, bool read_done, Route &r) {
    for (int mode = 0; mode != 1; read_done = false) {
        Step s{};
        for (int side = 0; side < 2 && !read_done; ++side) {
            if (src[side].eof || (have[side].size() > block && has_record(have[side]))) continue;
            src[side].read(have[side], block);
            s.read[side] = true;
        }
        mode = tx::step_mode(src[0].eof, src[1].eof, have[0].data(), have[0].size(), have[1].data(), have[1].size());
        size_t c[2];
        tx::pair_host(map, have[0].data(), have[0].size(), have[1].data(), have[1].size(), mode, r.st, r.out[0], r.out[1], &c[0], &c[1]);
        for (int side = 0; side < 2; ++side) {
            have[side].erase(have[side].begin(), have[side].begin() + (long)c[side]);
            s.consumed[side] = c[side];
            s.carry[side] = have[side].size();
        }
        s.mode = mode;
        r.steps.push_back(s);
    }
}

struct Tally {
    uint64_t cases = 0, steps = 0, feed_steps = 0, side_skipped = 0, ends = 0, too_long = 0;
};

// the feed: txfeed::Side decides, mem[] stands for the bytes in device memory (looked at by the conversion only)
bool feed_route(const tx::Map &map, const std::vector<uint8_t> in[2], const size_t longest[2], size_t block, Route &r, Tally &t) {
    Source src[2] = {{&in[0]}, {&in[1]}};
    std::vector<uint8_t> mem[2];
    txfeed::Side side[2];
    const size_t room = txfeed::room_of(block);
    bool read_done = false;
    for (;;) {
        Step s{};
        for (int k = 0; k < 2; ++k) {
            if (!side[k].wants(block)) {
                if (!side[k].eof) ++t.side_skipped;
                continue;
            }
            if (!txfeed::fits(side[k].carry, block, room)) {
                fprintf(stderr, "side %d wants to read with %zu bytes carried, the room is %zu\n", k, side[k].carry, room);
                return false;                                        // (a step must have said HAST_TX_TAIL_TOO_LONG before)
            }
            side[k].submitted(src[k].read(mem[k], block), block);
            s.read[k] = true;
        }
        for (int k = 0; k < 2; ++k)
            if (mem[k].size() != side[k].held() || mem[k].size() > room) {
                fprintf(stderr, "side %d holds %zu bytes, the plan says %zu, the room is %zu\n", k, mem[k].size(), side[k].held(), room);
                return false;
            }
        uint32_t lines[2] = {0, 0};
        for (int k = 0; k < 2; ++k)
            for (uint8_t b : mem[k]) lines[k] += b == '\n';
        const int mode = txfeed::mode_of(side[0].eof, side[1].eof, lines[0], lines[1]);
        if (mode != 0) {                                             // HAST_TX_ENDS: the step is the host loop's, its reads are made
            ++t.ends;
            read_done = true;
            // the reads of this step belong to the step the host loop logs first
            r.steps.push_back(s);
            break;
        }
        const uint64_t headers = r.st.headers;
        size_t c[2];
        tx::pair_host(map, mem[0].data(), mem[0].size(), mem[1].data(), mem[1].size(), 0, r.st, r.out[0], r.out[1], &c[0], &c[1]);
        bool too_long = false;
        for (int k = 0; k < 2; ++k) {
            mem[k].erase(mem[k].begin(), mem[k].begin() + (long)c[k]);
            side[k].stepped(lines[k], r.st.headers - headers, c[k]);
            s.consumed[k] = c[k];
            s.carry[k] = side[k].carry;
            if (side[k].wants(block) && !txfeed::fits(side[k].carry, block, room)) {
                too_long = true;
                if (longest[k] <= room - block) {
                    fprintf(stderr, "side %d carries %zu bytes of a room of %zu, its longest record has %zu\n", k, side[k].carry, room, longest[k]);
                    return false;
                }
            }
        }
        s.mode = 0;
        r.steps.push_back(s);
        ++t.feed_steps;
        if (too_long) {
            ++t.too_long;
            break;
        }
    }
    // both tails come down, the program's loop ends the run
    for (int k = 0; k < 2; ++k) src[k].eof = side[k].eof;
    Route rest;
    rest.st = r.st;
    program_loop(map, src, mem, block, read_done, rest);
    if (read_done) {               // the first step of the rest IS the step the feed left in the middle: its reads were the feed's
        rest.steps[0].read[0] = r.steps.back().read[0];
        rest.steps[0].read[1] = r.steps.back().read[1];
        r.steps.pop_back();
    }
    r.steps.insert(r.steps.end(), rest.steps.begin(), rest.steps.end());
    r.out[0] += rest.out[0];
    r.out[1] += rest.out[1];
    r.st = rest.st;
    return true;
}

void record(std::vector<uint8_t> &to, uint64_t i, int side, size_t len, bool known) {
    char head[64];
    const int n = snprintf(head, sizeof head, "@r%llu#%s/%d\n", (unsigned long long)i, known ? (i % 3 ? "k1" : "key2") : "absent", side + 1);
    to.insert(to.end(), head, head + n);
    for (size_t b = 0; b < len; ++b) to.push_back((uint8_t)"ACGT"[(i + b) & 3]);
    to.push_back('\n');
    to.push_back('+');
    to.push_back('\n');
    for (size_t b = 0; b < len; ++b) to.push_back((uint8_t)('!' + (i + b) % 40));
    to.push_back('\n');
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: test_tx_feed_plan SEED CASES\n");
        return 2;
    }
    g_rng = strtoull(argv[1], nullptr, 10);
    const uint64_t n_cases = strtoull(argv[2], nullptr, 10);
    const char map_text[] = "k1\tACGTACGTACGTACGT\nkey2\tTTTTCCCCGGGGAAAA\n";
    tx::Map map;
    tx::map_parse(reinterpret_cast<const uint8_t *>(map_text), sizeof map_text - 1, map);
    Tally t;
    for (uint64_t c = 0; c < n_cases; ++c) {
        const bool giant = c % 4 == 3;
        const size_t block = (size_t)between(giant ? 4096 : 64, 8192);          // (a giant record in blocks of 64 bytes is 16 000 steps over 1 MB)
        const uint64_t pairs = between(200, 2000);
        // unequal record counts: read 2 shorter, longer, or the same; unequal record lengths: one side up to 8 x the other
        uint64_t n_rec[2] = {pairs, pairs};
        const uint64_t shape = rnd() % 3;
        if (shape == 1) n_rec[1] = pairs - between(1, pairs / 2);
        if (shape == 2) n_rec[0] = pairs - between(1, pairs / 2);
        const size_t base = (size_t)between(1, 150);
        size_t len[2] = {base, base};
        len[rnd() & 1] = base * (size_t)between(2, 8);
        const uint64_t giant_at = giant ? between(0, n_rec[0] < n_rec[1] ? n_rec[0] - 1 : n_rec[1] - 1) : ~0ull;
        const int giant_side = (int)(rnd() & 1);
        std::vector<uint8_t> in[2];
        size_t longest[2] = {0, 0};
        for (int s = 0; s < 2; ++s)
            for (uint64_t i = 0; i < n_rec[s]; ++i) {
                const size_t had = in[s].size();
                const size_t l = i == giant_at && s == giant_side ? (size_t)between(520000, 560000) : len[s] + (size_t)(rnd() % (len[s] / 4 + 1));
                record(in[s], i, s, l, rnd() % 5 != 0);
                if (in[s].size() - had > longest[s]) longest[s] = in[s].size() - had;
            }
        for (int s = 0; s < 2; ++s)
            if (rnd() % 3 == 0 && in[s].size() > 10) in[s].resize(in[s].size() - (size_t)between(1, 10));      // an input that ends inside a record
        Route want, got;
        {
            Source src[2] = {{&in[0]}, {&in[1]}};
            std::vector<uint8_t> have[2];
            program_loop(map, src, have, block, false, want);
        }
        if (!feed_route(map, in, longest, block, got, t)) return 1;
        bool same = want.steps.size() == got.steps.size() && want.out[0] == got.out[0] && want.out[1] == got.out[1] && want.st.used == got.st.used &&
                    want.st.headers == got.st.headers;
        for (size_t i = 0; same && i < want.steps.size(); ++i) same = want.steps[i] == got.steps[i];
        if (!same) {
            fprintf(stderr, "case %llu (block %zu, %llu and %llu records): the feed's sequence is not the program's (%zu and %zu steps)\n", (unsigned long long)c, block,
                    (unsigned long long)n_rec[0], (unsigned long long)n_rec[1], got.steps.size(), want.steps.size());
            return 1;
        }
        ++t.cases;
        t.steps += want.steps.size();
    }
    fprintf(stderr, "cases=%llu steps=%llu feed_steps=%llu side_skipped=%llu ends=%llu too_long=%llu\n", (unsigned long long)t.cases, (unsigned long long)t.steps,
            (unsigned long long)t.feed_steps, (unsigned long long)t.side_skipped, (unsigned long long)t.ends, (unsigned long long)t.too_long);
    return 0;
}
