// test_carry_plan.cpp -- hast_amd/csrc/carry_plan.h driven as a sequential model of a carried-block feed (carry_feed.h without the GPU):
// two host arrays of exactly room_of(block) bytes stand for the device views, a toy framer consumes whole lines, and random inputs go
// through in blocks of 64, 65, 100 and 4096 bytes, short last blocks, host and device blocks mixed, the feed up to one block ahead of
// the framer.  Built with ASan + UBSan by tests/test_carry_plan_cpu.py: an offset outside a view is an error of the sanitizer's
// before it is one of this program's.  Prints "ok cases=N".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/carry_plan.h"

using namespace hast;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: %s (block %zu, seed %u)\n", __FILE__, __LINE__, #cond, g_block, g_seed); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

static size_t g_block;
static unsigned g_seed;

// lines of random lengths; long_lines: some are longer than a block (a step then leaves more than fits)
static std::string make_input(std::mt19937 &rng, size_t block, bool long_lines) {
    std::string s;
    const size_t target = rng() % (8 * block + 1);
    while (s.size() < target) {
        const size_t most = long_lines && rng() % 8 == 0 ? 2 * block + 8 : block - 1;
        const size_t len = rng() % 4 == 0 ? rng() % (most + 1) : rng() % (most < 40 ? most + 1 : 40);
        for (size_t i = 0; i < len; ++i) s.push_back((char)('a' + rng() % 26));
        s.push_back('\n');
    }
    if (!s.empty() && rng() % 2) s.resize(s.size() - 1 - rng() % (s.size() < 20 ? s.size() : 20));       // no line break at the end
    return s;
}

struct Feed {
    carry::Plan plan;
    size_t room;
    uint8_t *view[2];
    explicit Feed(size_t block) : room(carry::room_of(block)) {
        plan.block = block;
        for (uint8_t *&v : view) v = new uint8_t[room];
    }
    ~Feed() {
        for (uint8_t *v : view) delete[] v;
    }
    // one block in: true if the plan says it has to be uploaded
    bool submit(const char *src, size_t n, int what, bool allow_empty) {
        CHECK(plan.may_hand() && plan.hand(what));
        CHECK(plan.may_submit(n, allow_empty));
        const int slot = plan.submit_slot();
        CHECK(plan.new_off() == plan.block && plan.new_off() + n <= room);
        memcpy(view[slot] + plan.new_off(), src, n);
        const bool upload = plan.submitted(n);
        CHECK(upload == (what == 1 && n > 0) && plan.on_device[slot] == !upload && plan.n_new[slot] == n && !plan.handed);
        return upload;
    }
    // one step of the toy framer: whole lines go to `out`; false: what it leaves does not fit
    bool step(std::string &out, bool done_first) {
        CHECK(plan.waiting());
        const carry::View v = plan.view();
        CHECK(v.slot == plan.step_slot() && v.off <= plan.block && v.off == plan.block - plan.tail && v.off + v.bytes <= room);
        CHECK(v.bytes == plan.tail + plan.n_new[v.slot]);
        const uint8_t *p = view[v.slot] + v.off;
        size_t consumed = v.bytes;
        while (consumed && p[consumed - 1] != '\n') --consumed;
        const size_t left = v.bytes - consumed;
        if (!plan.fits(left)) {
            CHECK(left > plan.block);
            return false;
        }
        out.append(reinterpret_cast<const char *>(p), consumed);
        if (done_first) plan.done();                 // (hast_rs counts the block before it carries, hast_sq_feed behind)
        const int dst = v.slot ^ 1;
        const size_t at = plan.left_off(left);
        CHECK(dst != v.slot && at + left == plan.new_off() && at <= plan.block);          // ends where the new bytes begin: no overlap
        memcpy(view[dst] + at, p + consumed, left);
        plan.tail = left;
        if (!done_first) plan.done();
        CHECK(plan.step_slot() == dst);              // the next step finds them in its own view
        return true;
    }
    void take_tail(std::string &out) {
        CHECK(!plan.waiting());
        const carry::View v = plan.tail_view();
        CHECK(v.slot == plan.step_slot() && v.bytes == plan.tail && v.off + v.bytes == plan.block);
        out.append(reinterpret_cast<const char *>(view[v.slot] + v.off), v.bytes);
        plan.drop_tail();
        CHECK(plan.tail == 0 && plan.at_rest());
    }
};

static void run_case(size_t block, unsigned seed, bool long_lines) {
    g_block = block;
    g_seed = seed;
    std::mt19937 rng(seed * 7919u + (unsigned)block);
    const std::string in = make_input(rng, block, long_lines);
    Feed f(block);
    std::string out;
    size_t pos = 0;
    bool refused = false;
    const bool done_first = seed & 1, allow_empty = seed & 2;
    CHECK(f.plan.at_rest());
    for (bool more = true; more || f.plan.waiting();) {
        // up to two blocks on their way; a third is refused
        while (more && f.plan.may_hand() && (f.plan.waiting() ? rng() % 2 : 1)) {
            const size_t n = in.size() - pos < block ? in.size() - pos : rng() % 6 == 0 && in.size() - pos > block ? block - rng() % block : block;
            if (n == 0 && !allow_empty) {
                CHECK(!f.plan.may_submit(0, false));
                more = false;
                break;
            }
            f.submit(in.data() + pos, n, 1 + (int)(rng() % 2), allow_empty);
            pos += n;
            if (n == 0 || (pos == in.size() && rng() % 2)) more = false;
        }
        if (f.plan.n_submitted - f.plan.n_done == 2) CHECK(!f.plan.may_hand() && !f.plan.hand(1) && !f.plan.may_submit(1, true) && !f.plan.handed);
        if (!f.plan.waiting()) continue;
        if (!f.step(out, done_first)) {
            refused = true;
            break;
        }
    }
    if (refused) {
        CHECK(long_lines);
        CHECK(in.compare(0, out.size(), out) == 0);  // what was framed before is a prefix of the input
        return;
    }
    CHECK(pos == in.size());
    f.take_tail(out);
    CHECK(out == in);
}

int main() {
    size_t cases = 0, refused_possible = 0;
    for (size_t block : {(size_t)64, (size_t)65, (size_t)100, (size_t)4096}) {
        for (unsigned seed = 0; seed < 300; ++seed, ++cases) run_case(block, seed, false);
        for (unsigned seed = 0; seed < 60; ++seed, ++cases, ++refused_possible) run_case(block, seed, true);
        carry::Plan p;
        p.block = block;
        g_block = block;
        CHECK(p.fits(block) && !p.fits(block + 1) && p.fits(0) && p.left_off(block) == 0 && p.left_off(0) == block);
        CHECK(carry::room_of(block) == 2 * block + 64);
        CHECK(!p.may_submit(1, false));              // nothing in hand
        CHECK(p.hand(2) && !p.may_submit(block + 1, true) && !p.may_submit(0, false) && p.may_submit(0, true) && p.may_submit(block, false));
        CHECK(!p.submitted(0) && p.on_device[0]);    // an empty block is not uploaded
        CHECK(p.hand(1) && p.submitted(block) && !p.on_device[1] && !p.may_hand() && !p.hand(1));
        ++cases;
    }
    printf("ok cases=%zu refusals_tried=%zu\n", cases, refused_possible);
    return 0;
}
