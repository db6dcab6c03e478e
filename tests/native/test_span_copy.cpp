// Host test of hast_amd/csrc/span_copy.h: the lane function the copy kernels run (k_rs_copy, k_sqfa_copy, k_rb_copy) is stepped for
// every (tile, lane) of a case, forwards and then backwards -- on the device the calls run in no fixed order -- and held to a serial
// byte-by-byte concatenation written here.  Built with ASAN + UBSAN: the output buffer is exactly olo + total bytes and every item's
// source ends where the item ends, so a write at out + total or a load that leaves its item is caught; the olo bytes in front of the
// output hold a guard pattern.
// What the function requires of trailing items, tested here: the last item need NOT emit (dst[last + 1] >= total + bias is all), and
// items may lie behind the output, one of them across its end; their sources are never asked for.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/span_copy.h"

using namespace hast;

#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
            fprintf(stderr, __VA_ARGS__);               \
            fprintf(stderr, "\n");                      \
            exit(1);                                    \
        }                                               \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;          // fixed seed: every run sees the same cases
static uint32_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

constexpr uint8_t kGuard = 0xA5, kUnwritten = 0xEE;
constexpr uint32_t kLong = 3 * kSpanCopyTile + 1;      // an item longer than three tiles (where the output has room for it)

struct Item {
    uint32_t len;              // table length: dst[j + 1] - dst[j]
    bool fill;                 // one byte, emitted as '\n'; its source is the one byte '>'
};

// one case: the table, the expected output, and the items' sources in one of two layouts
struct Case {
    std::string name;
    std::vector<uint32_t> dst;             // dst[0 .. n]
    uint32_t first, last, bias, total;
    std::vector<uint8_t> want;             // [0, total)
    std::vector<uint8_t *> blocks;         // what free() takes back
    std::vector<const uint8_t *> item_src; // by item; nullptr: must not be asked for
    std::vector<uint32_t> order;           // permuted cases: the record of place j, else empty
    bool fills = false;
    ~Case() {
        for (uint8_t *b : blocks) free(b);
    }
};

static uint8_t content_byte() { return (uint8_t)('a' + rnd() % 26); }      // never '>' and never '\n'

// Lays the items out.  `in_front` items (their lengths sum to bias) emit into the bias; the output ends `cut` bytes before the
// items do.  shift: the residue mod 16 of item j's source address is (5 j + shift) % 16.  permute: 0 no, 1 reversal, 2 shuffle --
// then the sources are the records of one contiguous view in record order, exactly as long as the records are.
static Case *build(const std::string &name, const std::vector<Item> &items, uint32_t in_front, uint32_t cut, uint32_t shift, int permute) {
    Case *c = new Case;
    c->name = name;
    const uint32_t n = (uint32_t)items.size();
    c->dst.resize(n + 1);
    c->dst[0] = 0;
    for (uint32_t j = 0; j < n; ++j) c->dst[j + 1] = c->dst[j] + items[j].len;
    c->first = in_front;
    c->last = n - 1;
    c->bias = c->dst[in_front];
    CHECK(c->dst[n] - c->bias > cut, "%s: nothing left", name.c_str());
    c->total = c->dst[n] - c->bias - cut;
    c->want.assign(c->total, 0);
    c->item_src.assign(n, nullptr);
    std::vector<uint32_t> need(n, 0);      // source bytes of item j that may be read: those that land inside the output
    for (uint32_t j = in_front; j < n; ++j) {
        const uint32_t at = c->dst[j] - c->bias;
        need[j] = at >= c->total ? 0 : std::min(items[j].len, c->total - at);
        c->fills |= items[j].fill;
    }
    std::vector<uint8_t *> where(n, nullptr);
    if (permute) {
        c->order.resize(n);
        std::iota(c->order.begin(), c->order.end(), 0u);
        if (permute == 1) std::reverse(c->order.begin(), c->order.end());
        else
            for (uint32_t i = n; i > 1; --i) std::swap(c->order[i - 1], c->order[rnd() % i]);
        std::vector<uint32_t> place_of(n);
        for (uint32_t j = 0; j < n; ++j) place_of[c->order[j]] = j;
        const size_t view_bytes = std::accumulate(need.begin(), need.end(), (size_t)0);
        uint8_t *view = (uint8_t *)malloc(view_bytes ? view_bytes : 1);
        c->blocks.push_back(view);
        size_t at = 0;
        for (uint32_t r = 0; r < n; ++r) {                      // records in record order: the sources are not monotone in j
            where[place_of[r]] = view + at;
            at += need[place_of[r]];
        }
    } else {
        for (uint32_t j = 0; j < n; ++j) {
            if (!need[j]) continue;
            const uint32_t res = (5 * j + shift) % 16;
            uint8_t *b = nullptr;
            CHECK(posix_memalign((void **)&b, 16, res + need[j]) == 0, "alloc");
            c->blocks.push_back(b);
            where[j] = b + res;                                  // the block ends where the item's readable bytes end
        }
    }
    uint32_t pos = 0;                                            // the serial concatenation
    for (uint32_t j = in_front; j < n; ++j) {
        if (!need[j]) continue;
        c->item_src[j] = where[j];
        if (items[j].fill) {
            CHECK(items[j].len == 1, "a fill item is one byte");
            where[j][0] = '>';
            c->want[pos++] = '\n';
        } else {
            for (uint32_t i = 0; i < need[j]; ++i) c->want[pos++] = where[j][i] = content_byte();
        }
    }
    CHECK(pos == c->total, "%s: %u != %u", name.c_str(), pos, c->total);
    return c;
}

static uint64_t g_lane_calls = 0;

struct PlainSrc {
    static constexpr bool kFills = false;
    const Case *c;
    const uint8_t *at(uint32_t j) const {
        CHECK(j >= c->first && j <= c->last && c->item_src[j], "%s: the source of item %u was asked for", c->name.c_str(), j);
        return c->item_src[j];
    }
};
struct FillSrc : PlainSrc {
    static constexpr bool kFills = true;
    bool fill(const uint8_t *item) const { return item[0] == '>'; }
};
// the permutation in front of the source, as k_rb_copy has it: the table is by place, the sources by record
struct OrderSrc {
    static constexpr bool kFills = false;
    const Case *c;
    std::vector<const uint8_t *> rec_src;
    const uint8_t *at(uint32_t j) const {
        CHECK(j >= c->first && j <= c->last && rec_src[c->order[j]], "%s: the source of place %u was asked for", c->name.c_str(), j);
        return rec_src[c->order[j]];
    }
};

// the shape of the three kernels: the early exit of an empty output, then every (tile, lane)
template <class Src>
static void copy_all(const Case &c, uint32_t total, uint8_t *out16, uint32_t olo, const Src &src, bool backwards) {
    if (!total) return;
    const uint32_t n_tiles = span_copy_tiles(total, olo);
    for (uint32_t i = 0; i < n_tiles * 256; ++i) {
        const uint32_t k = backwards ? n_tiles * 256 - 1 - i : i;
        ++g_lane_calls;
        span_copy_lane(c.dst.data(), c.first, c.last, c.bias, total, out16, olo, src, k / 256, k % 256);
    }
}

template <class Src>
static void run(const Case &c, uint32_t olo, const Src &src) {
    uint8_t *out16 = nullptr;
    CHECK(posix_memalign((void **)&out16, 16, olo + c.total) == 0, "alloc");       // exactly: out + total is the redzone
    for (int backwards = 0; backwards < 2; ++backwards) {
        memset(out16, kGuard, olo);
        memset(out16 + olo, kUnwritten, c.total);
        copy_all(c, c.total, out16, olo, src, backwards != 0);
        for (uint32_t i = 0; i < olo; ++i) CHECK(out16[i] == kGuard, "%s olo %u: byte %u in front of the output was written", c.name.c_str(), olo, i);
        for (uint32_t i = 0; i < c.total; ++i)
            CHECK(out16[olo + i] == c.want[i], "%s olo %u %s: byte %u is %02x, not %02x", c.name.c_str(), olo, backwards ? "backwards" : "forwards", i,
                  out16[olo + i], c.want[i]);
    }
    free(out16);
}

static uint64_t g_cases = 0;
static void run_case(Case *c, bool every_olo) {
    for (uint32_t olo = 0; olo < 16; ++olo) {
        if (!every_olo && olo != 0 && olo != 9) continue;
        if (!c->order.empty()) {
            OrderSrc s{c, std::vector<const uint8_t *>(c->item_src.size(), nullptr)};
            for (size_t j = 0; j < c->item_src.size(); ++j) s.rec_src[c->order[j]] = c->item_src[j];
            run(*c, olo, s);
        } else {
            if (!c->fills) run(*c, olo, PlainSrc{c});
            run(*c, olo, FillSrc{{c}});
        }
        ++g_cases;
    }
    delete c;
}

// item lengths of a pattern until they sum to `total` exactly (the last one is cut to fit)
enum Pattern { kOnes, kSixteens, kSeventeens, kOneLong, kMixed, kPatterns };
static const char *const kPatternName[kPatterns] = {"ones", "16s", "17s", "one_long", "mixed"};
static std::vector<Item> emitting(Pattern pat, uint32_t total) {
    std::vector<Item> v;
    uint32_t sum = 0, j = 0;
    while (sum < total) {
        uint32_t len = 1;
        if (pat == kSixteens) len = 16;
        if (pat == kSeventeens) len = 17;
        if (pat == kOneLong && j == 2) len = kLong;
        if (pat == kMixed) len = rnd() % 41;                     // 0..40: empty items wherever the generator puts them
        len = std::min(len, total - sum);
        v.push_back(Item{len, false});
        sum += len;
        ++j;
    }
    while (!v.empty() && v.back().len == 0) v.pop_back();       // (the variants below decide what stands at the end)
    return v;
}

// empty items: 0 none; 1 at index `first`; 2, 3, 4 a run of 1, 2, 300 between two emitting items; 5 as the last items; 6 all of these
constexpr int kEmptyVariants = 7;
static std::vector<Item> with_empties(std::vector<Item> v, int variant) {
    const Item empty{0, false};
    const size_t mid = v.size() / 2;                            // between two emitting items when there are two
    if (variant == 5 || variant == 6) v.insert(v.end(), 3, empty);
    if (variant == 2 || variant == 6) v.insert(v.begin() + mid, 1, empty);
    if (variant == 3) v.insert(v.begin() + mid, 2, empty);
    if (variant == 4 || variant == 6) v.insert(v.begin() + (mid + 1 < v.size() ? mid + 1 : mid), 300, empty);
    if (variant == 1 || variant == 6) v.insert(v.begin(), 1, empty);
    return v;
}

static void table_search() {
    const std::vector<uint32_t> dst = {0, 0, 3, 3, 3, 10, 11, 11, 40, 40};      // items 0 .. 8; item 7 is the last that emits
    for (uint32_t lo = 0; lo <= 8; ++lo)
        for (uint32_t hi = lo; hi <= 8; ++hi)
            for (uint32_t v = 0; v < dst[hi + 1]; ++v) {        // the precondition: item hi is past v
                uint32_t want = lo;
                while (dst[want + 1] <= v) ++want;
                CHECK(span_first_past(dst.data(), lo, hi, v) == want, "lo %u hi %u v %u", lo, hi, v);
            }
}

int main() {
    table_search();
    CHECK(span_copy_tiles(1, 0) == 1 && span_copy_tiles(4096, 0) == 1 && span_copy_tiles(4096, 1) == 2 && span_copy_tiles(4081, 15) == 1, "tiles");

    // an empty output: the kernels' early exit, the lane function is not entered and nothing is written
    {
        Case c;
        c.dst = {0, 0, 0};
        c.first = 0, c.last = 1, c.bias = 0, c.total = 0;
        uint8_t guard[16];
        memset(guard, kGuard, sizeof guard);
        const uint64_t before = g_lane_calls;
        for (uint32_t olo = 0; olo < 16; ++olo) copy_all(c, 0, guard, olo, PlainSrc{&c}, false);
        CHECK(g_lane_calls == before, "an empty output entered the copy");
        for (uint8_t b : guard) CHECK(b == kGuard, "an empty output wrote");
    }

    const uint32_t totals[] = {1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5};
    const std::vector<Item> front = {{10, false}, {0, false}, {27, false}};     // bias 37, first = 3: what lies in front of the first header
    uint32_t shift = 0;
    for (int pat = 0; pat < kPatterns; ++pat)
        for (uint32_t total : totals)
            for (int ev = 0; ev < kEmptyVariants; ++ev)
                for (int biased = 0; biased < 2; ++biased)
                    for (int behind = 0; behind < 2; ++behind) {
                        std::vector<Item> v = with_empties(emitting((Pattern)pat, total), ev);
                        uint32_t cut = 0;
                        if (behind) {                            // the output ends 7 bytes inside an item; two more and an empty one follow
                            v.push_back(Item{20, false});
                            v.push_back(Item{0, false});
                            v.push_back(Item{5, false});
                            v.push_back(Item{1, false});
                            cut = 13 + 5 + 1;
                        }
                        if (biased) v.insert(v.begin(), front.begin(), front.end());
                        const std::string name = std::string(kPatternName[pat]) + " total " + std::to_string(total + (behind ? 7 : 0)) + " empties " +
                                                 std::to_string(ev) + (biased ? " biased" : "") + (behind ? " behind" : "");
                        run_case(build(name, v, biased ? 3 : 0, cut, shift++ % 16, 0), total <= 17 || total == 4097);
                    }

    // 5000 items of one byte
    run_case(build("5000 ones", emitting(kOnes, 5000), 0, 0, 0, 0), true);

    // the unaligned 16-byte load at every residue of the source address
    for (uint32_t s = 0; s < 16; ++s)
        for (Pattern pat : {kSeventeens, kOneLong, kSixteens})
            for (uint32_t total : {4097u, 3 * 4096u + 5})
                run_case(build(std::string(kPatternName[pat]) + " shift " + std::to_string(s), emitting(pat, total), 0, 0, s, 0), false);

    // fill items: first, two adjacent of which the second opens a 16-byte piece (with olo = 0), at the end of a piece, last
    for (uint32_t total : {40u, 4097u}) {
        std::vector<Item> v = {{1, true}, {14, false}, {1, true}, {1, true}, {14, false}, {1, true}, {0, false}, {1, true}};
        for (const Item &it : emitting(kMixed, total - 33 - 1)) v.push_back(it);
        v.push_back(Item{1, true});
        run_case(build("fills total " + std::to_string(total), v, 0, 0, 3, 0), true);
        v.insert(v.begin(), front.begin(), front.end());
        run_case(build("fills biased total " + std::to_string(total), v, 3, 0, 4, 0), true);
    }
    run_case(build("one fill", {{1, true}}, 0, 0, 0, 0), true);

    // a permutation in front of the sources: the offsets stay monotone, the sources do not
    for (int permute = 1; permute <= 2; ++permute)
        for (Pattern pat : {kMixed, kOneLong, kOnes})
            for (uint32_t total : {17u, 4097u, 3 * 4096u + 5})
                for (int ev : {0, 6})
                    run_case(build(std::string(kPatternName[pat]) + (permute == 1 ? " reversed " : " shuffled ") + std::to_string(total),
                                   with_empties(emitting(pat, total), ev), 0, 0, 0, permute),
                             total != 3 * 4096 + 5);

    printf("ok cases=%llu lane_calls=%llu\n", (unsigned long long)g_cases, (unsigned long long)g_lane_calls);
    return 0;
}
