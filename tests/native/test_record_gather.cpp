// Host test of hast_amd/csrc/record_gather.h: the lane function the gather kernels run (k_route_copy, k_rs_names, k_sq_copy) is stepped
// for every (wave, lane) of a tile, forwards and then backwards -- on the device the waves run in no fixed order -- and held to a serial
// concatenation written here.  Built with ASAN + UBSAN.  The output buffer is exactly as long as the items are, and the items lie in
// it in runs as the routing kernel places them, so their destinations are not monotone.  Every item's source is exactly the bytes the
// contract lets the function read (with the newline policy one fewer than the item is long) and stands between poisoned bytes, so a
// load in front of an item or behind it is caught; the staged entries behind the live items hold offsets far outside both buffers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../hast_amd/csrc/record_gather.h"

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

constexpr uint8_t kUnwritten = 0xEE;
constexpr uint32_t kLong = 5003;                        // an item of several thousand bytes: 78 steps and a rest
static const uint32_t kLens[] = {0, 1, 63, 64, 65, 127, 128, 129, kLong};
constexpr uint32_t kNLens = sizeof kLens / sizeof kLens[0];
constexpr uint32_t kRuns = 4;                           // the item i goes to run (7 i) % 4: four runs one behind the other

static uint64_t g_cases = 0, g_lane_calls = 0;

template <class Policy>
static void run_case(const std::string &name, const std::vector<uint32_t> &len) {
    const uint32_t live = (uint32_t)len.size();
    CHECK(live <= 256, "%s", name.c_str());
    // the staged tile: entries at and behind `live` must not be looked at
    std::vector<uint32_t> src(256, 0xFFFFFF00u), dst(256, 0xFFFFFF00u), n(256, 100000);
    // destinations: run by run, the items of a run in item order
    uint32_t total = 0;
    for (uint32_t run = 0; run < kRuns; ++run)
        for (uint32_t i = 0; i < live; ++i)
            if ((7 * i) % kRuns == run) {
                dst[i] = total;
                total += len[i];
            }
    // sources: every item at an 8-byte boundary (ASAN's granule), a poisoned granule at least in front of it and behind it; in a
    // shuffled order, so that they are not monotone either
    std::vector<uint32_t> order(live);
    for (uint32_t i = 0; i < live; ++i) order[i] = i;
    for (uint32_t i = live; i > 1; --i) std::swap(order[i - 1], order[rnd() % i]);
    std::vector<uint32_t> readable(live);
    size_t in_bytes = 8;
    for (uint32_t i : order) {
        readable[i] = Policy::kNewlineEnds && len[i] ? len[i] - 1 : len[i];
        n[i] = len[i];
        src[i] = (uint32_t)in_bytes;                             // (a readable length of 0: the offset of a poisoned byte)
        in_bytes += (readable[i] + 7) / 8 * 8 + 8;
    }
    uint8_t *in = nullptr;
    CHECK(posix_memalign((void **)&in, 8, in_bytes) == 0, "alloc");
    std::vector<uint8_t> want(total, 0);
    for (uint32_t i = 0; i < live; ++i) {
        for (uint32_t b = 0; b < readable[i]; ++b) want[dst[i] + b] = in[src[i] + b] = (uint8_t)('a' + rnd() % 26);
        if (Policy::kNewlineEnds && len[i]) want[dst[i] + len[i] - 1] = '\n';
    }
    ASAN_POISON_MEMORY_REGION(in, in_bytes);
    for (uint32_t i = 0; i < live; ++i) ASAN_UNPOISON_MEMORY_REGION(in + src[i], readable[i]);
    uint8_t *out = (uint8_t *)malloc(total ? total : 1);         // exactly: out + total is the redzone
    for (int backwards = 0; backwards < 2; ++backwards) {
        memset(out, kUnwritten, total ? total : 1);
        for (uint32_t k = 0; k < 256; ++k) {
            const uint32_t t = backwards ? 256 - 1 - k : k;
            ++g_lane_calls;
            record_gather_lane<Policy>(in, out, src.data(), dst.data(), n.data(), live, t / 64, t % 64);
        }
        if (!total) CHECK(out[0] == kUnwritten, "%s: an empty tile wrote", name.c_str());
        for (uint32_t p = 0; p < total; ++p)
            CHECK(out[p] == want[p], "%s %s %s: byte %u is %02x, not %02x", name.c_str(), Policy::kNewlineEnds ? "lines" : "bytes", backwards ? "backwards" : "forwards",
                  p, out[p], want[p]);
    }
    ASAN_UNPOISON_MEMORY_REGION(in, in_bytes);
    free(in);
    free(out);
    ++g_cases;
}

static void both(const std::string &name, const std::vector<uint32_t> &len) {
    run_case<GatherBytes>(name, len);
    run_case<GatherLines>(name, len);
}

// the lengths of `live` items: emitting ones taken round kLens from `phase` on (0 left out), with zero-length items
//   variant 0: none but those of the cycle (kLens holds a 0)   1: in front   2: a run of five in the middle   3: one between two that emit
//   4: at the end   5: all of these
static std::vector<uint32_t> lengths(uint32_t live, uint32_t phase, int variant) {
    std::vector<uint32_t> v(live);
    for (uint32_t i = 0; i < live; ++i) {
        uint32_t l = kLens[(i + phase) % kNLens];
        if (variant && l == 0) l = 2;
        v[i] = l;
    }
    auto zero = [&](uint32_t from, uint32_t count) {
        for (uint32_t i = from; i < from + count && i < live; ++i) v[i] = 0;
    };
    if (variant == 1 || variant == 5) zero(0, 3);
    if (variant == 2 || variant == 5) zero(live / 2, 5);
    if (variant == 3 || variant == 5) zero(live / 4 + 1, 1);
    if ((variant == 4 || variant == 5) && live >= 3) zero(live - 3, 3);
    return v;
}

int main() {
    const uint32_t lives[] = {0, 1, 63, 64, 65, 255, 256};
    for (uint32_t live : lives) {
        for (int variant = 0; variant < 6; ++variant)
            for (uint32_t phase = 0; phase < kNLens; ++phase)
                both("live " + std::to_string(live) + " phase " + std::to_string(phase) + " zeros " + std::to_string(variant), lengths(live, phase, variant));
        for (uint32_t l : kLens) both("live " + std::to_string(live) + " all " + std::to_string(l), std::vector<uint32_t>(live, l));
        for (int round = 0; round < 4; ++round) {
            std::vector<uint32_t> v(live);
            for (uint32_t &l : v) l = rnd() % 3 ? kLens[rnd() % (kNLens - 1)] : 0;      // a third empty, no long ones
            both("live " + std::to_string(live) + " random " + std::to_string(round), v);
        }
    }
    // the newline policy on an item of length 1: '\n' and no source byte at all (run_case gives it none)
    run_case<GatherLines>("one newline", {1});
    printf("ok cases=%llu lane_calls=%llu\n", (unsigned long long)g_cases, (unsigned long long)g_lane_calls);
    return 0;
}
