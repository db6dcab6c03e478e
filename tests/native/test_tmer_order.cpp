// Host-only test of the t-mer order of the mod-minimizer and of the overflow mark of exact-entry sub-buckets
// (hast_amd/csrc/hast_common.h):
//   1. tmer_order is a total order on the 4096 6-mers: no two t-mers tie at the same position;
//   2. tmer_class_word (the table k_classify_f keeps in LDS) decodes, 2 bits per t-mer, to tmer_class, and the kernel's
//      lookup (word (tm >> 4) & 255, bits 2 (tm & 15)) gives tmer_order for 6-mers and for longer t-mers alike;
//   3. the classes are those of the open-closed order: open syncmers (smallest 3-mer second) before closed ones before
//      the rest, and the class counts are in the expected proportions;
//   4. kFilterOverflowMark never equals an entry and never compares as a hit against any window's 14 code bits;
//   5. an overfull exact-entry filter (K = 15, m = 8, the geometry test_tmer_order_gpu.py classifies) has many sub-buckets
//      that hold exactly 8 entries without turning one away, and many that did turn one away.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../hast_amd/csrc/hast_common.h"

using namespace hast;

static uint64_t rng_state = 0x7e57ull;
static uint64_t rnd() { return rng_state = splitmix64(rng_state); }

int main() {
    // 1
    std::set<uint32_t> seen;
    for (uint32_t tm = 0; tm < 4096; ++tm) seen.insert(tmer_order(tm, 0));
    if (seen.size() != 4096) { printf("order: %zu distinct keys of 4096\n", seen.size()); return 1; }
    // 2
    uint32_t words[kTmerClassWords];
    for (uint32_t w = 0; w < kTmerClassWords; ++w) words[w] = tmer_class_word(w);
    for (uint32_t i = 0; i < 200000; ++i) {
        const uint32_t tm = i < 4096 ? i : (uint32_t)(rnd() & 0xFFFFFFu), pos = (uint32_t)(rnd() & 511u);
        const uint32_t cls = (words[(tm >> 4) & 0xFFu] >> ((tm << 1) & 31u)) & 3u;
        if (cls != tmer_class(tm & 0xFFFu) || tmer_order_cls(tm, pos, cls) != tmer_order(tm, pos)) { printf("lds: tm=%u\n", tm); return 1; }
        if ((tmer_order(tm, pos) & 0xFFFu) != pos || (tmer_order(tm, pos) >> 30) != cls) { printf("layout: tm=%u\n", tm); return 1; }
    }
    // 3
    int n[3] = {0, 0, 0};
    for (uint32_t tm = 0; tm < 4096; ++tm) {
        const uint32_t c = tmer_class(tm);
        if (c > 2) { printf("class: %u\n", c); return 1; }
        uint32_t h[4];
        for (int j = 0; j < 4; ++j) h[j] = (((tm >> (2 * (3 - j))) & 63u) + 1u) * 0x9E3779B1u;
        int at = 0;
        for (int j = 1; j < 4; ++j) if (h[j] < h[at]) at = j;
        if (c != (at == 1 ? 0u : (at == 0 || at == 3) ? 1u : 2u)) { printf("class of %u\n", tm); return 1; }
        ++n[c];
    }
    // a random 6-mer's smallest of 4 random 3-mers is at each place with probability ~1/4: ~1/4 open, ~1/2 closed
    if (n[0] < 800 || n[0] > 1250 || n[1] < 1800 || n[1] > 2300) { printf("class counts %d %d %d\n", n[0], n[1], n[2]); return 1; }
    // 4
    if ((kFilterOverflowMark & 3u) != 0 || kFilterOverflowMark == 0) { printf("mark: tag bits\n"); return 1; }
    for (uint32_t code = 0; code < (1u << 14); ++code) {
        for (uint32_t tags = 1; tags < 4; ++tags)
            if (filter_exact_entry(code, tags) == kFilterOverflowMark) { printf("mark: equals an entry\n"); return 1; }
        const uint32_t fpw = ((code & 0x3FFFu) ^ 0x3FFFu) * 0x00040004u;             // the probe's complement, in both halves
        const uint32_t x = ((kFilterOverflowMark << 16) | kFilterOverflowMark) ^ fpw;
        if ((x >> 16) >= 0xFFFDu || (x & 0xFFFFu) >= 0xFFFDu) { printf("mark: a hit for code %u\n", code); return 1; }
        if (((filter_exact_entry(code, 1) ^ fpw) & 0xFFFFu) < 0xFFFDu) { printf("entry: no hit for code %u\n", code); return 1; }
    }
    // 5: the GPU test's overfull filter, filed as k_filter_build files it (both strands, one sub-bucket per exact code)
    const int K = 15;
    const FilterGeom g = filter_geom_for(K, 0, 8, 0);
    if (!g.exact) { printf("geometry: K=15 m=8 should hold exact entries\n"); return 1; }
    std::vector<uint8_t> cnt(filter_nblocks(g) * kFilterSubs, 0);
    const uint64_t n_keys = 2 * 150000;                            // (two haplotypes of 150k keys, as the GPU test)
    for (uint64_t i = 0; i < n_keys; ++i) {
        const uint64_t key = kmer_canon(rnd() & kmer_mask(K), K);
        for (int o = 0; o < 2; ++o) {
            const uint64_t s = o ? kmer_revcomp(key, K) : key;
            if (o && s == key) break;
            const uint32_t pm = filter_sample_pos(s, g);
            const uint32_t blk = filter_block_of((uint32_t)(s >> (2 * (K - g.m - (int)pm))) & (uint32_t)kmer_mask(g.m), g.m);
            uint8_t &c = cnt[(size_t)blk * kFilterSubs + filter_exact_sub(filter_exact_code(s, pm, g))];
            c = c < 8 ? c + 1 : 9;                                 // 9: full, and an entry was turned away
        }
    }
    size_t full8 = 0, over = 0;
    for (uint8_t c : cnt) { full8 += c == 8; over += c == 9; }
    if (full8 < 5000 || over < 5000) { printf("overfull: %zu exactly full, %zu turned one away\n", full8, over); return 1; }
    printf("ok classes %d %d %d, K=15 m=8: %zu sub-buckets exactly full, %zu turned an entry away\n", n[0], n[1], n[2], full8, over);
    return 0;
}
