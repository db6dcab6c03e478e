// Host-only test of dense filing (hast_amd/csrc/hast_common.h, FilterGeom::dense): exact entries filed under every one of a
// string's W m-mers, probed under the m-mer that starts on a fixed grid of the row.
//   1. the rule of filter_geom_for: dense where exact entries fit, W is a power of two <= 8 and the mean load of a sub-bucket
//      stays <= 3.2; m, t, kp are those of the sampled scheme; exact_mode 1 ("once") and 0 (prints) never file densely;
//   2. for random K = 21 keys, both strands: the W (block, sub-bucket, entry) triples a dense insert files are distinct and
//      every one inverts to the string, bit for bit;
//   3. for random reads: filter_dense_pm names an m-mer that starts on the grid, the triple a window probes is one of those its
//      canonical key files, and a read of n windows names ceil(n / W) distinct blocks.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "../../hast_amd/csrc/hast_common.h"

using namespace hast;

static uint64_t rng_state = 0x9876543ull;
static uint64_t rnd() { return rng_state = splitmix64(rng_state); }

typedef std::tuple<uint32_t, uint32_t, uint32_t> Triple;          // block, sub-bucket, the 14 stored bits

static Triple triple_of(uint64_t s, uint32_t pm, const FilterGeom &g) {
    const uint32_t blk = filter_block_of((uint32_t)(s >> (2 * (g.k - g.m - (int)pm))) & (uint32_t)kmer_mask(g.m), g.m);
    const uint32_t c17 = filter_exact_code(s, pm, g);
    return Triple(blk, filter_exact_sub(c17), c17 & 0x3FFFu);
}
// what the build kernel's exact branch does with `dense` set: W entries per strand
static std::vector<Triple> dense_insert(uint64_t key, const FilterGeom &g) {
    std::vector<Triple> out;
    for (int o = 0; o < 2; ++o) {
        const uint64_t s = o ? kmer_revcomp(key, g.k) : key;
        if (o && s == key) break;
        for (uint32_t pm = 0; pm < filter_w(g); ++pm) out.push_back(triple_of(s, pm, g));
    }
    return out;
}
static uint64_t invert(const Triple &t, const FilterGeom &g, uint32_t *pm_out) {
    static uint32_t inv = 0;
    if (!inv) { inv = 1; for (int i = 0; i < 5; ++i) inv *= 2u - 0x1D2C5u * inv; inv &= 0x1FFFFu; }
    const uint32_t blk = std::get<0>(t), back17 = (std::get<1>(t) << 14) | std::get<2>(t);
    const uint32_t code = (back17 * inv) & 0x1FFFFu;
    const int rb = 2 * (g.k - g.m);
    const uint32_t pm = code >> rb, rest = code & ((1u << rb) - 1u);
    const uint64_t mm = (uint64_t)(blk ^ (blk >> g.m)) & kmer_mask(g.m);
    const uint64_t prefix = rest & ((1ull << (2 * pm)) - 1), suffix = rest >> (2 * pm);
    *pm_out = pm;
    return (pm ? prefix << (2 * (g.k - (int)pm)) : 0) | (mm << (2 * (g.k - g.m - (int)pm))) | suffix;
}

int main() {
    // 1. the rule
    struct { int k; uint64_t n; int mo, mode, m, t, kp, exact, dense; } want[] = {
        {21, 400000000ull, 0, -1, 14, 6, 21, 1, 1}, {21, 100000000ull, 0, -1, 14, 6, 21, 1, 1}, {21, 429000000ull, 14, -1, 14, 6, 21, 1, 1},
        {21, 430000000ull, 14, -1, 14, 6, 21, 1, 0}, {21, 800000000ull, 14, -1, 14, 6, 21, 1, 0},           // load 3.204, 5.96: sampled
        {21, 400000000ull, 0, 1, 14, 6, 21, 1, 0}, {21, 400000000ull, 0, 0, 14, 6, 21, 0, 0},               // once; prints
        {31, 800000000ull, 0, -1, 15, 6, 23, 0, 0}, {21, 40000ull, 0, -1, 8, 8, 16, 0, 0},                   // prints: never dense
        {15, 300000ull, 8, -1, 8, 8, 15, 1, 0}, {15, 98000ull, 8, -1, 8, 8, 15, 1, 1},                       // load 9.2 / 2.99 at m = 8
        {17, 400000000ull, 0, -1, 14, 6, 17, 1, 1}, {19, 400000000ull, 0, -1, 14, 8, 19, 1, 0}};             // W = 4; W = 6: exact entries, not a power of two
    for (auto &w : want) {
        const FilterGeom g = filter_geom_for(w.k, w.n, w.mo, 0, 0, w.mode);
        if (g.m != w.m || g.t != w.t || g.kp != w.kp || g.exact != w.exact || g.dense != w.dense) {
            printf("rule: K=%d n=%llu mode %d -> m=%d t=%d kp=%d exact=%d dense=%d (load %.3f)\n", w.k, (unsigned long long)w.n, w.mode, g.m, g.t, g.kp,
                   g.exact, g.dense, filter_dense_load(g, w.n));
            return 1;
        }
        if (g.dense && (!g.exact || (filter_w(g) & (filter_w(g) - 1)) || filter_w(g) > 8 || filter_dense_load(g, w.n) > kFilterDenseMaxLoad)) { printf("rule: dense outside its bounds\n"); return 1; }
    }
    for (uint32_t w = 1; w <= 8; w *= 2)
        for (uint32_t p = 0; p < 5000; ++p) {
            const uint32_t pm = filter_dense_pm(p, w);
            if (pm >= w || (p + pm) % w != w - 1) { printf("pm: W=%u p=%u -> %u\n", w, p, pm); return 1; }
        }
    // 2. + 3. at the benchmark's geometry and at the small ones the GPU tests use
    long n_keys = 0, n_windows = 0;
    struct { int k; uint64_t n; int mo; } geos[] = {{21, 400000000ull, 0}, {15, 98000ull, 8}, {17, 1000ull, 14}, {12, 10ull, 12}};
    for (auto &ge : geos) {
        const FilterGeom g = filter_geom_for(ge.k, ge.n, ge.mo, 0);
        if (!g.dense) { printf("geometry K=%d is not dense\n", ge.k); return 1; }
        const int K = g.k;
        const uint32_t W = filter_w(g);
        for (int it = 0; it < 20000; ++it, ++n_keys) {
            const uint64_t key = kmer_canon(rnd() & kmer_mask(K), K);
            const std::vector<Triple> filed = dense_insert(key, g);
            const bool own_rc = kmer_revcomp(key, K) == key;
            if (filed.size() != (own_rc ? W : 2 * W)) { printf("insert: %zu entries\n", filed.size()); return 1; }
            for (size_t i = 0; i < filed.size(); ++i) {
                uint32_t pm;
                const uint64_t s = i < W ? key : kmer_revcomp(key, K);
                if (std::get<0>(filed[i]) >= filter_nblocks(g) || std::get<1>(filed[i]) >= (uint32_t)kFilterSubs) { printf("insert: range\n"); return 1; }
                if (invert(filed[i], g, &pm) != s || pm != i % W) { printf("invert: K=%d pm=%zu %llx\n", K, i % W, (unsigned long long)s); return 1; }
            }
            // W different pm = W different codes: no two entries of a strand coincide even when its m-mers do (here: poly-A too)
            for (int o = 0; o < (own_rc ? 1 : 2); ++o)
                if (std::set<Triple>(filed.begin() + o * W, filed.begin() + (o + 1) * W).size() != W) { printf("insert: equal entries\n"); return 1; }
        }
        {
            const std::vector<Triple> filed = dense_insert(0, g);                     // poly-A: one m-mer at every position
            if (std::set<Triple>(filed.begin(), filed.begin() + W).size() != W) { printf("poly-A: equal entries\n"); return 1; }
        }
        for (int it = 0; it < 300; ++it) {
            const uint32_t L = (uint32_t)K + (uint32_t)(rnd() % 400), nwin = L - (uint32_t)K + 1;
            std::vector<uint8_t> code(L);
            for (auto &c : code) c = (uint8_t)(rnd() & 3);
            std::set<uint32_t> blocks;
            uint32_t runs = 0, last = 0xFFFFFFFFu;
            for (uint32_t p = 0; p < nwin; ++p, ++n_windows) {
                uint64_t fwd = 0;
                for (int i = 0; i < K; ++i) fwd = (fwd << 2) | code[p + i];
                const uint32_t pm = filter_dense_pm(p, W);
                const Triple probe = triple_of(fwd, pm, g);
                const std::vector<Triple> filed = dense_insert(kmer_canon(fwd, K), g);
                if (std::find(filed.begin(), filed.end(), probe) == filed.end()) { printf("probe: K=%d p=%u not among the filed entries\n", K, p); return 1; }
                blocks.insert(std::get<0>(probe));
                runs += std::get<0>(probe) != last;
                last = std::get<0>(probe);
            }
            // (two grid cells of one read share a random m-mer with probability < 1e-5 per read at m = 14; small m: runs only; the seed is fixed)
            const uint32_t cells = (nwin + W - 1) / W;
            if (runs > cells || (g.m >= 14 && blocks.size() != cells)) { printf("blocks: K=%d L=%u: %u runs, %zu blocks, want %u\n", K, L, runs, blocks.size(), cells); return 1; }
        }
    }
    // a 150-bp read at the benchmark's geometry: 130 windows, 17 blocks
    if ((150 - 21 + 1 + 7) / 8 != 17) return 1;
    printf("ok %ld keys, %ld windows\n", n_keys, n_windows);
    return 0;
}
