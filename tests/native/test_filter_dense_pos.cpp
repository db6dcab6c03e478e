// Host-only test of the DENSE filter's entries and marks (hast_amd/csrc/hast_common.h: filter_dense_code, filter_mark_sig,
// filter_dense_file -- the routine k_filter_build runs, here with its steps in sequence):
//   (a) the 2 W (block, sub-bucket, stored bits) triples a key files are distinct and each inverts to its string -- random keys and poly-A;
//   (b) a window of a random read probes a triple its canonical key files, and a read of n windows names ceil(n / W) blocks;
//   (c) the filing invariant: 98 000 keys at K = 15 / m = 8 (some 2000 sub-buckets overflow), filed forward, in reverse and
//       shuffled: every filed (string, pm) either matches a slot of its sub-bucket or that sub-bucket is marked and the mark's
//       signature holds both of the pair's bits -- no false negative; and of random windows that were never filed, fewer are
//       sent on to the table than a constant mark would send (both shares are printed);
//   (d) no mark value compares as a hit against any window: (mark ^ fpw) < 0xFFFD for all 2^14 stored values and all marks.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <unordered_set>
#include <vector>

#include "../../hast_amd/csrc/hast_common.h"

using namespace hast;

static uint64_t rng_state = 0x13572468ull;
static uint64_t rnd() { return rng_state = splitmix64(rng_state); }

typedef std::tuple<uint32_t, uint32_t, uint32_t> Triple;          // block, sub-bucket, the 14 stored bits

static Triple triple_of(uint64_t s, uint32_t pm, const FilterGeom &g) {
    const uint32_t blk = filter_block_of((uint32_t)(s >> (2 * (g.k - g.m - (int)pm))) & (uint32_t)kmer_mask(g.m), g.m);
    const uint32_t c17 = filter_dense_code(s, pm, g, (uint32_t)filter_pos_bits(g));
    return Triple(blk, filter_exact_sub(c17), c17 & 0x3FFFu);
}
static std::vector<Triple> triples_of_key(uint64_t key, const FilterGeom &g) {
    std::vector<Triple> out;
    for (int o = 0; o < 2; ++o) {
        const uint64_t s = o ? kmer_revcomp(key, g.k) : key;
        if (o && s == key) break;
        for (uint32_t pm = 0; pm < filter_w(g); ++pm) out.push_back(triple_of(s, pm, g));
    }
    return out;
}
// block + sub-bucket + stored bits -> the string, without a multiply
static uint64_t invert(const Triple &t, const FilterGeom &g, uint32_t *pm_out) {
    const uint32_t pb = (uint32_t)filter_pos_bits(g), blk = std::get<0>(t);
    const uint32_t pm = filter_dense_pm_of(std::get<1>(t), pb), rest = filter_dense_rest_of(std::get<1>(t), std::get<2>(t), pb);
    const uint64_t mm = (uint64_t)(blk ^ (blk >> g.m)) & kmer_mask(g.m);
    const uint64_t prefix = rest & ((1ull << (2 * pm)) - 1), suffix = rest >> (2 * pm);
    *pm_out = pm;
    return (pm ? prefix << (2 * (g.k - (int)pm)) : 0) | (mm << (2 * (g.k - g.m - (int)pm))) | suffix;
}
static int check_key(uint64_t key, const FilterGeom &g) {
    const int K = g.k;
    const uint32_t W = filter_w(g);
    const std::vector<Triple> filed = triples_of_key(key, g);
    const bool own_rc = kmer_revcomp(key, K) == key;
    if (filed.size() != (own_rc ? W : 2 * W)) { printf("(a) K=%d: %zu entries\n", K, filed.size()); return 1; }
    for (size_t i = 0; i < filed.size(); ++i) {
        uint32_t pm;
        const uint64_t s = i < W ? key : kmer_revcomp(key, K);
        if (std::get<0>(filed[i]) >= filter_nblocks(g) || std::get<1>(filed[i]) >= (uint32_t)kFilterSubs || std::get<2>(filed[i]) > 0x3FFFu) { printf("(a) range\n"); return 1; }
        if (invert(filed[i], g, &pm) != s || pm != i % W) { printf("(a) invert: K=%d pm=%zu %llx\n", K, i % W, (unsigned long long)s); return 1; }
    }
    if (std::set<Triple>(filed.begin(), filed.end()).size() != filed.size()) { printf("(a) K=%d key %llx: equal triples\n", K, (unsigned long long)key); return 1; }
    return 0;
}
// one read of base codes: (b)
static int check_read(const std::vector<uint8_t> &code, const FilterGeom &g, bool count_blocks, long *n_windows) {
    const int K = g.k;
    const uint32_t W = filter_w(g), L = (uint32_t)code.size(), nwin = L - (uint32_t)K + 1;
    std::set<uint32_t> blocks;
    uint32_t runs = 0, last = 0xFFFFFFFFu;
    for (uint32_t p = 0; p < nwin; ++p, ++*n_windows) {
        uint64_t fwd = 0;
        for (int i = 0; i < K; ++i) fwd = (fwd << 2) | code[p + i];
        const Triple probe = triple_of(fwd, filter_dense_pm(p, W), g);
        const std::vector<Triple> filed = triples_of_key(kmer_canon(fwd, K), g);
        if (std::find(filed.begin(), filed.end(), probe) == filed.end()) { printf("(b) K=%d p=%u: not among the filed triples\n", K, p); return 1; }
        blocks.insert(std::get<0>(probe));
        runs += std::get<0>(probe) != last;
        last = std::get<0>(probe);
    }
    // (two grid cells of one read share a random m-mer with probability < 1e-5 per read at m = 14; small m and poly-A: runs only)
    const uint32_t cells = (nwin + W - 1) / W;
    if (runs > cells || (count_blocks && g.m >= 14 && blocks.size() != cells)) { printf("(b) K=%d L=%u: %u runs, %zu blocks, want %u\n", K, L, runs, blocks.size(), cells); return 1; }
    return 0;
}

struct Filed { uint32_t sub_index, entry; };                      // sub-bucket (block * 8 + sub), the 16-bit entry
static uint32_t slot(const std::vector<uint32_t> &filt, uint32_t sub_index, int i) { return (filt[(size_t)sub_index * 4 + i / 2] >> (16 * (i & 1))) & 0xFFFFu; }

int main() {
    long n_keys = 0, n_windows = 0;
    struct { int k; uint64_t n; int mo; uint32_t w; } geos[] = {{21, 400000000ull, 0, 8}, {15, 98000ull, 8, 8}, {17, 1000ull, 14, 4}, {12, 10ull, 12, 1}};
    for (auto &ge : geos) {
        const FilterGeom g = filter_geom_for(ge.k, ge.n, ge.mo, 0);
        if (!g.dense || filter_w(g) != ge.w) { printf("geometry K=%d: dense=%d W=%u\n", ge.k, g.dense, filter_w(g)); return 1; }
        const int K = g.k;
        std::set<uint32_t> subs_used;
        for (int it = 0; it < 20000; ++it, ++n_keys) {
            const uint64_t key = kmer_canon(rnd() & kmer_mask(K), K);
            if (check_key(key, g)) return 1;
            for (const Triple &t : triples_of_key(key, g)) subs_used.insert(std::get<1>(t));
        }
        if (check_key(0, g)) return 1;                                                // poly-A: one m-mer at every position
        // all 8 sub-buckets stay in use whatever W is (W < 8: the flank's low bits fill in), as far as the flanks have bits to give
        const int spare = 3 - filter_pos_bits(g), flank_bits = 2 * (K - g.m);
        const uint32_t want_subs = filter_w(g) << (flank_bits < spare ? flank_bits : spare);
        if (subs_used.size() != want_subs) { printf("(a) K=%d: %zu sub-buckets in use, want %u\n", K, subs_used.size(), want_subs); return 1; }
        for (int it = 0; it < 300; ++it) {
            std::vector<uint8_t> code((size_t)K + (size_t)(rnd() % 400));
            for (auto &c : code) c = (uint8_t)(rnd() & 3);
            if (check_read(code, g, true, &n_windows)) return 1;
        }
        if (check_read(std::vector<uint8_t>((size_t)K + 137, 0), g, false, &n_windows)) return 1;      // a poly-A read
    }

    // (c) the invariant of filter_dense_file, three filing orders
    {
        const FilterGeom g = filter_geom_for(15, 98000, 8, 0);
        const int K = g.k;
        const uint32_t W = filter_w(g), pb = (uint32_t)filter_pos_bits(g);
        std::vector<uint64_t> keys;
        std::unordered_set<uint64_t> key_set;
        while (keys.size() < 98000) {
            const uint64_t key = kmer_canon(rnd() & kmer_mask(K), K);
            if (key_set.insert(key).second) keys.push_back(key);
        }
        // random windows that were never filed, and where each would look
        std::vector<Filed> strangers;
        while (strangers.size() < 400000) {
            const uint64_t s = rnd() & kmer_mask(K);
            if (key_set.count(kmer_canon(s, K))) continue;
            const uint32_t pm = (uint32_t)(rnd() % W);
            const uint32_t blk = filter_block_of((uint32_t)(s >> (2 * (K - g.m - (int)pm))) & (uint32_t)kmer_mask(g.m), g.m);
            const uint32_t c17 = filter_dense_code(s, pm, g, pb);
            strangers.push_back({blk * 8 + filter_exact_sub(c17), c17 & 0x3FFFu});
        }
        for (int order = 0; order < 3; ++order) {
            std::vector<uint64_t> ks = keys;
            if (order == 1) std::reverse(ks.begin(), ks.end());
            if (order == 2) for (size_t i = ks.size(); i > 1; --i) std::swap(ks[i - 1], ks[rnd() % i]);
            std::vector<uint32_t> filt((size_t)filter_nblocks(g) * 32, 0);
            std::vector<Filed> filed;
            for (uint64_t key : ks) {
                const uint32_t tags = 1 + (uint32_t)(key % 3);
                for (int o = 0; o < 2; ++o) {
                    const uint64_t s = o ? kmer_revcomp(key, K) : key;
                    if (o && s == key) break;
                    for (uint32_t pm = 0; pm < W; ++pm) {
                        const uint32_t blk = filter_block_of((uint32_t)(s >> (2 * (K - g.m - (int)pm))) & (uint32_t)kmer_mask(g.m), g.m);
                        const uint32_t c17 = filter_dense_code(s, pm, g, pb), sub_index = blk * 8 + filter_exact_sub(c17);
                        const uint32_t entry = filter_exact_entry(c17, tags);
                        filter_dense_file(&filt[(size_t)sub_index * 4], entry);
                        filed.push_back({sub_index, entry});
                    }
                }
            }
            long marked = 0, turned_away = 0;
            for (size_t sb = 0; sb < filt.size() / 4; ++sb) marked += filter_is_mark(slot(filt, (uint32_t)sb, 7));
            for (const Filed &f : filed) {
                bool there = false;
                for (int i = 0; i < 8; ++i) there = there || slot(filt, f.sub_index, i) == f.entry;
                if (there) continue;
                ++turned_away;
                const uint32_t s7 = slot(filt, f.sub_index, 7), sig = filter_mark_sig(f.entry >> 2) << 2;
                if (!filter_is_mark(s7) || (s7 & sig) != sig) { printf("(c) order %d: entry %04x of sub-bucket %u is lost (slot 7 = %04x)\n", order, f.entry, f.sub_index, s7); return 1; }
            }
            // slots fill in order and a mark only ever sits in slot 7
            for (size_t sb = 0; sb < filt.size() / 4; ++sb)
                for (int i = 0; i < 8; ++i) {
                    const uint32_t v = slot(filt, (uint32_t)sb, i);
                    if ((i < 7 && v && !(v & 3u)) || (i > 0 && v && !slot(filt, (uint32_t)sb, i - 1))) { printf("(c) order %d: sub-bucket %zu slot %d = %04x\n", order, sb, i, v); return 1; }
                }
            long sent_const = 0, sent_sig = 0;
            for (const Filed &f : strangers) {
                const uint32_t s7 = slot(filt, f.sub_index, 7), sig = filter_mark_sig(f.entry) << 2;
                if (!filter_is_mark(s7)) continue;
                ++sent_const;                                   // (a stranger matches no slot: the filing is a bijection)
                sent_sig += (s7 & sig) == sig;
            }
            printf("(c) order %d: %ld marked sub-buckets, %ld entries turned away; of %zu never-filed windows a constant mark sends on %.4f %%, the signature %.4f %%\n",
                   order, marked, turned_away, strangers.size(), 100.0 * sent_const / strangers.size(), 100.0 * sent_sig / strangers.size());
            if (marked < 500 || turned_away < marked) { printf("(c) order %d: too few overflows to test anything\n", order); return 1; }
            if (!(sent_sig < sent_const)) { printf("(c) order %d: the signature does not help\n", order); return 1; }
        }
    }

    // (d) a mark never compares as a hit, whatever the window's stored bits (finish(): the largest halfword of slot ^ fpw is >= 0xFFFD on a hit)
    for (uint32_t c = 0; c < (1u << 14); ++c) {
        const uint32_t fpw = mul24(c ^ 0x3FFFu, 0x00040004u);
        if ((fpw >> 16) != (fpw & 0xFFFFu) || (~(fpw >> 2) & 0x3FFFu) != c) { printf("(d) fpw of %u\n", c); return 1; }
        for (uint32_t sig14 = 1; sig14 < (1u << 14); ++sig14)
            if ((((sig14 << 2) ^ fpw) & 0xFFFFu) >= 0xFFFDu) { printf("(d) mark %04x hits stored bits %u\n", sig14 << 2, c); return 1; }
        const uint32_t sig = filter_mark_sig(c);
        if (sig == 0 || sig > 0x3FFFu || __builtin_popcount(sig) != 2) { printf("(d) signature of %u = %x\n", c, sig); return 1; }
        for (uint32_t tags = 1; tags <= 3; ++tags)
            if ((((filter_exact_entry(c, tags)) ^ fpw) & 0xFFFFu) < 0xFFFDu || filter_is_mark(filter_exact_entry(c, tags))) { printf("(d) entry %u\n", c); return 1; }
    }
    if (filter_is_mark(0) || !filter_is_mark(kFilterOverflowMark)) { printf("(d) filter_is_mark\n"); return 1; }
    printf("ok %ld keys, %ld windows\n", n_keys, n_windows);
    return 0;
}
