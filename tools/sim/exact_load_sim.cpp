// exact_load_sim.cpp -- design tool, not product code: load of the EXACT-entry filter (hast_common.h) for random and for clustered
// keys (synth_key, reserved = 1: runs of K windows around variant sites), one slice of the blocks: sub-bucket histogram and the
// share of random read windows that land in a FULL sub-bucket, and in a MARKED one (a ninth entry came: those ask the exact table).
//   exact_load_sim keys_per_hap clustered(0/1) [dense(0/1) [levers(0/1)]]
// dense = 0 models the sampled scheme (a string filed once per strand, under filter_sample_pos; windows probe there), dense = 1 dense
// filing (a string under each of its W m-mers; a probing window is a random string at a random position of the row's grid).
// levers = 1 (with dense = 1) files the same keys a second time by POSITION (filter_dense_code: sub-bucket = pm, the product's
// placement) next to the hashed placement above, keeps for both the SIGNATURE a mark would carry (filter_mark_sig of every entry
// turned away, the one slot 7 held included) and prints the 2 x 2 table: windows per read that must ask the exact table with a
// constant mark / a signed mark, sub-bucket by hash / by position.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include "../../hast_amd/csrc/hast_common.h"
using namespace hast;
int main(int argc, char **argv) {
    const uint64_t n_per_hap = strtoull(argv[1], 0, 10);
    const int clustered = atoi(argv[2]), dense = argc > 3 ? atoi(argv[3]) : 0, levers = (argc > 4 && dense) ? atoi(argv[4]) : 0, threads = 8;
    const uint32_t SLICE = 64;
    const int K = 21;
    FilterGeom g = filter_geom_for(K, 2 * n_per_hap, 0, 0, 0, 1);
    const uint32_t W = filter_w(g);
    if (dense && (W & (W - 1))) { printf("dense filing needs W a power of two\n"); return 1; }
    SynthParams p{0x4841535401ull, 0x4841535402ull, 0x4841535403ull, n_per_hap, 1000, 150, (uint32_t)K, (uint32_t)(clustered ? 1 : 0)};
    const uint64_t nb = filter_nblocks(g), nslice = nb / SLICE;
    std::vector<std::atomic<uint8_t>> cnt(nslice * 8);
    for (auto &c : cnt) c = 0;
    // levers: [0] = the hashed placement (its counts are `cnt`), [1] = by position; per sub-bucket the stored bits of the entry in
    // slot 7 (| 0x8000 once known) and the signature of the entries turned away
    const uint32_t PB = (uint32_t)filter_pos_bits(g);
    std::vector<std::atomic<uint8_t>> cnt_pos(levers ? nslice * 8 : 0);
    std::vector<std::atomic<uint16_t>> slot7[2], sig[2];
    for (int v = 0; v < 2; v++) {
        slot7[v] = std::vector<std::atomic<uint16_t>>(levers ? nslice * 8 : 0);
        sig[v] = std::vector<std::atomic<uint16_t>>(levers ? nslice * 8 : 0);
        for (auto &x : slot7[v]) x = 0;
        for (auto &x : sig[v]) x = 0;
    }
    for (auto &c : cnt_pos) c = 0;
    auto sign = [&](int v, uint64_t sub, uint32_t c14, uint8_t before) {          // `before`: entries the sub-bucket held when this one came
        if (before == 7) slot7[v][sub] = (uint16_t)(c14 | 0x8000u);
        if (before >= 8) sig[v][sub] |= (uint16_t)filter_mark_sig(c14);
        if (before == 8) {                                                        // the ninth: slot 7's entry is turned away with it
            uint16_t e;
            while (!((e = slot7[v][sub].load()) & 0x8000u)) std::this_thread::yield();
            sig[v][sub] |= (uint16_t)filter_mark_sig(e & 0x3FFFu);
        }
    };
    std::atomic<uint64_t> filed{0}, lost{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) th.emplace_back([&, t] {
        for (int h = 0; h < 2; h++)
            for (uint64_t j = t; j < n_per_hap; j += threads) {
                const uint64_t key = synth_key(p, h, j);
                for (int o = 0; o < 2; o++) {
                    const uint64_t s = o ? kmer_revcomp(key, K) : key;
                    if (o && s == key) break;
                    const uint32_t pm0 = dense ? 0u : filter_sample_pos(s, g), pm1 = dense ? W : pm0 + 1u;
                    for (uint32_t pm = pm0; pm < pm1; pm++) {
                        const uint32_t b = filter_block_of((uint32_t)(s >> (2 * (K - g.m - (int)pm))) & (uint32_t)kmer_mask(g.m), g.m);
                        if (b % SLICE) continue;
                        const uint32_t c17 = filter_exact_code(s, pm, g);
                        std::atomic<uint8_t> &c = cnt[(uint64_t)(b / SLICE) * 8 + filter_exact_sub(c17)];
                        // (duplicates -- the same string from both haplotypes -- would be one entry; ignored here)
                        // 0 .. 8 entries; 9 = the ninth came: slot 7 becomes the overflow mark, the entry it held is turned away too
                        uint8_t v = c.load();
                        while (v < 9 && !c.compare_exchange_weak(v, (uint8_t)(v + 1))) {}
                        if (v >= 8) lost += v == 8 ? 2 : 1; else filed++;
                        if (levers) {
                            sign(0, (uint64_t)(b / SLICE) * 8 + filter_exact_sub(c17), c17 & 0x3FFFu, v);
                            const uint32_t d17 = filter_dense_code(s, pm, g, PB);
                            const uint64_t sub = (uint64_t)(b / SLICE) * 8 + filter_exact_sub(d17);
                            uint8_t u = cnt_pos[sub].load();
                            while (u < 9 && !cnt_pos[sub].compare_exchange_weak(u, (uint8_t)(u + 1))) {}
                            sign(1, sub, d17 & 0x3FFFu, u);
                        }
                    }
                }
            }
    });
    for (auto &x : th) x.join();
    uint64_t hist[10] = {0};
    for (auto &c : cnt) hist[(int)c]++;
    // random windows
    std::atomic<uint64_t> in_slice{0}, full{0}, marked{0};
    std::atomic<uint64_t> sent[2][2];                                   // [placement][0 = constant mark, 1 = signed mark]
    for (auto &r : sent) for (auto &x : r) x = 0;
    th.clear();
    for (int t = 0; t < threads; t++) th.emplace_back([&, t] {
        for (uint64_t i = t; i < 40000000ull; i += threads) {
            const uint64_t s = synth_rand(99, i, 7) & kmer_mask(K);
            const uint32_t pm = dense ? filter_dense_pm((uint32_t)synth_rand(98, i, 7), W) : filter_sample_pos(s, g);
            const uint32_t b = filter_block_of((uint32_t)(s >> (2 * (K - g.m - (int)pm))) & (uint32_t)kmer_mask(g.m), g.m);
            if (b % SLICE) continue;
            in_slice++;
            const uint8_t v = cnt[(uint64_t)(b / SLICE) * 8 + filter_exact_sub(filter_exact_code(s, pm, g))];
            if (v >= 8) full++;
            if (v >= 9) marked++;
            if (levers)
                for (int pl = 0; pl < 2; pl++) {
                    const uint32_t c17 = pl ? filter_dense_code(s, pm, g, PB) : filter_exact_code(s, pm, g);
                    const uint64_t sub = (uint64_t)(b / SLICE) * 8 + filter_exact_sub(c17);
                    if ((pl ? cnt_pos[sub].load() : cnt[sub].load()) < 9) continue;
                    const uint16_t ws = (uint16_t)filter_mark_sig(c17 & 0x3FFFu);
                    sent[pl][0]++;
                    if ((sig[pl][sub].load() & ws) == ws) sent[pl][1]++;
                }
        }
    });
    for (auto &x : th) x.join();
    filed -= hist[9];                                                   // (the entry a mark overwrote)
    printf("clustered=%d dense=%d m=%d filed/block %.2f lost %.5f hist", clustered, dense, g.m, (double)filed / nslice, (double)lost / (double)(lost + filed));
    for (int i = 0; i <= 9; i++) printf(" %llu", (unsigned long long)hist[i]);
    printf("  windows in a full sub-bucket: %.5f = %.2f per 130-window read, in a marked one: %.5f = %.2f per read\n", (double)full / in_slice,
           130.0 * full / in_slice, (double)marked / in_slice, 130.0 * marked / in_slice);
    if (levers) {
        uint64_t hp[10] = {0};
        for (auto &c : cnt_pos) hp[(int)c]++;
        printf("  by position: hist");
        for (int i = 0; i <= 9; i++) printf(" %llu", (unsigned long long)hp[i]);
        printf("\n  windows per 130-window read that ask the table   constant mark   signed mark\n");
        for (int pl = 0; pl < 2; pl++)
            printf("    sub-bucket by %-8s                                %8.3f      %8.3f\n", pl ? "position" : "hash", 130.0 * sent[pl][0] / in_slice, 130.0 * sent[pl][1] / in_slice);
    }
}
