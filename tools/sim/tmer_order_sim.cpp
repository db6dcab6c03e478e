// tmer_order_sim.cpp -- design tool, not product code: the fingerprint filter under a chosen t-mer ORDER of the mod-minimizer
// (hast_common.h, tmer_order).  Unscaled and whole: N random canonical K-mers are filed under the block of both orientations
// into a byte per sub-bucket of EVERY block (2 GB at m = 14; filter_load_sim.cpp's slice "block id % SLICE == 0" is a biased
// sample -- the low bits of a block id are a function of the m-mer's last bases, which the order favours), then random
// 150-bp reads are pushed through.  Reports per read:
//   runs         windows whose block differs from the previous window's (+ 1): one HBM request each at best
//   blocks64     distinct blocks per 64-window probe instruction (what the kernel asks for)
//   full         windows without a match that land in a full sub-bucket (two full ones with two choices): sent to the table
//   full_ovf     ... of which the sub-bucket had an insert rejected (exact entries: only these need the table once slot 7
//                holds the overflow mark; the rest are proven misses)
// orders: hash = the multiplicative hash alone (the order up to this tool), oc = open-closed classes (s = 3) above that hash
// (the order up to the level table), table = hast_common.h's tmer_order (open-closed classes, the searched levels inside
// them -- tmer_level_table.h, tools/sim/tmer_rank_search.cpp -- then a hash).
//   tmer_order_sim <hash|oc|table> N K m t kp exact(0/1) choices [threads]
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../../hast_amd/csrc/hast_common.h"
using namespace hast;

int main(int argc, char **argv) {
    if (argc < 9) { fprintf(stderr, "usage: tmer_order_sim <hash|oc|table> N K m t kp exact choices [threads]\n"); return 2; }
    const bool oc = !strcmp(argv[1], "oc"), table = !strcmp(argv[1], "table");
    if (!oc && !table && strcmp(argv[1], "hash")) { fprintf(stderr, "order: hash, oc or table\n"); return 2; }
    const uint64_t N = strtoull(argv[2], 0, 10);
    const int K = atoi(argv[3]), m = atoi(argv[4]), t = atoi(argv[5]), kp = atoi(argv[6]), exact = atoi(argv[7]), choices = atoi(argv[8]);
    const int threads = argc > 9 ? atoi(argv[9]) : 8;
    FilterGeom g = filter_geom_for(kp, 0, m, t, 0, exact ? 1 : 0);       // (1: exact entries filed once -- this tool models the SAMPLED scheme)
    if (exact && !g.exact) { fprintf(stderr, "exact entries do not fit this geometry\n"); return 2; }
    // filter_sample_pos with the order as a parameter (the window's first kp bases only)
    auto sample = [&](uint64_t s) {
        if (table) return filter_sample_pos(s >> (2 * (K - kp)), g);
        const uint32_t nt = filter_nt(g), tmask = (uint32_t)kmer_mask(t);
        uint32_t best = 0xFFFFFFFFu;
        for (uint32_t j = 0; j < nt; ++j) {
            const uint32_t tm = (uint32_t)(s >> (2 * (K - t - (int)j))) & tmask;
            const uint32_t e = oc ? (tmer_class(tm & 0xFFFu) << 30) | ((mul24(tm + 1u, 0x9E3779u) >> 14) << 12) | j
                                  : ((mul24(tm + 1u, 0x9E3779u) >> 12) << 12) | j;
            best = e < best ? e : best;
        }
        const uint32_t x = best & 0xFFFu;
        return x - ((x * g.wdiv) >> 16) * filter_w(g);
    };
    auto block_at = [&](uint64_t s, uint32_t p) {
        return filter_block_of((uint32_t)(s >> (2 * (K - m - (int)p))) & (uint32_t)kmer_mask(m), m);
    };
    const uint64_t nb = filter_nblocks(g);
    // a byte per sub-bucket: entries filed (0..8), or kOvf = full AND an insert was turned away
    constexpr uint8_t kOvf = 9;
    std::vector<std::atomic<uint8_t>> cnt(nb * 8);
    for (auto &c : cnt) c.store(0, std::memory_order_relaxed);
    auto load = [&](uint64_t i) { const uint8_t c = cnt[i].load(std::memory_order_relaxed); return c > 8 ? 8 : c; };
    auto insert = [&](uint64_t i) {              // true: filed
        uint8_t c = cnt[i].load(std::memory_order_relaxed);
        for (;;) {
            const uint8_t n = c < 8 ? c + 1 : kOvf;
            if (cnt[i].compare_exchange_weak(c, n, std::memory_order_relaxed)) return c < 8;
        }
    };
    std::atomic<uint64_t> lost{0}, filed{0};
    std::vector<std::thread> th;
    for (int ti = 0; ti < threads; ti++) th.emplace_back([&, ti] {
        uint64_t my_lost = 0, my_filed = 0;
        for (uint64_t i = ti; i < N; i += threads) {
            const uint64_t key = kmer_canon(synth_rand(77, 1, i) & kmer_mask(K), K);
            for (int o = 0; o < 2; o++) {
                const uint64_t s = o ? kmer_revcomp(key, K) : key;
                if (o && s == key) break;
                const uint32_t p = sample(s);
                const uint64_t base = (uint64_t)block_at(s, p) * 8;
                bool ok;
                if (exact) ok = insert(base + filter_exact_sub(filter_exact_code(s, p, g)));
                else {
                    const uint32_t h = filter_keyhash(s), s1 = filter_sub_of(h), s2 = filter_sub2_of(h);
                    uint32_t a = s1, b = s2;
                    if (choices == 2 && s2 != s1 && load(base + s2) < load(base + s1)) { a = s2; b = s1; }
                    ok = insert(base + a);
                    if (!ok && choices == 2 && b != a) ok = insert(base + b);
                }
                ok ? ++my_filed : ++my_lost;
            }
        }
        lost += my_lost;
        filed += my_filed;
    });
    for (auto &x : th) x.join();
    uint64_t hist[9] = {0}, novf = 0;
    for (uint64_t i = 0; i < cnt.size(); ++i) { const uint8_t c = cnt[i].load(std::memory_order_relaxed); hist[c > 8 ? 8 : c]++; novf += c == kOvf; }
    const int L = 150, nreads = 400000;
    std::atomic<uint64_t> full{0}, full_ovf{0}, runs{0}, blocks64{0};
    th.clear();
    for (int ti = 0; ti < threads; ti++) th.emplace_back([&, ti] {
        std::vector<uint32_t> blk(L);
        std::vector<uint8_t> code(L);
        for (int r = ti; r < nreads; r += threads) {
            for (int j = 0; j < L; j += 32) { uint64_t x = synth_rand(99, r, j); for (int q = 0; q < 32 && j + q < L; q++) code[j + q] = (x >> (2 * q)) & 3; }
            const int nw = L - K + 1;
            uint64_t my_runs = 0, my_full = 0, my_ovf = 0;
            for (int p = 0; p < nw; p++) {
                uint64_t fwd = 0;
                for (int i = 0; i < K; i++) fwd = (fwd << 2) | code[p + i];
                const uint32_t sp = sample(fwd), b = block_at(fwd, sp);
                blk[p] = b;
                my_runs += p == 0 || b != blk[p - 1];
                const uint64_t base = (uint64_t)b * 8;
                bool f, o;
                if (exact) {
                    const uint32_t sub = filter_exact_sub(filter_exact_code(fwd, sp, g));
                    f = load(base + sub) >= 8;
                    o = cnt[base + sub].load(std::memory_order_relaxed) == kOvf;
                } else {
                    const uint32_t h = filter_keyhash(fwd);
                    f = load(base + filter_sub_of(h)) >= 8;
                    o = cnt[base + filter_sub_of(h)].load(std::memory_order_relaxed) == kOvf;
                    if (choices == 2) {
                        f = f && load(base + filter_sub2_of(h)) >= 8;
                        o = f && (o || cnt[base + filter_sub2_of(h)].load(std::memory_order_relaxed) == kOvf);
                    }
                }
                my_full += f;
                my_ovf += o;
            }
            runs += my_runs;
            full += my_full;
            full_ovf += my_ovf;
            for (int i0 = 0; i0 < nw; i0 += 64) {
                std::vector<uint32_t> v(blk.begin() + i0, blk.begin() + std::min(nw, i0 + 64));
                std::sort(v.begin(), v.end());
                blocks64 += std::unique(v.begin(), v.end()) - v.begin();
            }
        }
    });
    for (auto &x : th) x.join();

    printf("{\"order\": \"%s\", \"N\": %llu, \"K\": %d, \"m\": %d, \"t\": %d, \"kp\": %d, \"W\": %u, \"exact\": %d, \"choices\": %d, "
           "\"filed_per_block\": %.3f, \"lost_frac\": %.6f, \"sub_hist_0..8\": [%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu], "
           "\"full_subs_overflowed_frac\": %.4f, \"runs_per_read\": %.3f, \"blocks64_per_read\": %.3f, "
           "\"full_per_read\": %.4f, \"full_overflowed_per_read\": %.4f}\n",
           argv[1], (unsigned long long)N, K, m, t, kp, filter_w(g), exact, choices, (double)filed / (double)nb,
           (double)lost / (double)(lost + filed), (unsigned long long)hist[0], (unsigned long long)hist[1], (unsigned long long)hist[2],
           (unsigned long long)hist[3], (unsigned long long)hist[4], (unsigned long long)hist[5], (unsigned long long)hist[6],
           (unsigned long long)hist[7], (unsigned long long)hist[8], hist[8] ? (double)novf / (double)hist[8] : 0.0,
           (double)runs / nreads, (double)blocks64 / nreads, (double)full / nreads, (double)full_ovf / nreads);
    return 0;
}
