// tmer_rank_search.cpp -- design tool, not product code: searches the order of the 4096 6-mers INSIDE their open-closed class
// (hast_common.h, tmer_class) for the mod-minimizer of the fingerprint filter, and writes the result as the level table that
// tmer_order reads (hast_amd/csrc/tmer_level_table.h).
//
// Model.  Runs of windows that sample one m-mer are what k_classify_f pays an HBM request for (profiles/tmer_order_sim.txt):
// on a random string, runs per read = 1 + (P - 1) x density, where P is the windows of a read (130 at K = 21, 120 at K = 31)
// and density the fraction of consecutive windows whose sampled m-mer position differs.  A window's first kp bases hold
// nt = kp - t + 1 t-mers; the smallest by the order (leftmost on ties) at offset j samples the m-mer at j mod W.
//
// Order under search: a 4-bit LEVEL per t-mer, class-major (class 0 = open, 1 = closed, 2 = the rest get the level ranges
// [0, a), [a, b), [b, 16)), then a fixed bijective hash of the t-mer, then the position: the key of tmer_order_lvl.
//
// Search.  Simulated annealing over the levels, one t-mer at a time, from the open-closed start (every t-mer at its class's
// first level).  A visit evaluates ALL levels of the t-mer at once and only on the windows it touches (each occurrence in the
// training string +- nt windows): a window the t-mer is in is won by it below a threshold level and by the best other t-mer
// above it, so every transition's change is a step function of the level.  The level is drawn with probability
// exp(-objective / temperature); the temperature falls geometrically, and greedy sweeps (temperature 0) finish.  The training
// string is 16 fixed segments (threads <= 16 take them in turn, so the result does not depend on the thread count).
// Objective: C3's runs per read (K = 21, m = 14, kp = 21: W = 8, 16 t-mers per window) plus w5 x config 5's (K = 31, m = 15,
// kp = 23: W = 9, 18 t-mers).  Held-out strings (another seed) report both geometries for the hash order, open-closed, the
// search result and -- with --levels 256, the same search with 256 levels -- the order before quantising.
//
//   g++ -O2 -std=c++20 -pthread -o tmer_rank_search tools/sim/tmer_rank_search.cpp
//   tmer_rank_search [--train MBP] [--test MBP] [--sweeps N] [--greedy N] [--t0 T] [--t1 T] [--split a,b] [--levels 16|256]
//                    [--w5 W] [--threads N] [--seed S] [--out HEADER] [--eval-only]
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../../hast_amd/csrc/hast_common.h"
using namespace hast;

namespace {

constexpr int kSegs = 16;
struct Geo { int nt, W, P; };                       // t-mers per window, m-mers per window, windows per read
constexpr Geo kGeo[2] = {{16, 8, 130}, {18, 9, 120}};

// the orders this tool knows, as a key per 6-mer (position bits 0): smaller wins, ties -> leftmost
std::vector<uint32_t> keys_hash() {                 // the multiplicative hash alone (the order before open-closed)
    std::vector<uint32_t> k(4096);
    for (uint32_t v = 0; v < 4096; ++v) k[v] = (mul24(v + 1u, 0x9E3779u) >> 12) << 12;
    return k;
}
std::vector<uint32_t> keys_oc() {                   // open-closed above that hash (the order before the level table)
    std::vector<uint32_t> k(4096);
    for (uint32_t v = 0; v < 4096; ++v) k[v] = (tmer_class(v) << 30) | ((mul24(v + 1u, 0x9E3779u) >> 14) << 12);
    return k;
}
std::vector<uint32_t> keys_table() {                // hast_common.h's tmer_order: the level table in the tree
    std::vector<uint32_t> k(4096);
    for (uint32_t v = 0; v < 4096; ++v) k[v] = tmer_order(v, 0);
    return k;
}
uint32_t key_of_level(uint32_t v, uint32_t lvl, int lvl_bits) {      // tmer_order_lvl's key, any level width
    return (lvl << (32 - lvl_bits)) | (tmer_hash12(v) << (32 - lvl_bits - 12));
}

// random string of n bases as its 6-mer values (tv[i] = bases i .. i+5)
std::vector<uint16_t> random_tmers(uint64_t seed, uint64_t seg, size_t n) {
    std::vector<uint16_t> tv(n - 5);
    uint32_t x = 0;
    uint64_t w = 0;
    for (size_t i = 0; i < n; ++i) {
        if ((i & 31) == 0) w = synth_rand(seed, seg, i >> 5);
        x = ((x << 2) | (uint32_t)((w >> (2 * (i & 31))) & 3u)) & 0xFFFu;
        if (i >= 5) tv[i - 5] = (uint16_t)x;
    }
    return tv;
}

// sampled m-mer position of window w (absolute): the smallest key | offset of its nt t-mers, offset mod W
inline uint32_t sample(const uint16_t *tv, const uint32_t *key, size_t w, const Geo &g) {
    uint32_t best = 0xFFFFFFFFu;
    for (int j = 0; j < g.nt; ++j) best = std::min(best, key[tv[w + j]] | (uint32_t)j);
    return (uint32_t)w + (best & 0xFFFu) % (uint32_t)g.W;
}

// runs per read of one geometry over a set of strings
double runs_per_read(const std::vector<std::vector<uint16_t>> &segs, const std::vector<uint32_t> &key, const Geo &g) {
    uint64_t ch = 0, tr = 0;
    for (const auto &tv : segs) {
        const size_t nw = tv.size() - g.nt + 1;
        uint32_t prev = sample(tv.data(), key.data(), 0, g);
        for (size_t w = 1; w < nw; ++w) {
            const uint32_t s = sample(tv.data(), key.data(), w, g);
            ch += s != prev;
            prev = s;
        }
        tr += nw - 1;
    }
    return 1.0 + (g.P - 1) * (double)ch / (double)tr;
}

// one training segment: its t-mers, where each 6-mer occurs, and the sampled position of every window per geometry
struct Seg {
    std::vector<uint16_t> tv;
    std::vector<uint32_t> occ_start, occ;            // occurrences of 6-mer v: occ[occ_start[v] .. occ_start[v+1])
    std::vector<uint32_t> samp[2];
    void init(std::vector<uint16_t> t) {
        tv = std::move(t);
        occ_start.assign(4097, 0);
        for (uint16_t v : tv) ++occ_start[v + 1];
        for (int v = 0; v < 4096; ++v) occ_start[v + 1] += occ_start[v];
        occ.resize(tv.size());
        std::vector<uint32_t> at(occ_start.begin(), occ_start.end() - 1);
        for (size_t i = 0; i < tv.size(); ++i) occ[at[tv[i]]++] = (uint32_t)i;
    }
    size_t nw(int gi) const { return tv.size() - kGeo[gi].nt + 1; }
    void resample(const uint32_t *key) {
        for (int gi = 0; gi < 2; ++gi) {
            samp[gi].resize(nw(gi));
            for (size_t w = 0; w < nw(gi); ++w) samp[gi][w] = sample(tv.data(), key, w, kGeo[gi]);
        }
    }
    // changed transitions over the windows v touches, for every level of v (cnt[gi][L], L < nlev)
    void count_levels(uint32_t v, const uint32_t *key, int lvl_bits, int nlev, std::vector<int64_t> *cnt) const {
        const uint32_t sh = 32 - lvl_bits, low = (1u << sh) - 1, vkey = key_of_level(v, 0, lvl_bits);
        for (int gi = 0; gi < 2; ++gi) {
            const Geo &g = kGeo[gi];
            const int64_t n = (int64_t)nw(gi);
            int64_t *c = cnt[gi].data();
            // affected windows: the union of [i - nt + 1, i] over the occurrences i (sorted), as intervals [a, b]
            const uint32_t *o = occ.data() + occ_start[v], *oe = occ.data() + occ_start[v + 1];
            std::vector<uint32_t> thr, sv, so;    // per window of the interval: v wins below level thr (v's sample sv, else so)
            // transition between windows with samples (L < t ? a : b): add (changed) to c[L] for every L (difference array)
            auto emit = [&](uint32_t t1, uint32_t a1, uint32_t b1, uint32_t t2, uint32_t a2, uint32_t b2) {
                const uint32_t lo = std::min(t1, t2), hi = std::max(t1, t2);
                auto at = [&](uint32_t L) { return (int64_t)((L < t1 ? a1 : b1) != (L < t2 ? a2 : b2)); };
                const uint32_t e1 = std::min<uint32_t>(lo, nlev), e2 = std::min<uint32_t>(hi, nlev);
                if (e1 > 0) { const int64_t x = at(0); c[0] += x; c[e1] -= x; }
                if (e2 > e1) { const int64_t x = at(lo); c[e1] += x; c[e2] -= x; }
                if ((uint32_t)nlev > e2) { const int64_t x = at(hi); c[e2] += x; c[nlev] -= x; }
            };
            while (o != oe) {
                const int64_t a = std::max<int64_t>(0, (int64_t)*o - g.nt + 1);
                int64_t b = (int64_t)*o;
                for (++o; o != oe && (int64_t)*o - g.nt + 1 <= b + 1; ++o) b = (int64_t)*o;
                b = std::min(b, n - 1);
                if (a > b) continue;
                thr.resize((size_t)(b - a + 1)); sv.resize(thr.size()); so.resize(thr.size());
                for (int64_t w = a; w <= b; ++w) {
                    uint32_t best = 0xFFFFFFFFu, jv = 0xFFFFFFFFu;
                    const uint16_t *t = tv.data() + w;
                    for (int j = 0; j < g.nt; ++j) {
                        if (t[j] == v) { if (jv == 0xFFFFFFFFu) jv = (uint32_t)j; }
                        else best = std::min(best, key[t[j]] | (uint32_t)j);
                    }
                    const size_t k = (size_t)(w - a);
                    sv[k] = (uint32_t)w + jv % g.W;
                    if (best == 0xFFFFFFFFu) { thr[k] = 1u << lvl_bits; so[k] = 0; }
                    else {
                        thr[k] = (best >> sh) + (((vkey | jv) & low) < (best & low) ? 1u : 0u);
                        so[k] = (uint32_t)w + (best & 0xFFFu) % g.W;
                    }
                }
                for (int64_t w = std::max<int64_t>(1, a); w <= std::min(b + 1, n - 1); ++w) {
                    const bool in1 = w - 1 >= a, in2 = w <= b;
                    const size_t k1 = (size_t)(w - 1 - a), k2 = (size_t)(w - a);
                    emit(in1 ? thr[k1] : 0, in1 ? sv[k1] : 0, in1 ? so[k1] : samp[gi][w - 1],
                         in2 ? thr[k2] : 0, in2 ? sv[k2] : 0, in2 ? so[k2] : samp[gi][w]);
                }
            }
        }
    }
};

struct Args {
    double train = 32, test = 8, t0 = 2e-3, t1 = 2e-5, w5 = 0.0;
    int sweeps = 12, greedy = 3, a = 6, b = 12, levels = 16, threads = 8;
    uint64_t seed = 1;
    std::string out;
    bool eval_only = false;
};

}  // namespace

int main(int argc, char **argv) {
    Args A;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        auto next = [&]() { if (i + 1 >= argc) { fprintf(stderr, "%s: value missing\n", s.c_str()); exit(2); } return std::string(argv[++i]); };
        if (s == "--train") A.train = atof(next().c_str());
        else if (s == "--test") A.test = atof(next().c_str());
        else if (s == "--sweeps") A.sweeps = atoi(next().c_str());
        else if (s == "--greedy") A.greedy = atoi(next().c_str());
        else if (s == "--t0") A.t0 = atof(next().c_str());
        else if (s == "--t1") A.t1 = atof(next().c_str());
        else if (s == "--w5") A.w5 = atof(next().c_str());
        else if (s == "--split") { const std::string v = next(); if (sscanf(v.c_str(), "%d,%d", &A.a, &A.b) != 2) return 2; }
        else if (s == "--levels") A.levels = atoi(next().c_str());
        else if (s == "--threads") A.threads = std::max(1, std::min(16, atoi(next().c_str())));
        else if (s == "--seed") A.seed = strtoull(next().c_str(), 0, 10);
        else if (s == "--out") A.out = next();
        else if (s == "--eval-only") A.eval_only = true;
        else { fprintf(stderr, "unknown argument %s\n", s.c_str()); return 2; }
    }
    const int lvl_bits = A.levels == 256 ? 8 : 4, nlev = 1 << lvl_bits;
    // class ranges, scaled to the level count: class c owns [lo[c], lo[c+1])
    const int lo[4] = {0, A.a * nlev / 16, A.b * nlev / 16, nlev};
    if (!(0 < lo[1] && lo[1] < lo[2] && lo[2] < nlev)) { fprintf(stderr, "bad split\n"); return 2; }

    // held-out strings: another seed, the same segment layout
    std::vector<std::vector<uint16_t>> test(kSegs);
    const size_t tseg = (size_t)(A.test * 1e6 / kSegs);
    for (int s = 0; s < kSegs; ++s) test[s] = random_tmers(A.seed * 1000003ull + 77, (uint64_t)s, tseg);
    auto report = [&](const char *name, const std::vector<uint32_t> &key) {
        const double r3 = runs_per_read(test, key, kGeo[0]), r5 = runs_per_read(test, key, kGeo[1]);
        printf("{\"order\": \"%s\", \"held_out_mbp\": %.1f, \"runs_per_read_c3\": %.3f, \"runs_per_read_c5\": %.3f}\n", name, A.test, r3, r5);
        fflush(stdout);
        return std::make_pair(r3, r5);
    };
    report("hash", keys_hash());
    report("oc", keys_oc());
    report("table", keys_table());
    if (A.eval_only) return 0;

    // training segments
    std::vector<Seg> seg(kSegs);
    const size_t nseg = (size_t)(A.train * 1e6 / kSegs);
    {
        std::vector<std::thread> th;
        for (int ti = 0; ti < A.threads; ++ti) th.emplace_back([&, ti] {
            for (int s = ti; s < kSegs; s += A.threads) seg[s].init(random_tmers(A.seed, (uint64_t)s, nseg));
        });
        for (auto &x : th) x.join();
    }
    std::vector<uint32_t> lvl(4096), key(4096);
    for (uint32_t v = 0; v < 4096; ++v) { lvl[v] = (uint32_t)lo[tmer_class(v)]; key[v] = key_of_level(v, lvl[v], lvl_bits); }
    uint64_t trans[2] = {0, 0};
    for (auto &s : seg) for (int gi = 0; gi < 2; ++gi) trans[gi] += s.nw(gi) - 1;
    const double wgt[2] = {(kGeo[0].P - 1) / (double)trans[0], A.w5 * (kGeo[1].P - 1) / (double)trans[1]};

    // sweeps: a random visiting order per sweep, temperature geometric from t0 to t1, then greedy
    const int total = A.sweeps + A.greedy;
    std::vector<std::vector<int64_t>> cnt((size_t)kSegs * 2, std::vector<int64_t>(nlev + 1));
    uint32_t cur_v = 0;
    double temp = 0;
    uint64_t rng = splitmix64(A.seed ^ 0x5ea4c4ull);
    uint64_t moved = 0;
    bool deciding = false;                          // (the barrier's completion runs at every phase: only one decides)
    auto decide = [&]() noexcept {                  // (barrier completion: one thread, all counts in)
        if (!deciding) return;
        deciding = false;
        const uint32_t v = cur_v, c = tmer_class(v);
        std::vector<double> obj(nlev, 0.0);
        for (int s = 0; s < kSegs; ++s)
            for (int gi = 0; gi < 2; ++gi) {
                int64_t run = 0;
                for (int L = 0; L < nlev; ++L) { run += cnt[(size_t)s * 2 + gi][L]; obj[L] += wgt[gi] * (double)run; }
            }
        int pick = (int)lvl[v];
        if (temp > 0) {
            double mn = 1e300;
            for (int L = lo[c]; L < lo[c + 1]; ++L) mn = std::min(mn, obj[L]);
            double z = 0;
            for (int L = lo[c]; L < lo[c + 1]; ++L) z += std::exp(-(obj[L] - mn) / temp);
            double u = (double)((rng = splitmix64(rng)) >> 11) * 0x1.0p-53 * z;
            for (int L = lo[c]; L < lo[c + 1]; ++L) { u -= std::exp(-(obj[L] - mn) / temp); if (u <= 0) { pick = L; break; } }
        } else {
            for (int L = lo[c]; L < lo[c + 1]; ++L) if (obj[L] < obj[pick] - 1e-12) pick = L;
        }
        moved += (uint32_t)pick != lvl[v];
        lvl[v] = (uint32_t)pick;
        key[v] = key_of_level(v, lvl[v], lvl_bits);
    };
    std::barrier sync(A.threads, decide);
    std::vector<uint32_t> order(4096);
    for (uint32_t v = 0; v < 4096; ++v) order[v] = v;
    std::vector<std::thread> th;
    for (int ti = 0; ti < A.threads; ++ti) th.emplace_back([&, ti] {
        for (int s = ti; s < kSegs; s += A.threads) seg[s].resample(key.data());
        for (int sw = 0; sw < total; ++sw) {
            if (ti == 0) {                           // (every thread is between barriers: nobody reads these now)
                temp = sw < A.sweeps ? A.t0 * std::pow(A.t1 / A.t0, A.sweeps > 1 ? (double)sw / (A.sweeps - 1) : 0.0) : 0.0;
                for (uint32_t i = 4095; i > 0; --i) std::swap(order[i], order[(rng = splitmix64(rng)) % (i + 1)]);
                moved = 0;
            }
            sync.arrive_and_wait();
            for (uint32_t k = 0; k < 4096; ++k) {
                const uint32_t v = order[k];
                if (ti == 0) { cur_v = v; deciding = true; }
                for (int s = ti; s < kSegs; s += A.threads) {
                    for (int gi = 0; gi < 2; ++gi) std::fill(cnt[(size_t)s * 2 + gi].begin(), cnt[(size_t)s * 2 + gi].end(), 0);
                    seg[s].count_levels(v, key.data(), lvl_bits, nlev, &cnt[(size_t)s * 2]);
                }
                sync.arrive_and_wait();              // decide(): lvl[v], key[v]
                for (int s = ti; s < kSegs; s += A.threads) {
                    Seg &g = seg[s];
                    for (int gi = 0; gi < 2; ++gi) {
                        const int nt = kGeo[gi].nt;
                        const int64_t n = (int64_t)g.nw(gi);
                        for (uint32_t q = g.occ_start[v]; q < g.occ_start[v + 1]; ++q)
                            for (int64_t w = std::max<int64_t>(0, (int64_t)g.occ[q] - nt + 1); w <= (int64_t)g.occ[q] && w < n; ++w)
                                g.samp[gi][w] = sample(g.tv.data(), key.data(), (size_t)w, kGeo[gi]);
                    }
                }
                sync.arrive_and_wait();              // (no segment is read for the next t-mer before all are updated)
            }
            if (ti == 0) {
                uint64_t ch[2] = {0, 0};
                for (auto &g : seg)
                    for (int gi = 0; gi < 2; ++gi)
                        for (size_t w = 1; w < g.nw(gi); ++w) ch[gi] += g.samp[gi][w] != g.samp[gi][w - 1];
                fprintf(stderr, "sweep %d temp %.2e moved %llu train c3 %.4f c5 %.4f\n", sw, temp, (unsigned long long)moved,
                        1.0 + wgt[0] * (double)ch[0], 1.0 + (kGeo[1].P - 1) * (double)ch[1] / (double)trans[1]);
            }
            sync.arrive_and_wait();
        }
    });
    for (auto &x : th) x.join();

    uint64_t ch[2] = {0, 0};
    for (auto &g : seg)
        for (int gi = 0; gi < 2; ++gi)
            for (size_t w = 1; w < g.nw(gi); ++w) ch[gi] += g.samp[gi][w] != g.samp[gi][w - 1];
    printf("{\"order\": \"searched\", \"levels\": %d, \"split\": [%d, %d], \"train_mbp\": %.1f, \"train_runs_per_read_c3\": %.3f, "
           "\"train_runs_per_read_c5\": %.3f}\n", nlev, lo[1], lo[2], A.train, 1.0 + wgt[0] * (double)ch[0],
           1.0 + (kGeo[1].P - 1) * (double)ch[1] / (double)trans[1]);
    const auto r = report(nlev == 16 ? "searched" : "searched_256", key);
    int hist[256] = {0};
    for (uint32_t v = 0; v < 4096; ++v) ++hist[lvl[v]];
    printf("level_counts:");
    for (int L = 0; L < nlev; ++L) printf(" %d", hist[L]);
    printf("\n");

    if (!A.out.empty()) {
        if (nlev != 16) { fprintf(stderr, "--out needs --levels 16\n"); return 2; }
        FILE *f = fopen(A.out.c_str(), "w");
        if (!f) { perror(A.out.c_str()); return 1; }
        std::string cmd = "tmer_rank_search";
        for (int i = 1; i < argc; ++i) if (strcmp(argv[i], "--out") && (i == 1 || strcmp(argv[i - 1], "--out"))) cmd += std::string(" ") + argv[i];
        fprintf(f, "// tmer_level_table.h -- GENERATED by tools/sim/tmer_rank_search.cpp; do not edit.\n"
                   "//   %s --out hast_amd/csrc/tmer_level_table.h\n"
                   "// The level of every 6-mer (class-major: class 0 = levels [0, %d), class 1 = [%d, %d), class 2 = [%d, 16)), 4 bits each,\n"
                   "// 8 t-mers per word: t-mer v at bits 4 (v & 7) of word v >> 3.  Held out (%.0f Mbp): %.3f runs per 150-bp read at\n"
                   "// K = 21 / W = 8, %.3f at K = 31 / W = 9 (config 5).\n"
                   "#pragma once\n#include <stdint.h>\n\nnamespace hast {\n\n"
                   "constexpr uint32_t kTmerLevelClass1 = %d, kTmerLevelClass2 = %d;       // the first level of class 1 / 2\n"
                   "constexpr uint32_t kTmerLevelWords[512] = {\n",
                cmd.c_str(), lo[1], lo[1], lo[2], lo[2], A.test, r.first, r.second, lo[1], lo[2]);
        for (int w = 0; w < 512; ++w) {
            uint32_t x = 0;
            for (int i = 0; i < 8; ++i) x |= lvl[8 * w + i] << (4 * i);
            fprintf(f, "%s0x%08xu,%s", w % 8 ? " " : "    ", x, w % 8 == 7 ? "\n" : "");
        }
        fprintf(f, "};\n\n}  // namespace hast\n");
        fclose(f);
    }
    return 0;
}
