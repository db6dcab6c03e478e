// test_classify_plan.cpp -- the plan of a classify launch (hast_amd/csrc/classify_plan.h) and the LDS tile of the two classify kernels
// (hast_amd/csrc/classify_tile.h) on their own, host only.  The serial model below is the arithmetic classify_rows carried before the
// two headers existed, as it stood (per_read, pad, the search for the reads per tile, magic): over a grid of K, minimizer, row length,
// strictness, filter, LDS override and reads the plan must give the model's tile_reads, smem, grid and four divisors and refuse where
// the model refuses.  Of the layout alone: arrays disjoint, aligned and inside bytes(), every pad at least what its reader reaches;
// of the divisors: __umulhi(q, magic) == q / d for every q up to qmax; of the search: the best fill, ties to the larger tile.
//   test_classify_plan      exit 0 and "classify plan ok: <plans> plans" on stderr; 1 and the first broken rule otherwise
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "../../hast_amd/csrc/classify_plan.h"

using namespace hast;

static int fails = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, "\n");                                \
            if (++fails > 20) exit(1);                            \
        }                                                         \
    } while (0)

// ---- the serial model: classify_rows' arithmetic before classify_plan.h -----------------------------------------
struct Model {
    uint32_t max_pos, mh_stride, w64, l1_stride, tile_reads, tr_max, div_magic, div_mh, div_hw, div_l1g;
    size_t smem;
    int grid;
    bool refused;
};
static Model model_for(int k, int m, uint32_t read_len, int strict, bool filt, const FilterGeom &fg, size_t tile_lds, int n_cu, uint64_t n_reads) {
    Model a;
    a.max_pos = read_len >= (uint32_t)k ? read_len - k + 1 : 0;
    a.mh_stride = read_len >= (uint32_t)m ? read_len - m + 1 : 0;
    a.w64 = (read_len + 31) / 32;
    size_t per_read, pad;
    if (filt) {
        a.l1_stride = fg.dense ? 0 : ((read_len >= (uint32_t)fg.t ? read_len - (uint32_t)fg.t + 1 : 0) + 1 + 3) & ~3u;
        per_read = (size_t)(a.w64 + 1) * 8 + 8 + 8 + 4 + 4 + (size_t)a.l1_stride * 4 + (strict ? (size_t)(2 * a.w64 + 1) * 4 : 0);
        pad = 16 + (size_t)4 * 128 * 3 * sizeof(uint32_t) + 64 * 4 + 64;
    } else {
        const uint32_t wlen = (uint32_t)(k - m + 1);
        a.l1_stride = 0;
        per_read = (size_t)(a.w64 + 1) * 8 + 8 + 8 + 4 + 4 + (size_t)a.mh_stride * 4 + (strict ? (size_t)(2 * a.w64 + 1) * 4 : 0);
        pad = (size_t)wlen * 4 + 64 + 64 + 16;
    }
    const size_t lds_budget = tile_lds ? tile_lds : (filt ? (size_t)32000 - (size_t)kTmerLevelTableWords * 4 : (size_t)19968);
    const uint32_t tr_max = (uint32_t)std::min<size_t>(64, std::max<size_t>(1, lds_budget > pad + per_read ? (lds_budget - pad) / per_read : 1));
    uint32_t tr = tr_max;
    if (a.max_pos > 0) {
        double best = -1;
        for (uint32_t t = tr_max; t >= 1 && t + 8 > tr_max; --t) {
            const uint64_t q = (uint64_t)t * a.max_pos, blocks = (q + 63) / 64, slots = filt ? (blocks + 3) / 4 * 4 : (blocks + 7) / 8 * 8;
            const double eff = (double)q / (double)(slots * 64);
            if (eff > best + 1e-9) { best = eff; tr = t; }
        }
    }
    a.tile_reads = tr;
    a.tr_max = tr_max;
    a.smem = per_read * tr + pad;
    a.refused = a.smem + (filt ? (size_t)kTmerLevelTableWords * 4 : 0) > (160u << 10);
    auto magic = [](uint64_t qmax, uint32_t d) -> uint32_t {
        if (d <= 1 || qmax * d >= (1ull << 32)) return 0;
        return (uint32_t)((1ull << 32) / d) + 1;
    };
    a.div_magic = magic((uint64_t)tr * a.max_pos + 1024, a.max_pos);
    a.div_mh = magic((uint64_t)tr * a.mh_stride + 1024, a.mh_stride);
    a.div_hw = magic((uint64_t)tr * a.w64 * 2 + 1024, a.w64 * 2);
    a.div_l1g = magic((uint64_t)tr * (a.l1_stride / 4) + 1024, a.l1_stride / 4);
    const uint64_t n_tiles = (n_reads + tr - 1) / tr;
    a.grid = (int)std::min<uint64_t>(n_tiles, (uint64_t)n_cu * 8);
    return a;
}

// ---- the divisors ------------------------------------------------------------------------------------------------
static std::set<std::pair<uint64_t, uint32_t>> g_divided;       // (qmax, d) pairs stepped already
static void check_magic(uint64_t qmax, uint32_t d, uint32_t got) {
    const bool zero = d <= 1 || qmax * d >= (1ull << 32);
    CHECK((got == 0) == zero, "qmax %llu d %u magic %u", (unsigned long long)qmax, d, got);
    if (!got || qmax >= (1ull << 22) || !g_divided.insert({qmax, d}).second) return;
    for (uint64_t q = 0; q <= qmax; ++q)
        if ((uint32_t)((q * got) >> 32) != (uint32_t)(q / d)) {
            CHECK(false, "q %llu d %u magic %u", (unsigned long long)q, d, got);
            return;
        }
}

// ---- the layouts -------------------------------------------------------------------------------------------------
struct Region { const char *name; size_t at, len, align; };
static void check_regions(const std::vector<Region> &r, size_t bytes, const char *what, uint32_t tr, uint32_t read_len) {
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].at % r[i].align == 0, "%s.%s at %zu, tr %u read_len %u", what, r[i].name, r[i].at, tr, read_len);
        CHECK(r[i].at + r[i].len <= (i + 1 < r.size() ? r[i + 1].at : bytes), "%s.%s overlaps, tr %u read_len %u", what, r[i].name, tr, read_len);
    }
}
static void check_filter_tile(const classify::Plan &p, const FilterGeom &fg, int k, uint32_t read_len, bool strict) {
    const FilterTile L{p.tile_reads, p.w64, p.l1_stride, strict};
    const size_t TR = p.tile_reads;
    const std::vector<Region> r = {{"tile", L.tile_at(), 8, 8},
                                   {"dirty", L.dirty_at(), 4, 4},
                                   {"l1", L.l1_at(), TR * p.l1_stride * 4, 16},
                                   {"pack", L.pack_at(), TR * L.ws() * 8, 8},
                                   {"vote", L.vote_at(), TR * 8, 8},
                                   {"off", L.off_at(), TR * 8, 8},
                                   {"len", L.len_at(), TR * 4, 4},
                                   {"flag", L.flag_at(), TR * 4, 4},
                                   {"queue", L.queue_at(), kQueueBytes, 4},
                                   {"inv", L.inv_at(), strict ? TR * L.iw() * 4 : 0, 4}};
    check_regions(r, L.bytes(), "filter", p.tile_reads, read_len);
    CHECK(L.bytes() == p.smem, "read_len %u", read_len);
    CHECK(p.l1_stride % 4 == 0 && L.l1_words() == TR * p.l1_stride + kL1PadWords && L.pack_at() - L.l1_at() == L.l1_words() * 4, "read_len %u", read_len);
    CHECK(L.pack_words() == TR * L.ws(), "read_len %u", read_len);
    // the queue of a wave: fewer than 64 entries waiting and up to 64 new ones
    CHECK(kQCap >= 63 + 64 && kQueueBytes == (size_t)4 * 3 * kQCap * 4, "queue");
    // window_bits takes a row's word p / 32 and the next one, the masks of a strict row likewise
    if (read_len) CHECK((read_len - 1) / 32 + 1 < L.ws() && (read_len - 1) / 32 + 1 < L.iw(), "read_len %u", read_len);
    if (!fg.dense && p.max_pos > 0) {
        // phase M stores 4 entries at q0 <= l1_stride - 4; a row holds an entry per t-mer position
        CHECK(p.l1_stride >= read_len - (uint32_t)fg.t + 1 + 1, "read_len %u", read_len);
        // the probe reads l1[p], l1[p + g], .. and l1[p + NT - g] for p < max_pos: inside the row, so inside the last row + kL1PadWords
        const size_t reach = (TR - 1) * p.l1_stride + (p.max_pos - 1) + (filter_nt(fg) - (uint32_t)fg.g) + 1;
        CHECK(reach <= TR * p.l1_stride && reach <= L.l1_words(), "read_len %u k %d", read_len, k);
    }
}
static void check_exact_tile(const classify::Plan &p, int k, int m, uint32_t read_len, bool strict) {
    const uint32_t W = (uint32_t)(k - m + 1);
    const ExactTile L{p.tile_reads, p.w64, p.mh_stride, strict};
    const size_t TR = p.tile_reads;
    const std::vector<Region> r = {{"tile", L.tile_at(), 8, 8},
                                   {"pack", L.pack_at(), TR * L.ws() * 8, 8},
                                   {"vote", L.vote_at(), TR * 8, 8},
                                   {"off", L.off_at(), TR * 8, 8},
                                   {"len", L.len_at(), TR * 4, 4},
                                   {"flag", L.flag_at(), TR * 4, 4},
                                   {"mh", L.mh_at(), TR * p.mh_stride * 4, 4},
                                   {"inv", L.inv_at(), strict ? TR * L.iw() * 4 : 0, 4}};
    check_regions(r, L.bytes(W), "exact", p.tile_reads, read_len);
    CHECK(L.bytes(W) == p.smem, "read_len %u", read_len);
    CHECK(L.mh_words() == TR * p.mh_stride + kMhGapWords && L.inv_at() - L.mh_at() == L.mh_words() * 4 && L.pack_words() == TR * L.ws(), "read_len %u", read_len);
    if (read_len) CHECK((read_len - 1) / 32 + 1 < L.ws() && (read_len - 1) / 32 + 1 < L.iw(), "read_len %u", read_len);
    // a window's minimum reads W entries at its position: the last window of the last row ends with the array ...
    if (p.max_pos > 0) CHECK((TR - 1) * p.mh_stride + (p.max_pos - 1) + W <= TR * p.mh_stride, "read_len %u k %d m %d", read_len, k, m);
    // ... and a lane without a window reads W entries from the start of the array, whatever the array holds: inside the tile
    CHECK(L.mh_at() + std::max<size_t>(TR * p.mh_stride, W) * 4 <= L.bytes(W), "read_len %u k %d m %d", read_len, k, m);
    if (!strict) CHECK(L.mh_at() + TR * p.mh_stride * 4 + kMhGapWords * 4 + (size_t)W * 4 + kTileTailBytes == L.bytes(W), "read_len %u", read_len);
}

// ---- the search for the reads per tile ---------------------------------------------------------------------------
static void fill_of(uint32_t t, uint32_t max_pos, bool filt, uint64_t *q, uint64_t *slots) {
    *q = (uint64_t)t * max_pos;
    const uint64_t blocks = (*q + 63) / 64;
    *slots = filt ? (blocks + 3) / 4 * 4 : (blocks + 7) / 8 * 8;
}
static void check_search(const classify::Plan &p, uint32_t tr_max, bool filt, uint32_t read_len) {
    CHECK(p.tile_reads >= 1 && p.tile_reads <= tr_max && p.tile_reads + 8 > tr_max, "tr %u of %u, read_len %u", p.tile_reads, tr_max, read_len);
    if (p.max_pos == 0) {
        CHECK(p.tile_reads == tr_max, "read_len %u", read_len);
        return;
    }
    uint64_t q0, s0;
    fill_of(p.tile_reads, p.max_pos, filt, &q0, &s0);
    for (uint32_t t = tr_max; t >= 1 && t + 8 > tr_max; --t) {
        uint64_t q, s;
        fill_of(t, p.max_pos, filt, &q, &s);
        // q / s against q0 / s0, exactly: no candidate fills better (beyond the search's 1e-9), a larger one fills strictly worse
        if (t > p.tile_reads) CHECK(q * s0 < q0 * s, "tr %u: %u fills no worse, read_len %u", p.tile_reads, t, read_len);
        else CHECK((double)q / (double)(s * 64) <= (double)q0 / (double)(s0 * 64) + 1e-9, "tr %u: %u fills better, read_len %u", p.tile_reads, t, read_len);
    }
}

int main() {
    const int n_cu = 256;
    size_t plans = 0, refusals = 0;
    for (int k : {1, 5, 21, 31, 32}) {
        const int m_default = k <= 16 ? k : std::max(16, k - 8);           // what a context takes without HAST_MINIMIZER
        for (int m : {m_default, std::max(1, k - 5), 1}) {                  // m = 1: W = K, past 16 for the long K
            const uint32_t K = (uint32_t)k;
            for (uint32_t read_len : {1u, K - 1, K, 31u, 32u, 33u, 100u, 150u, 512u + K - 1, 4096u}) {
                if (read_len == 0) continue;                                // (K = 1: no row of K - 1 bases)
                for (int strict = 0; strict < 2; ++strict)
                    for (int f = 0; f < 3; ++f) {                           // filter off, sparse with t = 6, dense
                        FilterGeom fg = filter_geom_for(k, 400000000ull, 0, 6, 0, 1);
                        if (f) {
                            fg.t = std::min(6, fg.m);
                            fg.g = std::min(4, fg.kp - fg.t + 1);
                            fg.dense = f == 2;
                        }
                        for (size_t lds : {(size_t)0, (size_t)4096, (size_t)160 << 10}) {
                            const uint32_t tr = classify::plan_for(k, m, read_len, strict != 0, f != 0, fg, lds, n_cu, 1).tile_reads;
                            for (uint64_t n_reads : {(uint64_t)1, (uint64_t)tr, (uint64_t)tr + 1, (uint64_t)10000000}) {
                                const classify::Plan p = classify::plan_for(k, m, read_len, strict != 0, f != 0, fg, lds, n_cu, n_reads);
                                const Model a = model_for(k, m, read_len, strict, f != 0, fg, lds, n_cu, n_reads);
#define AT "k %d m %d read_len %u strict %d filter %d lds %zu reads %llu", k, m, read_len, strict, f, lds, (unsigned long long)n_reads
                                CHECK(p.max_pos == a.max_pos && p.mh_stride == a.mh_stride && p.w64 == a.w64 && p.l1_stride == a.l1_stride, AT);
                                CHECK(p.tile_reads == a.tile_reads, AT);
                                CHECK(p.smem == a.smem, AT);
                                CHECK(p.grid == a.grid && p.grid >= 1 && (uint64_t)p.grid <= (uint64_t)n_cu * 8, AT);
                                CHECK(p.div_magic == a.div_magic && p.div_mh == a.div_mh && p.div_hw == a.div_hw && p.div_l1g == a.div_l1g, AT);
                                CHECK(p.fits == !a.refused, AT);
                                refusals += !p.fits;
                                ++plans;
                                if (n_reads != 1) continue;                 // the rest does not depend on the reads
                                if (f) check_filter_tile(p, fg, k, read_len, strict != 0);
                                else check_exact_tile(p, k, m, read_len, strict != 0);
                                check_search(p, a.tr_max, f != 0, read_len);
                                check_magic((uint64_t)p.tile_reads * p.max_pos + 1024, p.max_pos, p.div_magic);
                                check_magic((uint64_t)p.tile_reads * p.mh_stride + 1024, p.mh_stride, p.div_mh);
                                check_magic((uint64_t)p.tile_reads * p.w64 * 2 + 1024, p.w64 * 2, p.div_hw);
                                check_magic((uint64_t)p.tile_reads * (p.l1_stride / 4) + 1024, p.l1_stride / 4, p.div_l1g);
#undef AT
                            }
                        }
                    }
            }
        }
    }
    // the first-level stride, spelled out: what the kernels with the row length compiled in assume (150, 100 and 512 bases, t = 6)
    CHECK(l1_stride_for(150, 6, false) == 148 && l1_stride_for(100, 6, false) == 96 && l1_stride_for(512, 6, false) == 508, "l1 stride");
    CHECK(l1_stride_for(150, 6, true) == 0 && l1_stride_for(3, 6, false) == 4 && l1_stride_for(6, 6, false) == 4 && l1_stride_for(8, 6, false) == 4 && l1_stride_for(9, 6, false) == 8, "l1 stride");
    // the bench's rows: 150 bases, K = 21 through the filter with exact entries -> 35 reads in 31768 bytes less the level table
    {
        FilterGeom fg = filter_geom_for(21, 400000000ull, 0, 6, 0, 1);
        const classify::Plan p = classify::plan_for(21, 16, 150, false, true, fg, 0, n_cu, 48000000);
        CHECK(fg.t == 6 && p.l1_stride == 148 && p.max_pos == 130 && p.grid == n_cu * 8 && p.fits, "150-bp rows");
        CHECK(p.smem + classify::kLevelTableBytes <= 32000 && p.tile_reads >= 28 && p.tile_reads <= 35, "150-bp rows: %u reads, %zu B", p.tile_reads, p.smem);
    }
    // a refusal: 2^24 bases per row cannot fit
    CHECK(!classify::plan_for(21, 16, 1u << 24, false, false, FilterGeom{}, 0, n_cu, 1).fits, "2^24 bases");
    CHECK(refusals > 0, "the grid holds no refusal");
    if (fails) return 1;
    fprintf(stderr, "classify plan ok: %zu plans, %zu refused, %zu divisors stepped\n", plans, refusals, g_divided.size());
    return 0;
}
