// Host-only test of the searched t-mer levels (hast_amd/csrc/tmer_level_table.h, tools/sim/tmer_rank_search.cpp) and of the
// order k_classify_f forms from them (hast_common.h):
//   1. the nibble table, read through the kernel's index and shift (word (tm >> 3) & 511, bits 4 (tm & 7)), gives tmer_level,
//      and tmer_order is the level's class, the level, then tmer_order_lvl's hash and position bits -- for 6-mers and for
//      24-bit t-mers (of which only the low 12 bits count);
//   2. tmer_order_lvl (what the kernel compares) orders any two (t-mer, position) pairs exactly as tmer_order does;
//   3. every level's class is the t-mer's open-closed class (tmer_class), and the level bounds are monotone;
//   4. both orders are total on the 4096 6-mers at one position, and every level of every class is used.
#include <cstdio>
#include <set>

#include "../../hast_amd/csrc/hast_common.h"

using namespace hast;

static uint64_t rng_state = 0x1e7e1ull;
static uint64_t rnd() { return rng_state = splitmix64(rng_state); }

int main() {
    // 1, 2
    for (uint32_t i = 0; i < 400000; ++i) {
        const uint32_t tm = i < 4096 ? i : (uint32_t)(rnd() & 0xFFFFFFu), pos = (uint32_t)(rnd() & 4095u);
        const uint32_t lvl = (kTmerLevelWords[(tm >> 3) & 0x1FFu] >> ((tm << 2) & 31u)) & 15u;
        if (lvl != tmer_level(tm & 0xFFFu)) { printf("lds: tm=%u\n", tm); return 1; }
        const uint32_t o = tmer_order(tm, pos), ol = tmer_order_lvl(tm, pos, lvl);
        if ((o >> 30) != tmer_level_class(lvl) || ((o >> 26) & 15u) != lvl || (o & 0x03FFFFFFu) != (ol & 0x03FFFFFFu) ||
            (ol >> 28) != lvl || (o & 0xFFFu) != pos) {
            printf("layout: tm=%u pos=%u order %08x lvl-order %08x\n", tm, pos, o, ol);
            return 1;
        }
        const uint32_t tm2 = (uint32_t)(rnd() & (i & 1 ? 0xFFFu : 0xFFFFFFu)), pos2 = (uint32_t)(rnd() & 15u);
        const uint32_t o2 = tmer_order(tm2, pos2), ol2 = tmer_order_lvl(tm2, pos2, tmer_level(tm2 & 0xFFFu));
        if ((o < o2) != (ol < ol2) || (o == o2) != (ol == ol2)) { printf("orders differ: %u@%u %u@%u\n", tm, pos, tm2, pos2); return 1; }
    }
    // 3
    if (!(0 < kTmerLevelClass1 && kTmerLevelClass1 < kTmerLevelClass2 && kTmerLevelClass2 < 16)) { printf("level bounds\n"); return 1; }
    int used[16] = {0};
    for (uint32_t tm = 0; tm < 4096; ++tm) {
        const uint32_t lvl = tmer_level(tm);
        if (tmer_level_class(lvl) != tmer_class(tm)) { printf("class of level %u != class of t-mer %u\n", lvl, tm); return 1; }
        ++used[lvl];
    }
    for (uint32_t l = 1; l < 16; ++l)
        if (tmer_level_class(l) < tmer_level_class(l - 1)) { printf("level -> class not monotone at %u\n", l); return 1; }
    // 4
    std::set<uint32_t> a, b;
    for (uint32_t tm = 0; tm < 4096; ++tm) { a.insert(tmer_order(tm, 7)); b.insert(tmer_order_lvl(tm, 7, tmer_level(tm))); }
    if (a.size() != 4096 || b.size() != 4096) { printf("order: %zu / %zu distinct keys of 4096\n", a.size(), b.size()); return 1; }
    for (int l = 0; l < 16; ++l) if (!used[l]) { printf("level %d unused\n", l); return 1; }
    printf("ok levels");
    for (int l = 0; l < 16; ++l) printf(" %d", used[l]);
    printf("\n");
    return 0;
}
