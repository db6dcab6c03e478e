// classify_plan.h -- the PLAN of one classify launch (hast_api.cpp, classify_rows): the row shape, the reads a workgroup's tile holds,
// the dynamic LDS that tile takes (classify_tile.h), the exact multiply-high divisors of the kernels' index arithmetic and the grid.
// Host-only integer code, no HIP: tests/native/test_classify_plan.cpp steps it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hast_common.h"
#include "classify_tile.h"

namespace hast {
namespace classify {

constexpr uint32_t kSegWindows = 482;     // + K-1 <= 513 bases per segment row for K <= 32
constexpr uint32_t kLongRead = 4096;      // longer reads go through the segmented path: a row's positions must fit the 12 bits tmer_order gives them

// 5 / 8 workgroups per CU; k_classify_f's static 2 KB (the t-mer level table) comes off its share (150-bp reads: 35 reads
// per tile, 31768 B in all, as with the 1-KB class table before it)
constexpr size_t kLevelTableBytes = (size_t)kTmerLevelTableWords * 4;
constexpr size_t kLdsBudgetFilter = (size_t)32000 - kLevelTableBytes, kLdsBudgetExact = 19968;
constexpr size_t kLdsMax = (size_t)160 << 10;      // what a workgroup can have at all

struct Plan {
    uint32_t max_pos, mh_stride, w64, l1_stride, tile_reads;      // ClassifyArgs' fields of the same names
    uint32_t div_magic, div_mh, div_hw, div_l1g;
    size_t smem;                                                  // dynamic LDS of the launch
    int grid;
    bool fits;                                                    // false: the tile needs more LDS than a workgroup can have (smem says how much)
};

// __umulhi(q, magic) == q / d for every q the kernel forms (exact while q*d < 2^32)
inline uint32_t magic(uint64_t qmax, uint32_t d) {
    if (d <= 1 || qmax * d >= (1ull << 32)) return 0;
    return (uint32_t)((1ull << 32) / d) + 1;
}

// fg is read only with use_filter; lds_override (the tile_lds option) replaces the budget when it is not 0
inline Plan plan_for(int k, int m, uint32_t read_len, bool strict, bool use_filter, const FilterGeom &fg, size_t lds_override, int n_cu, uint64_t n_reads) {
    Plan p;
    p.max_pos = read_len >= (uint32_t)k ? read_len - (uint32_t)k + 1 : 0;
    p.mh_stride = read_len >= (uint32_t)m ? read_len - (uint32_t)m + 1 : 0;
    p.w64 = (read_len + 31) / 32;
    p.l1_stride = use_filter ? l1_stride_for(read_len, (uint32_t)fg.t, fg.dense != 0) : 0;
    // a tile is affine in its reads: what 0 reads take, and what every read adds
    auto bytes_of = [&](uint32_t tr) {
        return use_filter ? FilterTile{tr, p.w64, p.l1_stride, strict}.bytes() : ExactTile{tr, p.w64, p.mh_stride, strict}.bytes((uint32_t)(k - m + 1));
    };
    const size_t pad = bytes_of(0), per_read = bytes_of(1) - pad;
    // Reads per tile: at most what fits the LDS budget of a workgroup and at most 64; among the
    // candidates take the one whose windows fill the waves' 64-window blocks best (a workgroup walks
    // 4 waves x 2 blocks per iteration: 150-bp reads => 31 reads = 4030 windows = 63 of 64 block slots).
    const size_t lds_budget = lds_override ? lds_override : (use_filter ? kLdsBudgetFilter : kLdsBudgetExact);
    const size_t fit = lds_budget > pad + per_read ? (lds_budget - pad) / per_read : 1;
    const uint32_t tr_max = (uint32_t)(fit > 64 ? 64 : fit < 1 ? 1 : fit);
    uint32_t tr = tr_max;
    if (p.max_pos > 0) {
        double best = -1;
        for (uint32_t t = tr_max; t >= 1 && t + 8 > tr_max; --t) {
            const uint64_t q = (uint64_t)t * p.max_pos, blocks = (q + 63) / 64, slots = use_filter ? (blocks + 3) / 4 * 4 : (blocks + 7) / 8 * 8;
            const double eff = (double)q / (double)(slots * 64);
            if (eff > best + 1e-9) { best = eff; tr = t; }
        }
    }
    p.tile_reads = tr;
    p.smem = bytes_of(tr);
    p.fits = p.smem + (use_filter ? kLevelTableBytes : 0) <= kLdsMax;
    p.div_magic = magic((uint64_t)tr * p.max_pos + 1024, p.max_pos);
    p.div_mh = magic((uint64_t)tr * p.mh_stride + 1024, p.mh_stride);
    p.div_hw = magic((uint64_t)tr * p.w64 * 2 + 1024, p.w64 * 2);
    p.div_l1g = magic((uint64_t)tr * (p.l1_stride / 4) + 1024, p.l1_stride / 4);
    const uint64_t n_tiles = (n_reads + tr - 1) / tr, cap = (uint64_t)n_cu * 8;
    p.grid = (int)(n_tiles < cap ? n_tiles : cap);
    return p;
}

}  // namespace classify
}  // namespace hast
