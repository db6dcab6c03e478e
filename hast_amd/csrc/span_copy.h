// span_copy.h -- items compacted into one output, the work split by OUTPUT bytes: the copy of k_rs_copy (FASTA lines into a base
// buffer), k_sqfa_copy (FASTA lines into the counter's stream) and k_rb_copy (records into three runs).  An item is anything from
// an empty line to one line of 10^8 bases: a lane or a wave per item would serialise the long ones and starve on the short ones.  So
// a workgroup owns kSpanCopyTile bytes of the destination at a time, finds by binary search in a monotone offset table the first and
// the last item that reach into them, and every lane moves the up to 16 bytes of its 16-byte aligned piece that lie inside the
// output: it looks its first item up between those two and walks on from there -- one 16-byte load as the source lies and one aligned
// 16-byte store where one item supplies the whole piece, byte by byte across item ends and at both ends of the output.
//
// The contract of span_copy_lane, which the kernels and tests/native/test_span_copy.cpp both step:
//   dst[first .. last + 1]  monotone; item j emits the bytes [dst[j], dst[j + 1]) - bias of the output, so an item with dst[j] ==
//                           dst[j + 1] emits nothing and is skipped wherever it stands: in front, in runs, between two that emit, at
//                           the end.  dst[first] <= bias and dst[last + 1] >= total + bias: the last item need not emit, and items
//                           may lie behind the output.  What they would emit at or behind `total` is neither read nor written.
//   bias                    table values in front of the output's first byte (k_rs_copy: the sequence bytes in front of the view's
//                           first header)
//   out = out16 + olo       out16 16-byte aligned, olo in 0..15; total >= 1 (an empty output is the caller's early exit)
//   src.at(j)               the first source byte of item j; asked only of items that emit into the lane's piece.  Byte i of the item
//                           is at(j)[i], and no load leaves [at(j), at(j) + dst[j + 1] - dst[j]): nothing outside the view is read.
//   Src::kFills, src.fill(at(j))   with kFills, an item for which fill() holds is one byte long and emits '\n'; of its source only
//                           what fill() looks at is read
// Every byte of [out, out + total) is written by exactly one (tile, lane), in any order of the calls; nothing in front of out and
// nothing at or behind out + total is written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define SPAN_HD __host__ __device__ __forceinline__
#else
#define SPAN_HD inline
#endif

namespace hast {

constexpr uint32_t kSpanCopyTile = 4096;         // destination bytes a workgroup owns at a time = 256 lanes x 16 B (untuned)

// tiles of an output of `total` bytes that starts olo bytes into its first tile
SPAN_HD uint32_t span_copy_tiles(uint32_t total, uint32_t olo) { return (olo + total + kSpanCopyTile - 1) / kSpanCopyTile; }

// the smallest j in [lo, hi] with dst[j + 1] > v; the caller knows that item hi is one
SPAN_HD uint32_t span_first_past(const uint32_t *dst, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (dst[mid + 1] > v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the work of lane `lane` (0..255) on tile `tile` (< span_copy_tiles(total, olo))
template <class Src>
SPAN_HD void span_copy_lane(const uint32_t *dst, uint32_t first, uint32_t last, uint32_t bias, uint32_t total, uint8_t *out16, uint32_t olo, const Src &src,
                            uint32_t tile, uint32_t lane) {
    uint8_t *out = out16 + olo;
    const uint32_t q_end = olo + total;                          // q: offsets from out16, p: from out
    const uint32_t t0q = tile * kSpanCopyTile, t1q = q_end - t0q < kSpanCopyTile ? q_end : t0q + kSpanCopyTile;
    const uint32_t q = t0q + lane * 16, qs = q < olo ? olo : q;
    if (q >= t1q) return;
    const uint32_t qe = t1q - q < 16 ? t1q : q + 16;             // qs < qe: total >= 1, so the first piece reaches past olo
    uint32_t p = qs - olo;
    const uint32_t e = qe - olo, t0 = (t0q < olo ? olo : t0q) - olo, t1 = t1q - olo;
    const uint32_t j0 = span_first_past(dst, first, last, t0 + bias);
    const uint32_t j1 = span_first_past(dst, j0, last, t1 - 1 + bias);
    uint32_t j = span_first_past(dst, j0, j1, p + bias);
    while (p < e) {
        const uint32_t a = dst[j], b = dst[j + 1];
        if (b <= p + bias) {                                     // an item that emits nothing
            ++j;
            continue;
        }
        const uint32_t upto = b - bias < e ? b - bias : e, k = upto - p;
        const uint8_t *item = src.at(j), *s = item + (p + bias - a);
        bool fill = false;
        if constexpr (Src::kFills) fill = src.fill(item);
        if (fill) {
            out[p] = '\n';
        } else if (k == 16) {
            __builtin_memcpy(__builtin_assume_aligned(out + p, 16), s, 16);
        } else {
            for (uint32_t i = 0; i < k; ++i) out[p + i] = s[i];
        }
        p = upto;
        ++j;
    }
}

}  // namespace hast

#if defined(__HIPCC__) || defined(__CUDACC__)
namespace hast {

// Workgroups of 256, any grid: the whole copy.  No barrier inside.
template <class Src>
__device__ __forceinline__ void span_copy(const uint32_t *dst, uint32_t first, uint32_t last, uint32_t bias, uint32_t total, uint8_t *out16, uint32_t olo,
                                          const Src &src) {
    const uint32_t n_tiles = span_copy_tiles(total, olo);
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) span_copy_lane(dst, first, last, bias, total, out16, olo, src, tile, threadIdx.x);
}

}  // namespace hast
#endif
