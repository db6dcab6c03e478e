// record_gather.h -- records gathered to their places, a wave per record: the copy of k_route_copy (routed records into four runs),
// k_rs_names (read names) and k_sq_copy (FASTQ sequences).  Every lane of a workgroup of 256 works out where ONE record lies and where
// it goes, these are staged in LDS, then each wave copies its 64 records one after the other, 64 bytes a step.  For records of tens to
// hundreds of bytes; items of any length: span_copy.h.
// The contract of record_gather_lane, which the kernels and tests/native/test_record_gather.cpp both step:
//   src[256], dst[256], n[256]   item i of the tile is the n[i] bytes at in + src[i] and goes to out + dst[i]
//   live                    items 0 .. live - 1 exist (256 or more: all); src, dst and n of the others are not looked at
//   wave, lane              wave w (0..3) copies the items 64 w .. 64 w + 63 that exist, lane l (0..63) bytes l, l + 64, ... of each
//   Policy::kNewlineEnds    true: the LAST byte of every item is '\n' (k_sq_copy: a sequence and the newline that ends it) and the
//                           source byte in its place is not read: an item of length 1 is '\n' and has no source
// An item of length 0 copies nothing, wherever it stands.  Nothing outside [in + src[i], in + src[i] + n[i]) is read and nothing
// outside [out + dst[i], out + dst[i] + n[i]) is written; destinations do not overlap, so the calls may run in any order.
// k_tx_copy (tx_kernels.hip) stays out: its bytes come out of rec1_byte / rec2_byte, it writes two outputs and stages a plan per pair.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define GATHER_HD __host__ __device__ __forceinline__
#else
#define GATHER_HD inline
#endif

namespace hast {

struct GatherBytes { static constexpr bool kNewlineEnds = false; };      // the item as it lies
struct GatherLines { static constexpr bool kNewlineEnds = true; };       // ends with '\n'

template <class Policy>
GATHER_HD void record_gather_lane(const uint8_t *in, uint8_t *out, const uint32_t *src, const uint32_t *dst, const uint32_t *n, uint32_t live, uint32_t wave,
                                  uint32_t lane) {
    const uint32_t first = wave * 64;
    const uint32_t in_wave = live > first ? (live - first < 64 ? live - first : 64) : 0;
    for (uint32_t r = 0; r < in_wave; ++r) {
        const uint32_t i = first + r, k = n[i];
        const uint8_t *s = in + src[i];
        uint8_t *d = out + dst[i];
        if constexpr (Policy::kNewlineEnds) {
            for (uint32_t b = lane; b + 1 < k; b += 64) d[b] = s[b];
            if (k && lane == ((k - 1) & 63)) d[k - 1] = '\n';
        } else {
            for (uint32_t b = lane; b < k; b += 64) d[b] = s[b];
        }
    }
}

#if defined(__HIPCC__) || defined(__CUDACC__)
// Workgroup of 256, once per tile, every thread: this lane's record (len = 0: none) joins the tile, then the tile is copied.  Two
// barriers inside, behind the staging and behind the copy.
template <class Policy>
__device__ __forceinline__ void record_gather_256(const uint8_t *in, uint8_t *out, uint32_t src, uint32_t dst, uint32_t len, uint32_t live) {
    __shared__ uint32_t s_src[256], s_dst[256], s_n[256];
    s_src[threadIdx.x] = src;
    s_dst[threadIdx.x] = dst;
    s_n[threadIdx.x] = len;
    __syncthreads();
    record_gather_lane<Policy>(in, out, s_src, s_dst, s_n, live, threadIdx.x >> 6, threadIdx.x & 63);
    __syncthreads();
}
#endif

}  // namespace hast
