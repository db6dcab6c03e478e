// scan_device.h -- the sums and prefix sums over a wave (64 lanes) and over a workgroup that the framing, routing and deflate
// kernels share (fq_, sq_, sq_fasta_, rs_, tx_ and dz_kernels.hip, nl_index.h).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hast {

// the sum of v over the wave, to every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// the sum of v over lanes 0 .. lane
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += u;
    }
    return v;
}

// Workgroup of 256: the sum of v over all its threads, to every thread.  s: 4 words of LDS; one __syncthreads inside, so every thread
// calls it, and a second call on the same words needs a barrier behind the reads of the first.
__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t *s) {
    const uint32_t c = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}

// Workgroup of 256: the sum of v over the threads in front of this one.  s_wave: 4 words of LDS; one __syncthreads inside, so every
// thread calls it, and a second call on the same s_wave needs a barrier behind the first.
__device__ __forceinline__ uint32_t block_exclusive_sum_256(uint32_t v, uint32_t *s_wave) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_sum(v, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = incl - v;
    for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
    return before;
}

// Workgroup of 1024: exclusive scan of v[0, n) in place (n: a few 10^4; every thread takes a run of the values); returns the total,
// to every thread.  s_part: 1024 words of LDS.
__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t *v, uint32_t n, uint32_t *s_part) {
    const uint32_t per = (n + 1023) / 1024, lo = threadIdx.x * per < n ? threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += v[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {                 // Hillis-Steele inclusive scan
        const uint32_t x = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0;
        __syncthreads();
        s_part[threadIdx.x] += x;
        __syncthreads();
    }
    uint32_t run = threadIdx.x ? s_part[threadIdx.x - 1] : 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = v[i];
        v[i] = run;
        run += c;
    }
    return s_part[1023];
}

}  // namespace hast
