// gz_wave.h -- what a WAVE does around gz_core.h's token parse, shared by the inflate kernels (gz_kernels.hip k_gz_decode,
// bz_kernels.hip k_bz_inflate): the compressed words around the read position in LDS, the 64 bits at every lane's bit offset, and
// the prefix sum that gives a step's tokens their places in the output.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hast {
namespace gz {

struct WIn {                       // the compressed words around the read position: a ring of 128 words in LDS (s_in[word & 127]),
    const uint32_t *w;             // always the 128 words from rb on (rb a multiple of 64, the position inside the first 64); the 64
    uint64_t nwords;               // words behind them wait in a VGPR (nxt), loaded ~20 steps before they are put into the ring
    uint64_t rb;
    uint32_t nxt;
};
__device__ __forceinline__ uint32_t wload(const WIn &b, uint64_t i) { return i < b.nwords ? b.w[i] : 0u; }
__device__ __forceinline__ void win_at(WIn &b, uint32_t *s_in, uint64_t pos) {      // (uniform) the ring covers `pos` and the 4 words behind it
    const uint64_t wi = pos >> 5;
    const uint32_t lane = threadIdx.x;
    if (wi < b.rb || wi >= b.rb + 128) {
        b.rb = wi & ~63ull;
        __builtin_amdgcn_wave_barrier();
        s_in[(uint32_t)(b.rb + lane) & 127] = wload(b, b.rb + lane);
        s_in[(uint32_t)(b.rb + 64 + lane) & 127] = wload(b, b.rb + 64 + lane);
        b.nxt = wload(b, b.rb + 128 + lane);
        __builtin_amdgcn_wave_barrier();
    } else if (wi >= b.rb + 64) {
        __builtin_amdgcn_wave_barrier();
        s_in[(uint32_t)(b.rb + lane) & 127] = b.nxt;                          // (the words rb + 128 .. rb + 191 take the place of rb .. rb + 63)
        b.rb += 64;
        b.nxt = wload(b, b.rb + 128 + lane);
        __builtin_amdgcn_wave_barrier();
    }
}
__device__ __forceinline__ uint64_t win_bits(const WIn &b, const uint32_t *s_in, uint64_t pos) {      // the 64 bits at pos + lane
    const uint32_t rel = (uint32_t)(pos - b.rb * 32) + threadIdx.x, wi = (uint32_t)b.rb + (rel >> 5), sh = rel & 31;
    const uint32_t w0 = s_in[wi & 127], w1 = s_in[(wi + 1) & 127], w2 = s_in[(wi + 2) & 127];
    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh), hi = __builtin_amdgcn_alignbit(w2, w1, sh);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {              // inclusive prefix sum over the 64 lanes (DPP: rows, then row 15 -> next row, then 31 -> upper half)
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
    return x;
}

}  // namespace gz
}  // namespace hast
