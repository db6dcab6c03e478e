// bz_kernels.hip -- gfx950 device code of the BLOCKED gzip inflate (BGZF; bz_core.h has the format's rules, bz_api.cpp the stream).
// A BGZF member says where it ends and what it inflates to, and copies nothing from in front of itself, so nothing of gz_kernels.hip's
// speculative machinery is needed (no block-start search, no chain, no marker symbols, no windows, no translate):
//   k_bz_inflate   a WAVE per member: from the member's first deflate bit to its final block, straight to BYTES at the member's place
//                  in the batch's output.  The symbol loop is k_gz_decode's: a token parsed at each of 64 bit offsets (gz_core.h
//                  parse_token), the chain of real tokens walked with one scalar read per token, rounds of at most 64 bytes written by
//                  all lanes, recent output in an LDS ring, far sources loaded past the L1 behind a wait for the wave's own stores
//   k_bz_crc     a workgroup per member: CRC-32 of its bytes by 256 slices (gz_core.h crc_*), compared with the trailer's; bytes
//                  produced compared with ISIZE; one word per member, and the index of the batch's first refused member by atomicMin
// Bound: k_bz_inflate by latency per token, as k_gz_decode (hence by waves in flight: 5 per SIMD, 7.9 KB of LDS each); k_bz_crc streams.
#include <hip/hip_runtime.h>

#include "bz_core.h"
#include "bz_device.h"
#include "gz_core.h"
#include "gz_wave.h"

namespace hast {
namespace bz {

using namespace hast::gz;

// byte stores of a wave, and loads of what it stored a while ago (past the L1: the stores have reached the L2 once s_waitcnt says so)
__device__ __forceinline__ void byte_store(uint8_t *p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ uint8_t byte_load_far(const uint8_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Workgroup shape, waves per SIMD and LDS per wave are k_gz_decode's (64 lanes, 5 waves per SIMD, 7.9 KB: tables at zlib's bounds and
// a ring that holds 1024 BYTES where k_gz_decode's holds 512 symbols); no other choice has been measured for this kernel.
// Every store is a BYTE store inside [out_off, out_off + isize): neighbours' regions meet at arbitrary byte addresses.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) k_bz_inflate(const Member *__restrict__ mem, uint32_t n_mem, const uint32_t *__restrict__ w, uint8_t *__restrict__ out_base, MemberOut *__restrict__ res) {
    __shared__ uint32_t s_tab[kLitTabCap + kDistTabCap];
    // two lives, as in k_gz_decode: lane 0's header parse (code-length table + HdrScratch), then the words around the read position
    // (128) and a round's tokens (64)
    constexpr uint32_t kScrWords = (sizeof(HdrScratch) + 3) / 4;
    __shared__ uint32_t s_misc[kPreTabCap + (kScrWords > 64 ? kScrWords : 64)];
    __shared__ uint32_t s_hdr[4];
    uint32_t *const s_in = s_misc, *const s_tok = s_misc + kPreTabCap;
    __shared__ uint8_t s_ring[kRing];
    constexpr uint32_t kIsLit = 0x40000000u, kIsMatch = 0x80000000u;
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    if (j >= n_mem) return;
    const Member m = mem[j];
    uint8_t *const out = out_base + m.out_off;
    const uint64_t nbits = m.end_bit;                                          // (the trailer's first bit: nothing at or behind it is data)
    const uint32_t cap = m.isize;
    const uint32_t *const lit = s_tab, *const dst = s_tab + kLitTabCap;
    constexpr uint64_t kFarAway = ~0ull >> 1;
    WIn in{w, ((nbits + 31) >> 5) + 2, kFarAway, 0};
    uint64_t at = m.first_bit;
    uint32_t n = 0, why = kBadNone;
    auto refuse = [&](uint32_t rc, uint32_t err) {                             // gz_core.h's status bit + error code -> why
        why = rc == kStStarved ? (uint32_t)kBadCutShort : rc == kStNoRoom ? (uint32_t)kBadTooLong : ((err == kErrTooFar ? (uint32_t)kBadTooFar : (uint32_t)kBadDeflate) | (err << 8));
    };
    for (;;) {
        if (at + 3 > nbits) { why = kBadCutShort; break; }
        const uint32_t hdr3 = (uint32_t)(bits_at(w, at) & 7);
        const uint32_t final = hdr3 & 1, type = hdr3 >> 1;
        uint32_t n2 = n, rc = 0, err = kErrNone;
        if (type == 0) {
            const uint64_t byte = (at + 3 + 7) >> 3;
            if ((byte + 4) * 8 > nbits) { why = kBadCutShort; break; }
            const uint8_t *bytes = reinterpret_cast<const uint8_t *>(w) + byte;
            const uint32_t len = bytes[0] | ((uint32_t)bytes[1] << 8), nlen = bytes[2] | ((uint32_t)bytes[3] << 8);
            if ((len ^ 0xFFFFu) != nlen) { refuse(kStError, kErrStoredLen); break; }
            if ((byte + 4 + len) * 8 > nbits) { why = kBadCutShort; break; }
            if (n + len > cap) { why = kBadTooLong; break; }
            for (uint32_t k0 = 0; k0 < len; k0 += 64) {
                const uint32_t k = k0 + lane;
                if (k < len) {
                    const uint8_t v = bytes[4 + k];
                    s_ring[(n + k) & (kRing - 1)] = v;
                    byte_store(out + n + k, v);
                }
            }
            __syncthreads();
            n2 = n + len;
            at = (byte + 4 + len) * 8;
        } else if (type == 3) {
            refuse(kStError, kErrBlockType);
            break;
        } else {
            __syncthreads();                                                  // (everyone is done with the previous block's tables, words and tokens)
            if (lane == 0) {
                Tables t{s_tab, s_tab + kLitTabCap, s_misc};
                HdrScratch &scr = *reinterpret_cast<HdrScratch *>(s_misc + kPreTabCap);
                uint32_t bad = 0;
                uint64_t behind = at + 3;
                if (type == 1) fixed_tables(t, scr);
                else {
                    Bits hb{w, nbits, 0, 0, 0};
                    seek(hb, behind);
                    bad = read_dynamic(hb, t, false, true, scr);
                    if (overran(hb)) bad = 0x80000000u;                       // (also an "error" read out of what lies behind the data)
                    behind = pos(hb);
                }
                s_hdr[0] = bad;
                s_hdr[1] = (uint32_t)behind;
                s_hdr[2] = (uint32_t)(behind >> 32);
            }
            __syncthreads();
            const uint32_t bad = s_hdr[0];
            if (bad) {
                if (bad == 0x80000000u) why = kBadCutShort;
                else refuse(kStError, bad);
                break;
            }
            uint64_t pos = (uint64_t)s_hdr[1] | ((uint64_t)s_hdr[2] << 32);
            in.rb = kFarAway;                                                 // (the header parse has used the words' place)
            {   // two literals per first-level entry where both codes fit (gz_core.h pair_entry): every entry worked out before any is replaced
                uint32_t pe[(1u << kLitRoot) / 64];
                uint32_t l2 = lane;
                asm volatile("" : "+v"(l2));
#pragma unroll
                for (uint32_t q = 0; q < (1u << kLitRoot) / 64; ++q) pe[q] = pair_entry(lit, q * 64 + l2);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (uint32_t q = 0; q < (1u << kLitRoot) / 64; ++q) s_tab[q * 64 + l2] = pe[q];
                __syncthreads();
            }
            // ---- the block's bytes, a step = the 64 bit offsets from pos on ----
            bool block_done = false, full = false;
            while (!block_done && !rc) {
                if (pos >= nbits) { rc = kStStarved; break; }
                const uint64_t avail = nbits - pos;
                const uint32_t limit = avail < 64 ? (uint32_t)avail : 64u;
                win_at(in, s_in, pos);
                const uint64_t bits = win_bits(in, s_in, pos);
                const Token tk = full ? parse_token(bits, lit, dst) : parse_token_fast(bits, lit, dst);
                full = false;
                const uint32_t need = tk.dist ? (tk.dist > tk.olen ? tk.dist - tk.olen : 0u) : 0xFFFFu;      // bytes of the round that may stand in front of it
                uint32_t p = 0;
                for (;;) {                                                    // the chain, from one stop to the next
                    // while (p < limit) { t = info of lane p; if (t >= 128) { stop = t; break; }  tokmask |= 1 << p;  p += t; } -- by hand, as in k_gz_decode
                    uint64_t tokmask = 0;
                    uint32_t stop;
                    asm volatile("s_mov_b32 %[t], 0\n\t"
                                 "s_cmp_lt_u32 %[p], %[limit]\n\t"
                                 "s_cbranch_scc0 2f\n"
                                 "1:\n\t"
                                 "v_readlane_b32 %[t], %[info], %[p]\n\t"
                                 "s_cmpk_ge_u32 %[t], 0x80\n\t"
                                 "s_cbranch_scc1 2f\n\t"
                                 "s_bitset1_b64 %[mask], %[p]\n\t"
                                 "s_add_u32 %[p], %[p], %[t]\n\t"
                                 "s_cmp_lt_u32 %[p], %[limit]\n\t"
                                 "s_cbranch_scc1 1b\n\t"
                                 "s_mov_b32 %[t], 0\n"
                                 "2:\n"
                                 : [t] "=&s"(stop), [mask] "+s"(tokmask), [p] "+s"(p)
                                 : [info] "v"(tk.info), [limit] "s"(limit)
                                 : "scc");
                    if (!stop && p > avail) { rc = kStStarved; break; }       // the last token reads past the member's data
                    if (tokmask) {
                        const bool is_tok = (tokmask >> lane) & 1;
                        const uint32_t incl = wave_incl_scan(is_tok ? tk.olen : 0u), start = incl - (is_tok ? tk.olen : 0u);
                        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                        // nothing in front of the member's first byte is its own: not even the bytes of the member in front of it in the buffer
                        if (__ballot(is_tok && tk.dist > n2 + start)) { err = kErrTooFar; rc = kStError; break; }
                        uint32_t base = 0;
                        uint64_t rem = tokmask;
                        while (rem) {
                            const bool in_rem = (rem >> lane) & 1;
                            const unsigned long long vm = __ballot(in_rem && (incl - base > 64 || need < start - base));
                            uint64_t cur = rem;
                            uint32_t nsym = total - base;
                            if (vm) {
                                const uint32_t fv = (uint32_t)__builtin_ctzll(vm);
                                cur = rem & ((1ull << fv) - 1);
                                nsym = (uint32_t)__builtin_amdgcn_readlane((int)start, (int)fv) - base;
                            }
                            if (n2 + nsym > cap) { rc = kStNoRoom; break; }   // (more than ISIZE: nothing is written behind the member's region)
                            __builtin_amdgcn_wave_barrier();
                            s_tok[lane] = 0;
                            if ((cur >> lane) & 1) {
                                const uint32_t st = start - base;
                                if (tk.dist) s_tok[st] = kIsMatch | st | (tk.dist << 14);
                                else {
                                    s_tok[st] = kIsLit | (tk.val & 0xFF);
                                    if (tk.olen == 2) s_tok[st + 1] = kIsLit | (tk.val >> 8);
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                            const uint32_t mine = s_tok[lane];
                            const unsigned long long mm = __ballot((mine & kIsMatch) != 0);
                            const bool act = lane < nsym;
                            const uint32_t bstart = n2;
                            uint8_t v = (uint8_t)(mine & 0xFF);
                            if (mm) {
                                const unsigned long long upto = mm & (~0ull >> (63 - lane));
                                const uint32_t leader = 63u - (uint32_t)__builtin_clzll(upto | 1ull);
                                const uint32_t tv = (uint32_t)__shfl((int)mine, (int)leader, 64);
                                const bool is_m = act && !(mine & kIsLit);
                                const uint32_t off = tv & 63, dist = (tv >> 14) & 0xFFFF, k = lane - off;
                                const int64_t ring_lo = (int64_t)bstart - (int64_t)kRing;                   // what the ring holds (the round reads before it writes)
                                uint32_t kk = k;
                                if (k >= dist) {                               // a run: byte k repeats byte k mod dist (k < 64: exact in float)
                                    const uint32_t q = (uint32_t)(((float)k + 0.5f) * __frcp_rn((float)dist));
                                    kk = k - q * dist;
                                }
                                // (>= 0 for every match of the round: checked above)
                                const int64_t src = (int64_t)bstart + (int64_t)off - (int64_t)dist + (int64_t)kk;
                                const bool far = is_m && src >= 0 && src < ring_lo;
                                if (__ballot(far)) __builtin_amdgcn_s_waitcnt(0);
                                if (is_m && src >= 0) v = far ? byte_load_far(out + src) : s_ring[(uint32_t)src & (kRing - 1)];
                            }
                            __builtin_amdgcn_wave_barrier();
                            if (act) {
                                s_ring[(bstart + lane) & (kRing - 1)] = v;
                                byte_store(out + bstart + lane, v);
                            }
                            base += nsym;
                            n2 += nsym;
                            rem &= ~cur;
                        }
                        if (rc) break;
                    }
                    if (!stop) break;
                    const uint32_t kind = stop >> 7, tl = stop & 127;
                    if (kind == kTokSlow) {                                   // the step that starts here parses in full
                        full = true;
                        break;
                    }
                    if (kind == kTokErrLit || kind == kTokErrDist) {
                        if (p + 48 > avail) rc = kStStarved;                  // (read out of what is not the member's data)
                        else { err = kind == kTokErrLit ? kErrLitCode : kErrDistCode; rc = kStError; }
                        break;
                    }
                    if (p + tl > avail) { rc = kStStarved; break; }
                    if (kind == kTokEob) {
                        pos += p + tl;
                        block_done = true;
                        break;
                    }
                    // a long match, on its own, 64 bytes per step: the lanes of a step read before any of them writes
                    const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)tk.olen, (int)p), distance = (uint32_t)__builtin_amdgcn_readlane((int)tk.dist, (int)p);
                    if (distance > n2) { err = kErrTooFar; rc = kStError; break; }
                    if (n2 + len > cap) { rc = kStNoRoom; break; }
                    const bool near = ring_holds_long_match(distance, len);
                    if (!near) __builtin_amdgcn_s_waitcnt(0);
                    for (uint32_t k0 = 0; k0 < len; k0 += 64) {
                        const uint32_t k = k0 + lane;
                        uint8_t v = 0;
                        if (k < len) {
                            const uint32_t kk = k < distance ? k : k % distance;
                            const uint32_t src = n2 - distance + kk;
                            v = near ? s_ring[src & (kRing - 1)] : byte_load_far(out + src);
                        }
                        __builtin_amdgcn_wave_barrier();
                        if (k < len) {
                            s_ring[(n2 + k) & (kRing - 1)] = v;
                            byte_store(out + n2 + k, v);
                        }
                    }
                    n2 += len;
                    p += tl;
                }
                if (!block_done && !rc) pos += p;
            }
            if (rc) {
                refuse(rc, err);
                n = n2;
                break;
            }
            at = pos;
        }
        n = n2;
        if (final) break;
    }
    if (lane == 0) res[j] = MemberOut{why, n};
}

// ---- the verdict per member: k_bz_inflate's, bytes produced against ISIZE, CRC-32 against the trailer's ----------------------------------
// k_gz_crc's method on bytes: 256 slices of equal length counted from the END (only the first may be short), a table-driven CRC per
// slice (the table in LDS), combined pairwise with x^(8 s 2^k); a lane's slice is contiguous and read 16 bytes a load where the
// ADDRESS allows it (members start at arbitrary byte addresses).
__global__ void __launch_bounds__(256) k_bz_crc(const Member *__restrict__ mem, uint32_t n_mem, const uint8_t *__restrict__ out_base, const MemberOut *__restrict__ res, uint32_t *__restrict__ verdict, uint32_t *first) {
    __shared__ uint32_t s_tab[256], s_part[256];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (c >= n_mem) return;
    const Member m = mem[c];
    const MemberOut r = res[c];
    uint32_t why = r.why;                                                      // (uniform from here on)
    if (!why && r.n_out != m.isize) why = r.n_out < m.isize ? kBadTooShort : kBadTooLong;
    if (!why) {
        uint32_t crc = 0;
        const uint32_t n = m.isize;
        if (n) {
            s_tab[tid] = crc_table_entry(tid);
            __syncthreads();
            const uint8_t *s = out_base + m.out_off;
            const uint32_t slice = (n + 255) / 256;
            const long long hi = (long long)n - (long long)(255 - tid) * slice, lo = hi - slice;
            uint32_t v = 0xFFFFFFFFu;
            auto step = [&](uint32_t b) { v = s_tab[(v ^ b) & 0xFF] ^ (v >> 8); };
            auto step4 = [&](uint32_t x) { step(x); step(x >> 8); step(x >> 16); step(x >> 24); };
            long long i = lo < 0 ? 0 : lo;
            for (; i < hi && (reinterpret_cast<uintptr_t>(s + i) & 15); ++i) step(s[i]);
            for (; i + 16 <= hi; i += 16) {
                const uint4 q = *reinterpret_cast<const uint4 *>(s + i);
                step4(q.x); step4(q.y); step4(q.z); step4(q.w);
            }
            for (; i < hi; ++i) step(s[i]);
            s_part[tid] = hi <= 0 ? 0u : v ^ 0xFFFFFFFFu;
            uint32_t xk = crc_x2nmodp(slice, 3);
            __syncthreads();
            for (uint32_t st = 1; st < 256; st <<= 1) {
                if ((tid & (2 * st - 1)) == 0) s_part[tid] = crc_combine_op(s_part[tid], s_part[tid + st], xk);
                xk = crc_multmodp(xk, xk);
                __syncthreads();
            }
            crc = s_part[0];
        }
        if (crc != m.crc) why = kBadCrc;
    }
    if (tid == 0) {
        verdict[c] = why;
        if (why) {
            atomicMin(&first[0], c);
            atomicMin(&first[1], (c << 8) | (why & 0xFF));
        }
    }
}

hipError_t launch_inflate(const Member *d_mem, uint32_t n, const uint32_t *d_w, uint8_t *d_out, MemberOut *d_res, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_bz_inflate, dim3(n), dim3(64), 0, s, d_mem, n, d_w, d_out, d_res);
    return hipGetLastError();
}
hipError_t launch_check(const Member *d_mem, uint32_t n, const uint8_t *d_out, const MemberOut *d_res, uint32_t *d_verdict, uint32_t *d_first, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_bz_crc, dim3(n), dim3(256), 0, s, d_mem, n, d_out, d_res, d_verdict, d_first);
    return hipGetLastError();
}

}  // namespace bz
}  // namespace hast
