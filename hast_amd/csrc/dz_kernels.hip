// dz_kernels.hip -- gzip members written ON THE GPU (gfx950): bytes that already lie in HBM (the routed runs of a FASTQ block) leave
// the device compressed.  The per-piece arithmetic is dz_core.h (shared with the host test); this file is its shape on a wave.
//   k_dz_piece    a wave per piece of 16 KB: match search + greedy parse 64 positions a step, histogram, code lengths (ranks by the
//                 wave, tree and header by lane 0), bits placed by a prefix sum and OR-ed into LDS, whole words to the piece's slot of
//                 the workspace; CRC-32 of the piece by 64 slices.  61 KB of LDS: two pieces a CU.
//   k_dz_scan     one workgroup: where every piece lands in its member (prefix sum of the sizes), the members' CRC-32 (XOR of the
//                 pieces' terms), sizes, headers and trailers; k_dz_scan<true>: the same for blocked gzip (BGZF), members of three
//                 pieces with a frame each, written by a lane per member
//   k_dz_gather   a workgroup per piece: its bytes to their place (stored pieces straight from the input), whole words where the
//                 destination allows
// All global stores are plain vector stores.  The output is a function of the input bytes alone (dz_core.h says why).
#include <hip/hip_runtime.h>

#include "dz_core.h"
#include "dz_device.h"
#include "scan_device.h"

namespace hast {
namespace dz {

namespace {

struct Workspace {              // views into d_work
    uint8_t *slots;             // max_pieces x kSlotBytes
    uint32_t *sizes, *crcs;     // per piece: bytes in its slot (kStoredFlag | input bytes: stored), its term of the member's CRC-32
    uint64_t *offs;             // per piece: where it starts in its member (blocked: behind the start of its run's first member)
};
__host__ __device__ inline Workspace workspace_at(void *d_work, uint32_t max_pieces) {
    Workspace w;
    w.slots = static_cast<uint8_t *>(d_work);
    w.offs = reinterpret_cast<uint64_t *>(w.slots + (size_t)max_pieces * kSlotBytes);
    w.sizes = reinterpret_cast<uint32_t *>(w.offs + max_pieces);
    w.crcs = w.sizes + max_pieces;
    return w;
}

// piece p of the job: its run, its index in the run; false: the job has fewer pieces
__device__ inline bool locate(const Job *job_p, uint32_t p, uint32_t &run, uint32_t &idx) {
    // (the job is read where it lies: a copy of it indexed by the run would live in scratch memory)
    const Job &job = *job_p;
    uint64_t first = 0;
    for (uint32_t r = 0; r < job.n_runs && r < (uint32_t)kMaxRuns; ++r) {
        const uint64_t np = n_pieces(job.n_bytes[r]);
        if (p < first + np) {
            run = r;
            idx = (uint32_t)(p - first);
            return true;
        }
        first += np;
    }
    return false;
}

// bytes 4w .. 4w + 3 of s (any alignment) from the aligned words they lie in
__device__ inline uint32_t load_word(const uint8_t *s, uint32_t w) {
    const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3);
    const uint32_t *base = reinterpret_cast<const uint32_t *>(s - sa) + w;
    return sa ? (base[0] >> (8 * sa)) | (base[1] << (32 - 8 * sa)) : base[0];
}

__device__ inline uint32_t wave_xor(uint32_t v) {
    for (int d = 32; d; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}

}  // namespace

__global__ void k_dz_job_one(Job *job, uint64_t n_bytes) {
    for (int r = 0; r < kMaxRuns; ++r) job->src_off[r] = job->n_bytes[r] = 0;
    job->n_bytes[0] = n_bytes;
    job->n_runs = 1;
    job->emit_empty = 1;
}
__global__ void k_dz_job_from_route(Job *job, const RouteState *rs) {
    // a block the caller routes itself (a record only the host can decide): its runs are not handed out, so nothing is compressed
    if (rs->flags & 1) {
        for (int r = 0; r < kMaxRuns; ++r) job->src_off[r] = job->n_bytes[r] = 0;
        job->n_runs = 0;
        job->emit_empty = 0;
        return;
    }
    uint64_t at = 0;
    for (int r = 0; r < kMaxRuns; ++r) {
        job->src_off[r] = at;
        job->n_bytes[r] = rs->bytes[r];
        at += rs->bytes[r];
    }
    job->n_runs = kMaxRuns;
    job->emit_empty = 0;
}
// the two runs of a converted step (tx_kernels.hip): run 0 from the buffer's first byte, run 1 from second_off on, their sizes where
// k_tx_scan_out left them (TxDevState.out_bytes); an empty run becomes nothing
__global__ void k_dz_job_from_tx(Job *job, const uint64_t *run_bytes, uint64_t second_off) {
    const uint64_t n0 = run_bytes[0], n1 = run_bytes[1];
    job->src_off[0] = 0;
    job->n_bytes[0] = n0;
    job->src_off[1] = second_off;
    job->n_bytes[1] = n1;
    job->src_off[2] = job->n_bytes[2] = 0;
    job->src_off[3] = job->n_bytes[3] = 0;
    job->n_runs = 2;
    job->emit_empty = 0;
}

// the three runs of a binned view of stage 03's read stream (rs_kernels.hip: k_rb_*): back to back from the buffer's first byte, their
// sizes where k_rb_scan left them (RbState.raw_bytes); an empty run becomes nothing
__global__ void k_dz_job_from_bins(Job *job, const uint64_t *run_bytes) {
    const uint64_t n0 = run_bytes[0], n1 = run_bytes[1], n2 = run_bytes[2];
    job->src_off[0] = 0;
    job->n_bytes[0] = n0;
    job->src_off[1] = n0;
    job->n_bytes[1] = n1;
    job->src_off[2] = n0 + n1;
    job->n_bytes[2] = n2;
    job->src_off[3] = job->n_bytes[3] = 0;
    job->n_runs = 3;
    job->emit_empty = 0;
}

__global__ void __launch_bounds__(64) k_dz_piece(const Job *d_job, const uint8_t *src, uint32_t max_pieces, void *d_work, uint32_t flags) {
    __shared__ uint32_t s_in[kPiece / 4 + 2];
    __shared__ uint32_t s_table[kHashSize];               // the match search's table, then the piece's output words
    __shared__ uint64_t s_startm[kPiece / 64], s_matchm[kPiece / 64];
    __shared__ uint32_t s_matches[kMaxMatches];
    __shared__ uint32_t s_freq[kNumLit + kNumDist];
    __shared__ uint8_t s_lens[kNumLit + kNumDist + 4];
    __shared__ uint16_t s_codes[kNumLit + kNumDist];
    __shared__ uint32_t s_crc[256];
    __shared__ CodeScratch s_cs;
    __shared__ HeaderScratch s_hs;
    __shared__ uint16_t s_added[4];
    static_assert(kOutWords <= kHashSize, "the output words reuse the table");

    const uint32_t lane = threadIdx.x, p = blockIdx.x;
    const Job &job = *d_job;
    uint32_t run, idx;
    if (p >= max_pieces || !locate(d_job, p, run, idx)) return;
    const Workspace ws = workspace_at(d_work, max_pieces);
    const uint64_t run_bytes = job.n_bytes[run], piece_off = (uint64_t)idx * kPiece;
    const uint32_t n = (uint32_t)(run_bytes - piece_off < kPiece ? run_bytes - piece_off : kPiece);
    const uint8_t *s = src + job.src_off[run] + piece_off;
    uint8_t *const in = reinterpret_cast<uint8_t *>(s_in);

    for (uint32_t w = lane; w < kPiece / 4 + 2; w += 64) {
        uint32_t v = 0;
        if (4 * w + 4 <= n) v = load_word(s, w);
        else
            for (uint32_t k = 0; 4 * w + k < n; ++k) v |= (uint32_t)s[4 * w + k] << (8 * k);
        s_in[w] = v;
    }
    for (uint32_t i = lane; i < kHashSize; i += 64) s_table[i] = 0;
    for (uint32_t i = lane; i < kNumLit + kNumDist; i += 64) s_freq[i] = 0;
    for (uint32_t i = lane; i < 256; i += 64) s_crc[i] = gz::crc_table_entry(i);
    __syncthreads();

    // ---- match search, parse, histogram: 64 positions a step ----
    uint32_t pos = 0, nm = 0;                               // wave-uniform: where the next token starts, matches so far
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t at = base + lane;
        uint32_t len = 0, dist = 0;
        if (at < n && !(flags & kLiteralsOnly)) probe(in, n, s_table, at, len, dist);
        __syncthreads();                                    // every lane has read the table ...
        if (at < n) enter(in, n, s_table, at);              // ... before this step's positions go in (atomic max: order does not matter)
        const uint32_t end = base + 64 < n ? base + 64 : n;
        uint64_t sm = 0, mm = 0;
        while (pos < end) {                                 // the chain of tokens through this step's positions: scalar, the lengths read lane by lane
            const uint32_t i = __builtin_amdgcn_readfirstlane(pos - base);
            const uint32_t l = __builtin_amdgcn_readlane(len, i);
            sm |= 1ull << i;
            if (l) {
                mm |= 1ull << i;
                pos += l;
            } else ++pos;
        }
        if ((sm >> lane) & 1) {
            const bool is_match = (mm >> lane) & 1;
            if (is_match) s_matches[nm + __popcll(mm & ((1ull << lane) - 1))] = pack_match(len, dist);
            tally(s_freq, in[at], is_match ? len : 0, dist);
        }
        nm += (uint32_t)__popcll(mm);
        if (lane == 0) {
            s_startm[base / 64] = sm;
            s_matchm[base / 64] = mm;
        }
        __syncthreads();
    }

    // ---- the codes ----
    if (lane == 0) {
        s_freq[256] = 1;
        at_least_two(s_freq, kNumLit, s_added);
        at_least_two(s_freq + kNumLit, kNumDist, s_added + 2);
    }
    __syncthreads();
    rank_symbols(s_freq, kNumLit, s_cs, lane, 64);
    __syncthreads();
    if (lane == 0) (void)build_lengths(s_freq, kNumLit, 15, s_lens, s_cs);
    __syncthreads();
    rank_symbols(s_freq + kNumLit, kNumDist, s_cs, lane, 64);
    __syncthreads();
    if (lane == 0) {
        (void)build_lengths(s_freq + kNumLit, kNumDist, 15, s_lens + kNumLit, s_cs);
        forget_added(s_freq, s_added);
        forget_added(s_freq + kNumLit, s_added + 2);
        make_codes(s_lens, kNumLit, s_codes, s_cs);
        make_codes(s_lens + kNumLit, kNumDist, s_codes + kNumLit, s_cs);
        plan_header(s_lens, s_hs, s_cs);
    }
    __syncthreads();
    const uint32_t sym_bits = wave_sum(body_bits(s_freq, s_lens, lane, 64));
    const uint32_t header_bits = s_hs.bits;
    const uint32_t cb = coded_bytes(header_bits, sym_bits);

    // ---- CRC-32 of the piece: a slice a lane ----
    {
        const uint32_t slice = (n + 63) / 64;
        const uint32_t lo = lane * slice < n ? lane * slice : n, hi = lo + slice < n ? lo + slice : n;
        const uint32_t c = wave_xor(crc_term(crc_bytes(s_crc, in + lo, hi - lo), n - hi));
        // ... and what it adds to the member's CRC: the piece knows how many bytes of its member lie behind it (the run's, or in
        // blocked mode those of its group of kBlockedPieces pieces), so k_dz_scan only XORs
        if (lane == 0) ws.crcs[p] = crc_term(c, ((flags & kBlocked) ? blocked_member_end(run_bytes, idx) : run_bytes) - piece_off - n);
    }
    if (cb >= n) {                                          // not smaller than its bytes: a stored block, copied from the input by k_dz_gather
        if (lane == 0) ws.sizes[p] = n | kStoredFlag;
        return;
    }

    // ---- emission ----
    uint32_t *const out = s_table;
    for (uint32_t i = lane; i < kHashSize; i += 64) out[i] = 0;
    __syncthreads();
    uint32_t at_bit = 3 + header_bits;
    if (lane == 0) {
        put_bits(out, 0, 4, 3);                             // BFINAL = 0, BTYPE = 10b
        (void)write_header(s_hs, out, 3);
    }
    __syncthreads();
    nm = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint64_t sm = s_startm[base / 64], mm = s_matchm[base / 64];
        uint32_t nb = 0;
        uint64_t v = 0;
        if ((sm >> lane) & 1) {
            if ((mm >> lane) & 1) v = match_bits(s_matches[nm + __popcll(mm & ((1ull << lane) - 1))], s_lens, s_codes, nb);
            else v = literal_bits(in[base + lane], s_lens, s_codes, nb);
        }
        const uint32_t incl = wave_inclusive_sum(nb, lane);
        put_bits(out, at_bit + incl - nb, v, nb);
        at_bit += __shfl(incl, 63, 64);
        nm += (uint32_t)__popcll(mm);
    }
    __syncthreads();
    if (lane == 0) {
        put_bits(out, at_bit, s_codes[256], s_lens[256]);
        const uint32_t a = (at_bit + s_lens[256] + 3 + 7) & ~7u;       // the empty stored block: 000b, padding, LEN = 0, NLEN = FFFF
        put_bits(out, a, 0xFFFF0000u, 32);
    }
    __syncthreads();
    uint32_t *const slot = reinterpret_cast<uint32_t *>(ws.slots + (size_t)p * kSlotBytes);
    for (uint32_t w = lane; w < (cb + 3) / 4; w += 64) slot[w] = out[w];
    if (lane == 0) ws.sizes[p] = cb;
}

// One workgroup.  Per run: the pieces' places in the member, the member's CRC-32, size, header and trailer.
// kBlockedRun: the run leaves as blocked gzip (dz_core.h).  A piece's place is then the prefix sum of the sizes plus a frame for every
// member in front of its own plus that member's header, and header and trailer of a member are written by the lane that holds the
// member's first piece: it reads the sizes and CRC terms of the (at most two) pieces behind it where k_dz_piece left them, not from
// its neighbours in the lap, so a member whose pieces lie in two laps (member 85: pieces 255, 256, 257) is no special case.
template <bool kBlockedRun>
__global__ void __launch_bounds__(256) k_dz_scan(const Job *d_job, uint32_t max_pieces, void *d_work, uint8_t *dst, uint64_t cap, Result *res) {
    __shared__ uint64_t s_scan[256];
    __shared__ uint32_t s_x[256];
    const uint32_t tid = threadIdx.x;
    const Job &job = *d_job;
    const Workspace ws = workspace_at(d_work, max_pieces);
    uint64_t total_pieces = 0;
    for (uint32_t r = 0; r < job.n_runs && r < (uint32_t)kMaxRuns; ++r) total_pieces += n_pieces(job.n_bytes[r]);
    if (total_pieces > max_pieces) {
        if (tid == 0) {
            for (int r = 0; r < kMaxRuns; ++r) res->out_bytes[r] = 0, res->member_off[r] = ~0ull;
            res->flags = kResPieces;
        }
        return;
    }
    uint64_t first = 0, member_off = 0;
    uint32_t flags = 0;
    for (uint32_t r = 0; r < (uint32_t)kMaxRuns; ++r) {
        const uint64_t nb = r < job.n_runs ? job.n_bytes[r] : 0;
        const uint64_t np = n_pieces(nb);
        if (r >= job.n_runs || (nb == 0 && !job.emit_empty)) {
            if (tid == 0) res->out_bytes[r] = 0, res->member_off[r] = ~0ull;
            continue;
        }
        if (kBlockedRun && np == 0) {                       // (emit_empty) the end-of-file block
            const bool fits = member_off + kBlockedFrame <= cap;
            if (tid == 0) {
                res->out_bytes[r] = fits ? kBlockedFrame : 0;
                res->member_off[r] = fits ? member_off : ~0ull;
                if (fits) put_blocked_frame(dst + member_off, kBlockedFrame, 0, 0);
            }
            if (!fits) flags |= kResOverflow;
            else member_off += kBlockedFrame;
            continue;
        }
        uint64_t at = kBlockedRun ? 0 : kMemberHead;        // uniform: where the next piece starts in the member (blocked: the sizes in front of it)
        uint32_t x = 0;
        for (uint64_t c = 0; c < np; c += 256) {
            const uint64_t i = c + tid;
            uint64_t sz = 0;
            if (i < np) {
                const uint32_t w = ws.sizes[first + i];
                sz = (w & kStoredFlag) ? (uint64_t)(w & ~kStoredFlag) + 5 : w;
                x ^= ws.crcs[first + i];
            }
            s_scan[tid] = sz;
            __syncthreads();
            for (uint32_t d = 1; d < 256; d <<= 1) {
                const uint64_t u = tid >= d ? s_scan[tid - d] : 0;
                __syncthreads();
                s_scan[tid] += u;
                __syncthreads();
            }
            if (i < np) {
                const uint64_t in_front = at + s_scan[tid] - sz;
                if (!kBlockedRun) ws.offs[first + i] = in_front;
                else {
                    ws.offs[first + i] = in_front + (i / kBlockedPieces) * kBlockedFrame + kBlockedHead;
                    if (i % kBlockedPieces == 0) {          // the member's first piece: its frame
                        uint32_t total = kBlockedFrame + (uint32_t)sz, crc = ws.crcs[first + i];
                        for (uint64_t k = i + 1; k < i + kBlockedPieces && k < np; ++k) {
                            const uint32_t w = ws.sizes[first + k];
                            total += (w & kStoredFlag) ? (w & ~kStoredFlag) + 5 : w;
                            crc ^= ws.crcs[first + k];
                        }
                        const uint64_t start = member_off + in_front + (i / kBlockedPieces) * kBlockedFrame;
                        // (a run that does not fit cap is reported below; what is written of it lies in front of cap)
                        if (start + total <= cap) put_blocked_frame(dst + start, total, crc, (uint32_t)(blocked_member_end(nb, i) - i * kPiece));
                    }
                }
            }
            at += s_scan[255];
            __syncthreads();
        }
        if (!kBlockedRun) {
            s_x[tid] = x;
            __syncthreads();
            for (uint32_t d = 128; d; d >>= 1) {
                if (tid < d) s_x[tid] ^= s_x[tid + d];
                __syncthreads();
            }
        }
        const uint64_t total = kBlockedRun ? at + n_members(nb) * kBlockedFrame : at + kMemberTail;
        const bool fits = member_off + total <= cap;
        if (tid == 0) {
            res->out_bytes[r] = fits ? total : 0;
            res->member_off[r] = fits ? member_off : ~0ull;
            if (fits && !kBlockedRun) {
                uint8_t *m = dst + member_off;
                const uint8_t head[kMemberHead] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
                for (uint32_t k = 0; k < kMemberHead; ++k) m[k] = head[k];
                m += at;
                m[0] = 3;                                   // the empty final block (fixed code: BFINAL = 1, BTYPE = 01b, end of block)
                m[1] = 0;
                const uint32_t crc = s_x[0], isize = (uint32_t)nb;
                for (uint32_t k = 0; k < 4; ++k) m[2 + k] = (uint8_t)(crc >> (8 * k)), m[6 + k] = (uint8_t)(isize >> (8 * k));
            }
        }
        if (!fits) flags |= kResOverflow;
        else member_off += total;
        first += np;
        __syncthreads();
    }
    if (tid == 0) {
        res->flags = flags;
        res->reserved = 0;
    }
}

// A workgroup per piece: size bytes from its slot, or (stored) 5 bytes of block header and the input's bytes, to their place.
__global__ void __launch_bounds__(256) k_dz_gather(const Job *d_job, const uint8_t *src, uint32_t max_pieces, const void *d_work, uint8_t *dst, const Result *res) {
    const uint32_t tid = threadIdx.x, p = blockIdx.x;
    const Job &job = *d_job;
    uint32_t run, idx;
    if (p >= max_pieces || (res->flags & kResPieces) || !locate(d_job, p, run, idx)) return;
    const uint64_t moff = res->member_off[run];
    if (moff == ~0ull) return;
    const Workspace ws = workspace_at(const_cast<void *>(d_work), max_pieces);
    const uint32_t w = ws.sizes[p];
    uint8_t *d = dst + moff + ws.offs[p];
    const uint8_t *s;
    uint32_t n;
    if (w & kStoredFlag) {
        n = w & ~kStoredFlag;
        s = src + job.src_off[run] + (uint64_t)idx * kPiece;
        if (tid < 5) {
            const uint32_t h[5] = {0u, n & 0xFF, n >> 8, ~n & 0xFF, (~n >> 8) & 0xFF};
            d[tid] = (uint8_t)h[tid];
        }
        d += 5;
    } else {
        n = w;
        s = ws.slots + (size_t)p * kSlotBytes;
    }
    uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3);
    if (head > n) head = n;
    const uint32_t words = (n - head) / 4, tail_at = head + 4 * words;
    if (tid < head) d[tid] = s[tid];
    uint32_t *dw = reinterpret_cast<uint32_t *>(d + head);
    for (uint32_t k = tid; k < words; k += 256) dw[k] = load_word(s + head, k);
    if (tid < n - tail_at) d[tail_at + tid] = s[tail_at + tid];
}

size_t workspace_bytes(uint32_t max_pieces) { return (size_t)max_pieces * (kSlotBytes + sizeof(uint64_t) + 2 * sizeof(uint32_t)) + 64; }

hipError_t launch_job_one(Job *d_job, uint64_t n_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_dz_job_one, dim3(1), dim3(1), 0, s, d_job, n_bytes);
    return hipGetLastError();
}
hipError_t launch_job_from_route(Job *d_job, const RouteState *d_rs, hipStream_t s) {
    hipLaunchKernelGGL(k_dz_job_from_route, dim3(1), dim3(1), 0, s, d_job, d_rs);
    return hipGetLastError();
}
hipError_t launch_job_from_tx(Job *d_job, const uint64_t *d_run_bytes, uint64_t second_off, hipStream_t s) {
    hipLaunchKernelGGL(k_dz_job_from_tx, dim3(1), dim3(1), 0, s, d_job, d_run_bytes, second_off);
    return hipGetLastError();
}
hipError_t launch_job_from_bins(Job *d_job, const uint64_t *d_run_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_dz_job_from_bins, dim3(1), dim3(1), 0, s, d_job, d_run_bytes);
    return hipGetLastError();
}
hipError_t launch_compress(const Job *d_job, const uint8_t *d_src, uint32_t max_pieces, void *d_work, uint8_t *d_dst, uint64_t cap, Result *d_res,
                           uint32_t flags, hipStream_t s) {
    if (max_pieces) hipLaunchKernelGGL(k_dz_piece, dim3(max_pieces), dim3(64), 0, s, d_job, d_src, max_pieces, d_work, flags);
    if (flags & kBlocked) hipLaunchKernelGGL(k_dz_scan<true>, dim3(1), dim3(256), 0, s, d_job, max_pieces, d_work, d_dst, cap, d_res);
    else hipLaunchKernelGGL(k_dz_scan<false>, dim3(1), dim3(256), 0, s, d_job, max_pieces, d_work, d_dst, cap, d_res);
    if (max_pieces) hipLaunchKernelGGL(k_dz_gather, dim3(max_pieces), dim3(256), 0, s, d_job, d_src, max_pieces, (const void *)d_work, d_dst, (const Result *)d_res);
    return hipGetLastError();
}

}  // namespace dz
}  // namespace hast
