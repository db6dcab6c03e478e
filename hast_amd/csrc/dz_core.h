// dz_core.h -- deflate (RFC 1951) ENCODING of one piece of a gzip member, written once for the device and for the host: the role
// gz_core.h plays for decoding.  k_dz_piece (dz_kernels.hip) runs these functions with a wave per piece; tests/native/test_dz_core.cpp
// restates the wave's steps with plain loops over the same functions, so the arithmetic, the header edge cases and the layout are
// checked against zlib and against gz_core.h's decode_chunk on the CPU before they cost GPU time.
//
// A PIECE is kPiece input bytes, compressed with no history across pieces:
//   match search  64 positions a step.  A lane looks its position's 4 bytes up in a table of recent positions (hash of the 4 bytes ->
//                 the LATEST earlier position with that hash that lies in front of this step's 64) and at distance 1 (runs); every
//                 candidate is verified byte by byte, so a colliding entry costs ratio, never correctness.  The step's positions are
//                 entered with an atomic MAX after all 64 have read: the table's content is a function of the input alone, whatever
//                 order the lanes' stores land in (reproducible output).
//   parse         greedy: the chain of chosen tokens 0 -> 0 + its token's length -> ... is walked through the step's 64 (length,
//                 distance) pairs where they lie in registers.  What is kept of a piece: a bit per position "a token starts here",
//                 a bit "... and it is a match", and the matches' (length, distance) in chain order; literals are the input bytes.
//   code          symbol histogram (atomic adds while parsing) -> Huffman code lengths limited to 15 bits (7 for the code-length
//                 code) -> canonical codes; the dynamic header is run-length coded (16 / 17 / 18) with HCLEN trimmed.
//   emission      64 positions a step: a lane makes its token's bits (at most 48), a prefix sum of the bit counts gives every
//                 token its place, the bits are OR-ed into the piece's output words in LDS.
//   fallback      a piece whose coded form would not be smaller than its bytes becomes a STORED block.
// A coded piece is: non-final dynamic block, then an empty stored block (000b, padding, 00 00 FF FF: what Z_SYNC_FLUSH and pigz
// write), so every piece ends on a byte boundary and pieces are concatenated as bytes.  A member is: 10-byte header, the pieces, an
// empty final block (fixed code: 03 00), CRC-32, ISIZE.
#pragma once
#include <stdint.h>

#include "bz_core.h"
#include "gz_core.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define DZ_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define DZ_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define DZ_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define DZ_ATOMIC_ADD(p, v) (*(p) += (v))
#define DZ_ATOMIC_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#define DZ_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

namespace hast {
namespace dz {

constexpr uint32_t kPiece = 16384;                      // input bytes of a piece (a stored block holds at most 65535)
constexpr uint32_t kHashBits = 12, kHashSize = 1u << kHashBits;
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258;
constexpr uint32_t kMaxMatches = kPiece / kMinMatch;    // chosen matches do not overlap
constexpr uint32_t kNumLit = 286, kNumDist = 30, kNumCl = 19;
constexpr uint32_t kOutWords = kPiece / 4;              // a coded piece is smaller than its input, or it is stored
constexpr uint32_t kSlotBytes = kPiece;                 // what a coded piece may take of the workspace
constexpr uint32_t kStoredFlag = 1u << 31;              // in a piece's size word: the piece is a stored block (its bytes are the input's)
constexpr uint32_t kMemberHead = 10, kMemberTail = 2 + 8;

// most bytes a member of n input bytes takes: every piece stored (5 bytes of block header each)
GZ_HD uint64_t n_pieces(uint64_t n) { return (n + kPiece - 1) / kPiece; }
GZ_HD uint64_t bound(uint64_t n) { return kMemberHead + n + 5 * n_pieces(n) + kMemberTail; }

// ---- BLOCKED gzip (BGZF, bz_core.h) out of the same pieces ------------------------------------------------------------------------
// A run's pieces, unchanged, framed as members of at most kBlockedPieces pieces: 18 bytes of header with the BC subfield (BSIZE =
// the member's bytes - 1), the pieces, the empty final block, CRC-32 and ISIZE of THAT member's input.  A run of n > 0 bytes is
// n_members(n) such members back to back; an empty run with emit_empty is one empty member, which is BGZF's end-of-file block.
// Four pieces do not always fit a member (18 + 4 * (16384 + 5) + 10 = 65 584 bytes when every piece is stored), three do.
constexpr uint32_t kBlockedPieces = 3, kBlockedInput = kBlockedPieces * kPiece;
constexpr uint32_t kBlockedHead = 18, kBlockedFrame = kBlockedHead + kMemberTail;
static_assert(kBlockedHead == bz::kMinHeader, "the header is the BC subfield alone");
static_assert(kBlockedFrame + kBlockedPieces * (kPiece + 5) <= bz::kMaxMember, "a member of stored pieces fits BSIZE");
static_assert(kBlockedFrame + (kBlockedPieces + 1) * (kPiece + 5) > bz::kMaxMember, "... and one piece more would not");
static_assert(kBlockedInput <= bz::kMaxIsize, "a member inflates to no more than a BGZF block may");
GZ_HD uint64_t n_members(uint64_t n) { return (n + kBlockedInput - 1) / kBlockedInput; }
GZ_HD uint64_t bound_blocked(uint64_t n) { return n + 5 * n_pieces(n) + kBlockedFrame * (n_members(n) ? n_members(n) : 1); }
// input bytes of a run of n that lie in front of the end of the member piece idx belongs to (where its CRC term is advanced to)
GZ_HD uint64_t blocked_member_end(uint64_t n, uint64_t idx) {
    const uint64_t e = (idx / kBlockedPieces + 1) * kBlockedInput;
    return e < n ? e : n;
}
// header and trailer of a member of `total` bytes in all (byte stores: a member starts at any address)
GZ_HD void put_blocked_frame(uint8_t *m, uint32_t total, uint32_t crc, uint32_t isize) {
    const uint32_t bsize = total - 1;
    m[0] = 0x1f; m[1] = 0x8b; m[2] = 8; m[3] = 4;           // FEXTRA
    m[4] = m[5] = m[6] = m[7] = 0;                          // MTIME
    m[8] = 0; m[9] = 0xff;                                  // XFL, OS: unknown
    m[10] = 6; m[11] = 0;                                   // XLEN
    m[12] = 'B'; m[13] = 'C'; m[14] = 2; m[15] = 0;
    m[16] = (uint8_t)bsize; m[17] = (uint8_t)(bsize >> 8);
    uint8_t *t = m + total - kMemberTail;
    t[0] = 3; t[1] = 0;                                     // the empty final block (fixed code: BFINAL = 1, BTYPE = 01b, end of block)
    for (uint32_t k = 0; k < 4; ++k) t[2 + k] = (uint8_t)(crc >> (8 * k)), t[6 + k] = (uint8_t)(isize >> (8 * k));
}
// (the host's statement of a blocked run: blocked_run, at the end of this file)

// ---- a compression call as it lies in device memory (the launchers: dz_device.h) ----
constexpr int kMaxRuns = 4;
// What to compress: up to four runs of bytes inside one device buffer, a gzip member each.  The sizes may be known on the device only
// (the routed runs of a FASTQ block: launch_job_from_route), so the kernels read them here and the grids are sized by an upper bound.
struct Job {
    uint64_t src_off[kMaxRuns], n_bytes[kMaxRuns];
    uint32_t n_runs;
    uint32_t emit_empty;        // 1: a run of 0 bytes becomes an empty member (20 bytes; blocked: 28); 0: it becomes nothing
};
struct Result {
    uint64_t out_bytes[kMaxRuns];       // bytes of every run's member (blocked: members); they lie back to back from d_dst[0] on
    uint64_t member_off[kMaxRuns];
    uint32_t flags;                     // 1: the members do not fit cap, 2: more pieces than the workspace holds (nothing is written then)
    uint32_t reserved;
};
constexpr uint32_t kResOverflow = 1, kResPieces = 2;
// how launch_compress is to work (its flags word)
constexpr uint32_t kLiteralsOnly = 1;   // no match search (Huffman coding alone)
constexpr uint32_t kBlocked = 2;        // the runs leave as blocked gzip

// the host's check of a Result before it copies members: those of the first n_runs runs lie back to back from 0 on and end inside
// cap.  off[c]: where run c's member lies (an empty run's: where it would), *total: the bytes of all of them
enum Layout { kLayoutOk = 0, kLayoutGap = 1, kLayoutPastCap = 2 };  // (a gap or an overlap)
inline Layout member_layout(const Result &r, int n_runs, uint64_t cap, uint64_t off[kMaxRuns], uint64_t *total) {
    uint64_t at = 0;
    for (int c = 0; c < n_runs; ++c) {
        off[c] = at;
        if (!r.out_bytes[c]) continue;
        if (r.member_off[c] != at) return kLayoutGap;
        if (r.out_bytes[c] > cap || at > cap - r.out_bytes[c]) return kLayoutPastCap;
        at += r.out_bytes[c];
    }
    *total = at;
    return kLayoutOk;
}

// ---- match search ------------------------------------------------------------------------------------------------------------
GZ_HD uint32_t load4(const uint8_t *in, uint32_t p) {
    return (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16) | ((uint32_t)in[p + 3] << 24);
}
GZ_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }
GZ_HD uint32_t match_len(const uint8_t *in, uint32_t n, uint32_t cand, uint32_t p) {      // cand < p; bytes equal from there, <= 258
    const uint32_t lim = n - p < kMaxMatch ? n - p : kMaxMatch;
    uint32_t l = 0;
    while (l < lim && in[cand + l] == in[p + l]) ++l;
    return l;
}
// position p's match against the table as the steps in front of p's left it (table entries are position + 1, 0 = none) and
// against distance 1.  len = 0: a literal.  The longer one wins, the table's on a tie.
GZ_HD void probe(const uint8_t *in, uint32_t n, const uint32_t *table, uint32_t p, uint32_t &len, uint32_t &dist) {
    len = 0;
    dist = 0;
    if (p + kMinMatch > n) return;
    const uint32_t e = table[hash4(load4(in, p))];
    if (e) {
        const uint32_t l = match_len(in, n, e - 1, p);
        if (l >= kMinMatch) { len = l; dist = p - (e - 1); }
    }
    if (p && in[p - 1] == in[p]) {
        const uint32_t l = match_len(in, n, p - 1, p);
        if (l >= kMinMatch && l > len) { len = l; dist = 1; }
    }
}
GZ_HD void enter(const uint8_t *in, uint32_t n, uint32_t *table, uint32_t p) {
    if (p + kMinMatch <= n) DZ_ATOMIC_MAX(&table[hash4(load4(in, p))], p + 1);
}

// ---- symbols -----------------------------------------------------------------------------------------------------------------
GZ_HD uint32_t ilog2(uint32_t v) {                     // v >= 1
    uint32_t r = 0;
    while (v >>= 1) ++r;
    return r;
}
// length 3 .. 258 -> code 0 .. 28 (symbol 257 + code), extra bits and their value
GZ_HD void len_symbol(uint32_t len, uint32_t &code, uint32_t &nextra, uint32_t &extra) {
    const uint32_t l = len - 3;
    if (len == kMaxMatch) { code = 28; nextra = 0; extra = 0; }
    else if (l < 8) { code = l; nextra = 0; extra = 0; }
    else {
        const uint32_t e = ilog2(l) - 2;
        code = 4 * e + 4 + ((l >> e) & 3);
        nextra = e;
        extra = l & ((1u << e) - 1);
    }
}
// distance 1 .. 32768 -> code 0 .. 29
GZ_HD void dist_symbol(uint32_t dist, uint32_t &code, uint32_t &nextra, uint32_t &extra) {
    const uint32_t d = dist - 1;
    if (d < 4) { code = d; nextra = 0; extra = 0; }
    else {
        const uint32_t e = ilog2(d) - 1;
        code = 2 * e + 2 + ((d >> e) & 1);
        nextra = e;
        extra = d & ((1u << e) - 1);
    }
}
GZ_HD uint32_t pack_match(uint32_t len, uint32_t dist) { return ((len - 3) << 16) | (dist - 1); }
GZ_HD uint32_t match_length(uint32_t m) { return (m >> 16) + 3; }
GZ_HD uint32_t match_distance(uint32_t m) { return (m & 0xFFFFu) + 1; }

// freq: kNumLit literal/length counts, then kNumDist distance counts
GZ_HD void tally(uint32_t *freq, uint32_t byte, uint32_t len, uint32_t dist) {
    if (!len) DZ_ATOMIC_ADD(&freq[byte], 1u);
    else {
        uint32_t c, ne, ex;
        len_symbol(len, c, ne, ex);
        DZ_ATOMIC_ADD(&freq[257 + c], 1u);
        dist_symbol(dist, c, ne, ex);
        DZ_ATOMIC_ADD(&freq[kNumLit + c], 1u);
    }
}

// ---- code construction -------------------------------------------------------------------------------------------------------
// What one lane needs to make the lengths of one code (LDS on the device: arrays indexed by values just read).
struct CodeScratch {
    uint32_t weight[2 * kNumLit];       // leaves in order of rising count, then the inner nodes in the order they are made
    uint16_t parent[2 * kNumLit];
    uint16_t order[kNumLit];            // the used symbols by (count, symbol) rising
    uint8_t depth[2 * kNumLit];
    uint32_t count[17], next[16];       // codes per length, next code per length
    uint32_t n_used;
};
// A code needs two symbols at least (zlib's rule for what it writes; a lone distance code of length 1 would pass inflate, none at
// all needs HDIST = 1 with a zero length, which old inflaters refuse): the lowest unused symbols are counted once while the lengths
// are made (added[]: which ones, kNoSymbol = none), and not at all when the block's bits are counted (forget_added).
constexpr uint16_t kNoSymbol = 0xFFFF;
GZ_HD void at_least_two(uint32_t *freq, uint32_t n, uint16_t added[2]) {
    uint32_t used = 0, k = 0;
    added[0] = added[1] = kNoSymbol;
    for (uint32_t s = 0; s < n; ++s) used += freq[s] != 0;
    for (uint32_t s = 0; s < n && used < 2; ++s)
        if (!freq[s]) { freq[s] = 1; ++used; added[k++] = (uint16_t)s; }
}
GZ_HD void forget_added(uint32_t *freq, const uint16_t added[2]) {
    for (int k = 0; k < 2; ++k)
        if (added[k] != kNoSymbol) freq[added[k]] = 0;
}
// order[rank] = symbol, for the symbols s = lane, lane + lanes, ...: a rank is counted, not swapped into place, so the lanes of a
// wave share the work and write different slots.  Lane 0 also leaves n_used.
GZ_HD void rank_symbols(const uint32_t *freq, uint32_t n, CodeScratch &cs, uint32_t lane, uint32_t lanes) {
    uint32_t used = 0;
    if (lane == 0) {
        for (uint32_t t = 0; t < n; ++t) used += freq[t] != 0;
        cs.n_used = used;
    }
    for (uint32_t s = lane; s < n; s += lanes) {
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < n; ++t) {
            const uint32_t g = freq[t];
            r += g && (g < f || (g == f && t < s));
        }
        cs.order[r] = (uint16_t)s;
    }
}
// Huffman lengths of the ranked symbols, no longer than maxbits: the tree by two queues (sorted leaves, inner nodes as made), depths
// from the root down, lengths past the limit moved up the way zlib's gen_bitlen does it (for every pair of leaves that sit too deep a
// leaf one level above the limit's deepest used level goes down one), then the lengths dealt out again by rising count.  The code
// stays complete.  Returns how many leaves had to move (0: the tree fitted as it was).  (one lane; n_used >= 2)
GZ_HD uint32_t build_lengths(const uint32_t *freq, uint32_t n, uint32_t maxbits, uint8_t *lens, CodeScratch &cs) {
    const uint32_t m = cs.n_used;
    for (uint32_t s = 0; s < n; ++s) lens[s] = 0;
    for (uint32_t i = 0; i < m; ++i) cs.weight[i] = freq[cs.order[i]];
    uint32_t leaf = 0, inner = m, made = m;             // next unused leaf, next unused inner node, next node to make
    while (made < 2 * m - 1) {
        uint32_t sum = 0;
        for (int k = 0; k < 2; ++k) {                   // the two lightest nodes not yet under a parent; a leaf on a tie
            const uint32_t pick = (leaf < m && (inner >= made || cs.weight[leaf] <= cs.weight[inner])) ? leaf++ : inner++;
            sum += cs.weight[pick];
            cs.parent[pick] = (uint16_t)made;
        }
        cs.weight[made++] = sum;
    }
    uint32_t *const count = cs.count;
    for (uint32_t l = 0; l <= 16; ++l) count[l] = 0;
    cs.depth[2 * m - 2] = 0;
    for (uint32_t i = 2 * m - 2; i-- > 0;) {
        uint32_t d = (uint32_t)cs.depth[cs.parent[i]] + 1;
        if (d > maxbits) d = maxbits;                   // (inner nodes too: what hangs below them starts from the limit)
        cs.depth[i] = (uint8_t)d;
        if (i < m) count[d]++;
    }
    // Kraft's sum in units of 2^-maxbits: 2^maxbits for the tree as built, more once leaves were lifted to the limit.  One move
    // takes exactly one unit off: the deepest leaf above the limit goes down a level and takes a leaf of the limit's level as
    // its sibling (-2^(maxbits-bits) + 2 * 2^(maxbits-bits-1) - 1).
    uint32_t kraft = 0;
    for (uint32_t l = 1; l <= maxbits; ++l) kraft += count[l] << (maxbits - l);
    uint32_t moves = 0;
    for (; kraft > (1u << maxbits); --kraft, ++moves) {
        uint32_t bits = maxbits - 1;
        while (count[bits] == 0) --bits;
        count[bits]--;
        count[bits + 1] += 2;
        count[maxbits]--;
    }
    uint32_t i = 0;                                      // the rarest symbols take the longest codes
    for (uint32_t l = maxbits; l >= 1; --l)
        for (uint32_t k = 0; k < count[l]; ++k) lens[cs.order[i++]] = (uint8_t)l;
    return moves;
}
// canonical codes, bit-reversed: deflate writes Huffman codes most significant bit first into a stream that is filled from bit 0
GZ_HD void make_codes(const uint8_t *lens, uint32_t n, uint16_t *codes, CodeScratch &cs) {
    uint32_t *const count = cs.count, *const next = cs.next;
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) count[lens[s]]++;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s];
        codes[s] = l ? (uint16_t)gz::rev_bits(next[l]++, (int)l) : (uint16_t)0;
    }
}

// ---- bit output: 32-bit words, LSB first, zeroed in front -------------------------------------------------------------------
GZ_HD void put_bits(uint32_t *out, uint32_t bitpos, uint64_t v, uint32_t nbits) {          // nbits <= 48; v has no bits above nbits
    if (!nbits) return;
    const uint32_t w = bitpos >> 5, sh = bitpos & 31;
    DZ_ATOMIC_OR(&out[w], (uint32_t)(v << sh));
    if (sh + nbits > 32) DZ_ATOMIC_OR(&out[w + 1], (uint32_t)(v >> (32 - sh)));
    if (sh + nbits > 64) DZ_ATOMIC_OR(&out[w + 2], (uint32_t)(v >> (64 - sh)));
}

// ---- the dynamic block's header ---------------------------------------------------------------------------------------------
struct HeaderScratch {
    uint16_t rle[kNumLit + kNumDist];   // code-length symbols: symbol | extra value << 5
    uint32_t n_rle;
    uint32_t cl_freq[kNumCl];
    uint8_t cl_lens[kNumCl];
    uint16_t cl_codes[kNumCl];
    uint32_t hlit, hdist, hclen;
    uint32_t bits;                      // of the header behind the 3 block bits
};
GZ_HD uint32_t cl_extra_bits(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }
// lens: kNumLit + kNumDist lengths.  Leaves the run-length coded lengths and their code in hs (one lane; cs: scratch for the code)
GZ_HD void plan_header(const uint8_t *lens, HeaderScratch &hs, CodeScratch &cs) {
    uint32_t hlit = kNumLit, hdist = kNumDist;
    while (hlit > 257 && lens[hlit - 1] == 0) --hlit;
    while (hdist > 1 && lens[kNumLit + hdist - 1] == 0) --hdist;
    hs.hlit = hlit;
    hs.hdist = hdist;
    for (uint32_t s = 0; s < kNumCl; ++s) hs.cl_freq[s] = 0;
    // the two alphabets' lengths are one sequence (a run may cross from one into the other)
    const uint32_t total = hlit + hdist;
    uint32_t n = 0, i = 0;
    while (i < total) {
        const uint32_t v = lens[i < hlit ? i : kNumLit + (i - hlit)];
        uint32_t run = 1;
        while (i + run < total && lens[i + run < hlit ? i + run : kNumLit + (i + run - hlit)] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const uint32_t r = run < 138 ? run : 138;
                hs.rle[n++] = (uint16_t)(18 | ((r - 11) << 5));
                hs.cl_freq[18]++;
                run -= r;
            }
            if (run >= 3) {
                hs.rle[n++] = (uint16_t)(17 | ((run - 3) << 5));
                hs.cl_freq[17]++;
                run = 0;
            }
        } else {
            hs.rle[n++] = (uint16_t)v;                  // the length itself, then repeats of it
            hs.cl_freq[v]++;
            --run;
            while (run >= 3) {
                const uint32_t r = run < 6 ? run : 6;
                hs.rle[n++] = (uint16_t)(16 | ((r - 3) << 5));
                hs.cl_freq[16]++;
                run -= r;
            }
        }
        for (; run; --run) {
            hs.rle[n++] = (uint16_t)v;
            hs.cl_freq[v]++;
        }
    }
    hs.n_rle = n;
    uint16_t added[2];
    at_least_two(hs.cl_freq, kNumCl, added);
    rank_symbols(hs.cl_freq, kNumCl, cs, 0, 1);
    build_lengths(hs.cl_freq, kNumCl, 7, hs.cl_lens, cs);
    make_codes(hs.cl_lens, kNumCl, hs.cl_codes, cs);
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = 19;
    while (hclen > 4 && hs.cl_lens[order[hclen - 1]] == 0) --hclen;
    hs.hclen = hclen;
    uint32_t bits = 5 + 5 + 4 + 3 * hclen;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t sym = hs.rle[k] & 31;
        bits += hs.cl_lens[sym] + cl_extra_bits(sym);
    }
    hs.bits = bits;
}
// the header from bit `at` on (one lane); returns the first bit behind it
GZ_HD uint32_t write_header(const HeaderScratch &hs, uint32_t *out, uint32_t at) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    put_bits(out, at, (hs.hlit - 257) | ((hs.hdist - 1) << 5) | ((hs.hclen - 4) << 10), 14);
    at += 14;
    for (uint32_t k = 0; k < hs.hclen; ++k, at += 3) put_bits(out, at, hs.cl_lens[order[k]], 3);
    for (uint32_t k = 0; k < hs.n_rle; ++k) {
        const uint32_t sym = hs.rle[k] & 31, nb = hs.cl_lens[sym], ne = cl_extra_bits(sym);
        put_bits(out, at, (uint64_t)hs.cl_codes[sym] | ((uint64_t)(hs.rle[k] >> 5) << nb), nb + ne);
        at += nb + ne;
    }
    return at;
}
// bits of the block's symbols, the end-of-block code included, from the counts (symbols s = lane, lane + lanes, ...: the lanes' sums add up)
GZ_HD uint32_t body_bits(const uint32_t *freq, const uint8_t *lens, uint32_t lane, uint32_t lanes) {
    uint32_t bits = 0;
    for (uint32_t s = lane; s < kNumLit + kNumDist; s += lanes) {
        uint32_t extra = 0;
        if (s >= 257 && s < kNumLit) extra = gz::len_extra((int)(s - 257));
        else if (s >= kNumLit) extra = gz::dist_extra((int)(s - kNumLit));
        bits += freq[s] * (lens[s] + extra);
    }
    return bits;
}
// a token's bits: a literal's code, or length code, extra bits, distance code, extra bits (at most 15 + 5 + 15 + 13)
GZ_HD uint64_t literal_bits(uint32_t byte, const uint8_t *lens, const uint16_t *codes, uint32_t &nbits) {
    nbits = lens[byte];
    return codes[byte];
}
GZ_HD uint64_t match_bits(uint32_t m, const uint8_t *lens, const uint16_t *codes, uint32_t &nbits) {
    uint32_t c, ne, ex, at;
    len_symbol(match_length(m), c, ne, ex);
    uint64_t v = codes[257 + c];
    at = lens[257 + c];
    v |= (uint64_t)ex << at;
    at += ne;
    dist_symbol(match_distance(m), c, ne, ex);
    v |= (uint64_t)codes[kNumLit + c] << at;
    at += lens[kNumLit + c];
    v |= (uint64_t)ex << at;
    at += ne;
    nbits = at;
    return v;
}
// bytes of a coded piece: 3 block bits, header, symbols, then the empty stored block (3 bits, padding, 4 bytes)
GZ_HD uint32_t coded_bytes(uint32_t header_bits, uint32_t symbol_bits) { return (3 + header_bits + symbol_bits + 3 + 7) / 8 + 4; }

// ---- CRC-32 of plain bytes by slices --------------------------------------------------------------------------------------------
GZ_HD uint32_t crc_bytes(const uint32_t *table, const uint8_t *p, uint32_t n) {           // zlib's crc32(0, p, n); table[i] = gz::crc_table_entry(i)
    uint32_t v = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) v = table[(v ^ p[i]) & 0xFF] ^ (v >> 8);
    return n ? v ^ 0xFFFFFFFFu : 0u;
}
// what a slice's CRC adds to the CRC of the whole it lies in: bytes_behind = bytes of the whole behind the slice.  The whole's CRC
// is the XOR of its slices' terms (crc_combine_op is linear in crc_a).
GZ_HD uint32_t crc_term(uint32_t crc, uint64_t bytes_behind) { return crc ? gz::crc_multmodp(gz::crc_x2nmodp(bytes_behind, 3), crc) : 0u; }

// ---- a blocked run on the host -------------------------------------------------------------------------------------------------
// The host's statement of a blocked run (what k_dz_scan<true> and k_dz_gather do between them): pieces = the n_pieces(n) pieces'
// bytes back to back as a member holds them (a stored one with its 5 bytes), sizes = their lengths, crcs = the CRC-32 of every
// piece's own input.  out has bound_blocked(n) bytes; returns the bytes written.
inline uint64_t blocked_run(const uint8_t *pieces, const uint32_t *sizes, const uint32_t *crcs, uint64_t n, bool emit_empty, uint8_t *out) {
    const uint64_t np = n_pieces(n);
    if (!np) {
        if (emit_empty) put_blocked_frame(out, kBlockedFrame, 0, 0);
        return emit_empty ? kBlockedFrame : 0;
    }
    uint64_t at = 0;
    for (uint64_t i = 0; i < np; i += kBlockedPieces) {
        const uint64_t end = blocked_member_end(n, i);
        uint32_t body = 0, crc = 0;
        for (uint64_t k = i; k < i + kBlockedPieces && k < np; ++k) {
            const uint64_t piece_end = (k + 1) * kPiece < n ? (k + 1) * kPiece : n;
            for (uint32_t b = 0; b < sizes[k]; ++b) out[at + kBlockedHead + body + b] = pieces[b];
            pieces += sizes[k];
            body += sizes[k];
            crc ^= crc_term(crcs[k], end - piece_end);
        }
        put_blocked_frame(out + at, kBlockedFrame + body, crc, (uint32_t)(end - i * kPiece));
        at += kBlockedFrame + body;
    }
    return at;
}

}  // namespace dz
}  // namespace hast
