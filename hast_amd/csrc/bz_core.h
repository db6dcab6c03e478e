// bz_core.h -- the rules of BLOCKED gzip (BGZF: bgzip, htslib, many sequencer pipelines), written once for the host reader
// (bgzf_reader.h), the device stream (bz_api.cpp, bz_kernels.hip) and the native test (tests/native/test_bz_core.cpp).  Plain
// integer code, no HIP calls, as sq_core.h / rs_core.h / dz_core.h are.
//
// A BGZF file is a series of gzip members of at most 64 KB of data each.  Every member's header carries the member's compressed
// size (the `BC` subfield of the extra field), its trailer carries CRC-32 and inflated size, and no match may reach in front of its
// member.  So the members of a stretch of the file are found WITHOUT inflating anything, their places in the output are one prefix
// sum, and every member is decoded from a known start with no history -- by a host thread each (bgzf_reader.h) or by a wave each
// (k_bz_inflate).  Here: the header rule, the record a kernel reads per member, and the plan of a batch of whole members.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BZ_HD __host__ __device__ inline
#else
#define BZ_HD inline
#endif

namespace hast {
namespace bz {

constexpr uint32_t kMaxIsize = 1u << 16;      // what a member may inflate to
constexpr size_t kMaxMember = 1u << 16;       // ... and its whole size (BSIZE is 16 bits: total - 1)
constexpr size_t kMinHeader = 18;             // a header with the BC subfield alone

// The header rule: a gzip header with FEXTRA only and a `BC` subfield of length 2 anywhere in the part of the extra field that is
// there (h[0 .. n)); hdr = header bytes, total = the whole member's bytes (header + deflate data + 8 bytes of trailer).
BZ_HD bool parse_header(const unsigned char *h, size_t n, size_t &hdr, size_t &total) {
    if (n < kMinHeader || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 4) == 0) return false;
    if (h[3] & ~4u) return false;                              // BGZF writers set FEXTRA only
    const size_t xlen = h[10] | ((size_t)h[11] << 8);
    // the BC subfield is the first one in every known writer; look through the part we have
    const size_t lim = n < 12 + xlen ? n : 12 + xlen;
    size_t p = 12;
    while (p + 4 <= lim) {
        const size_t slen = h[p + 2] | ((size_t)h[p + 3] << 8);
        if (h[p] == 'B' && h[p + 1] == 'C' && slen == 2 && p + 6 <= n) {
            total = (size_t)(h[p + 4] | ((size_t)h[p + 5] << 8)) + 1;
            hdr = 12 + xlen;
            return total >= hdr + 8 + 2;
        }
        p += 4 + slen;
    }
    return false;
}

// What a kernel reads per member.  Bit positions count from the first bit of the batch's input words.
struct Member {
    uint64_t first_bit;         // the first bit of the deflate data
    uint64_t end_bit;           // one past the last input bit: the first bit of the trailer (the byte in front of it is the last one read as data)
    uint64_t out_off;           // the member's first byte in the batch's output
    uint32_t isize;             // bytes it inflates to (<= kMaxIsize)
    uint32_t crc;               // wanted CRC-32
};
static_assert(sizeof(Member) == 32, "Member is copied to the device as it is");

// why a member is refused (one word per member, bits 0-7; bits 8.. = gz_core.h's error code where there is one)
enum : uint32_t {
    kBadNone = 0,
    kBadDeflate = 1,            // not valid deflate
    kBadCutShort = 2,           // the deflate data runs into the trailer
    kBadTooLong = 3,            // inflates to more than ISIZE
    kBadTooShort = 4,           // ... to less
    kBadCrc = 5,
    kBadTooFar = 6              // a match reaches in front of the member's first byte
};
BZ_HD const char *bad_text(uint32_t why) {
    switch (why & 0xFF) {
    case kBadDeflate: return "invalid deflate data";
    case kBadCutShort: return "the deflate data does not end in front of the trailer";
    case kBadTooLong: return "more bytes than ISIZE says";
    case kBadTooShort: return "fewer bytes than ISIZE says";
    case kBadCrc: return "CRC-32 mismatch";
    case kBadTooFar: return "a match reaches in front of its block";
    default: return "no error";
    }
}

// The ring of a member's most recent BYTES in LDS (k_bz_inflate): the predicates are those of gz_core.h's ring of 512 symbols, the
// ring holds twice as many bytes in the same LDS.
constexpr uint32_t kRing = 1024;
BZ_HD bool ring_holds_long_match(uint32_t distance, uint32_t len) { return distance >= len ? distance <= kRing : distance <= kRing - 256; }

// ---- the batch plan ---------------------------------------------------------------------------------------------------------------
// what the walk met behind the last member it took
enum Stop : uint32_t {
    kStopFull = 0,              // the next member does not fit the batch's limits: it is there, whole
    kStopEnd,                   // end of input
    kStopCut,                   // a member (or its header) is cut by the end of the bytes present and more may come: carry it
    kStopTruncated,             // ... and no more will come: the file ends inside a block
    kStopTooLarge,              // a member claims more than 64 KB (error, as the host reader)
    kStopNotGzip,               // bytes that do not start with 1f 8b: end of stream, ignored as gzread does
    kStopNotBgzf                // a gzip member that is not BGZF: unsupported from here
};
struct Plan {
    size_t n_members = 0;
    size_t resume = 0;          // bytes of p[] the batch's members take: the walk resumes here
    uint64_t out_bytes = 0;
    Stop stop = kStopEnd;
};

// The next batch: whole members from p[0] on while they fit batch_in_bytes of input and batch_out_bytes of output (both raised so
// that one member always fits) and `cap` records.  at_eof: no byte follows p[n - 1].  bit_base: the bit of the batch's input words
// at which p[0] lies.
inline Plan plan_batch(const unsigned char *p, size_t n, bool at_eof, size_t batch_in_bytes, size_t batch_out_bytes, uint64_t bit_base, Member *out, size_t cap) {
    Plan pl;
    if (batch_in_bytes < kMaxMember) batch_in_bytes = kMaxMember;
    if (batch_out_bytes < kMaxIsize) batch_out_bytes = kMaxIsize;
    size_t at = 0;
    for (;;) {
        const size_t have = n - at;
        if (have == 0) { pl.stop = at_eof ? kStopEnd : kStopCut; break; }
        const unsigned char *q = p + at;
        // (fewer than two bytes: a lone 1f may begin a member)
        if (q[0] != 0x1f || (have >= 2 && q[1] != 0x8b)) { pl.stop = kStopNotGzip; break; }
        if (have < kMinHeader) { pl.stop = at_eof ? kStopTruncated : kStopCut; break; }
        size_t hdr = 0, total = 0;
        if (!parse_header(q, have, hdr, total)) {
            // (the BC subfield may lie behind what is there of a long extra field)
            const size_t xlen = q[10] | ((size_t)q[11] << 8);
            const bool fextra_only = q[2] == 8 && q[3] == 4;
            if (fextra_only && have < 12 + xlen && !at_eof) { pl.stop = kStopCut; break; }
            pl.stop = kStopNotBgzf;
            break;
        }
        if (have < total) { pl.stop = at_eof ? kStopTruncated : kStopCut; break; }
        const unsigned char *t = q + total - 8;
        const uint32_t crc = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        if (isize > kMaxIsize) { pl.stop = kStopTooLarge; break; }
        if (pl.n_members && (pl.n_members >= cap || at + total > batch_in_bytes || pl.out_bytes + isize > batch_out_bytes)) { pl.stop = kStopFull; break; }
        Member &m = out[pl.n_members++];
        m.first_bit = bit_base + (uint64_t)(at + hdr) * 8;
        m.end_bit = bit_base + (uint64_t)(at + total - 8) * 8;
        m.out_off = pl.out_bytes;
        m.isize = isize;
        m.crc = crc;
        pl.out_bytes += isize;
        at += total;
    }
    pl.resume = at;
    return pl;
}

}  // namespace bz
}  // namespace hast
