// Host driver for the BLOCKED framing of the device deflate encoder (hast_amd/csrc/dz_core.h: kBlockedPieces, put_blocked_frame,
// blocked_run): the pieces are those of tests/native/test_dz_core.cpp (its piece() is compiled in here as it stands), and what
// k_dz_scan<true> and k_dz_gather do with them is restated with plain loops -- laps of 256 "threads", a piece's place from the
// prefix sum of the sizes, a member's frame written by the thread that holds its first piece from the sizes and CRC terms as
// k_dz_piece leaves them (advanced to the end of the MEMBER).
//   test_dz_blocked [-n] IN OUT   IN as one run of blocked gzip into OUT (-n: emit_empty off, an empty run becomes nothing).  Checks
//                                 on the way: the restated kernels' bytes are dz::blocked_run's; bz::parse_header accepts every
//                                 member with an 18-byte header, at most 65 536 bytes in all and an ISIZE of at most 49 152;
//                                 bz::plan_batch walks the whole output and stops with kStopEnd; the output is no longer than
//                                 dz::bound_blocked, and is the ordinary member's size - 20 + 28 a member.
//                                 Prints "pieces stored bytes members ordinary_bytes".
// (the caller inflates OUT with zlib, member after member, and compares)
#define main test_dz_core_main
#include "test_dz_core.cpp"
#undef main

#include "../../hast_amd/csrc/bz_core.h"

static void check(bool ok, const char *what) {
    if (!ok) {
        fprintf(stderr, "test_dz_blocked: %s\n", what);
        exit(2);
    }
}

int main(int argc, char **argv) {
    bool emit_empty = true;
    if (argc == 4 && !strcmp(argv[1], "-n")) {
        emit_empty = false;
        ++argv;
        --argc;
    }
    check(argc == 3, "usage: test_dz_blocked [-n] IN OUT");
    std::vector<uint8_t> data;
    {
        FILE *f = fopen(argv[1], "rb");
        check(f != nullptr, "cannot open the input");
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
        fclose(f);
    }
    const uint64_t n = data.size(), np = n_pieces(n);
    uint32_t crc_table[256];
    for (uint32_t i = 0; i < 256; ++i) crc_table[i] = gz::crc_table_entry(i);

    // ---- k_dz_piece: every piece's bytes, its size word and its CRC term (blocked: advanced to the end of its member) ----
    Counters ct;
    std::vector<uint8_t> pieces;                            // the pieces' bytes back to back (a stored one with its 5 bytes)
    std::vector<uint32_t> plain_crc(np), term(np), size_word(np);
    for (uint64_t i = 0; i < np; ++i) {
        const uint64_t off = i * kPiece;
        const uint32_t m = (uint32_t)(n - off < kPiece ? n - off : kPiece);
        piece(data.data() + off, m, pieces, ct);
        size_word[i] = ct.sizes[i] > m ? (m | kStoredFlag) : ct.sizes[i];     // (what the kernel leaves in ws.sizes)
        const uint32_t slice = (m + 63) / 64;
        uint32_t pc = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t lo = lane * slice < m ? lane * slice : m, hi = lo + slice < m ? lo + slice : m;
            pc ^= crc_term(crc_bytes(crc_table, data.data() + off + lo, hi - lo), m - hi);
        }
        check(pc == crc_bytes(crc_table, data.data() + off, m), "a piece's CRC-32 by slices differs from the bytewise one");
        plain_crc[i] = pc;
        term[i] = crc_term(pc, blocked_member_end(n, i) - off - m);
    }

    // ---- k_dz_scan<true>: laps of 256 pieces ----
    const uint64_t cap = bound_blocked(n);
    std::vector<uint8_t> out(cap + 64, 0xA5);
    std::vector<uint64_t> offs(np);
    uint64_t total = 0, members = 0;
    if (np == 0) {
        if (emit_empty) {
            put_blocked_frame(out.data(), kBlockedFrame, 0, 0);
            total = kBlockedFrame;
            members = 1;
        }
    } else {
        uint64_t at = 0;
        for (uint64_t c = 0; c < np; c += 256) {
            uint64_t scan[256], sz[256];
            for (uint32_t tid = 0; tid < 256; ++tid) {
                const uint64_t i = c + tid;
                sz[tid] = 0;
                if (i < np) sz[tid] = (size_word[i] & kStoredFlag) ? (uint64_t)(size_word[i] & ~kStoredFlag) + 5 : size_word[i];
                scan[tid] = sz[tid] + (tid ? scan[tid - 1] : 0);
            }
            for (uint32_t tid = 0; tid < 256; ++tid) {
                const uint64_t i = c + tid;
                if (i >= np) continue;
                const uint64_t in_front = at + scan[tid] - sz[tid];
                offs[i] = in_front + (i / kBlockedPieces) * kBlockedFrame + kBlockedHead;
                if (i % kBlockedPieces) continue;
                uint32_t mtotal = kBlockedFrame + (uint32_t)sz[tid], crc = term[i];
                for (uint64_t k = i + 1; k < i + kBlockedPieces && k < np; ++k) {      // (pieces of the next lap among them: member 85)
                    mtotal += (size_word[k] & kStoredFlag) ? (size_word[k] & ~kStoredFlag) + 5 : size_word[k];
                    crc ^= term[k];
                }
                const uint64_t start = in_front + (i / kBlockedPieces) * kBlockedFrame;
                check(start + mtotal <= cap, "a member ends behind the bound");
                put_blocked_frame(out.data() + start, mtotal, crc, (uint32_t)(blocked_member_end(n, i) - i * kPiece));
                ++members;
            }
            at += scan[255];
        }
        total = at + n_members(n) * kBlockedFrame;
        check(members == n_members(n), "not a member per three pieces");
        // ---- k_dz_gather: every piece to its place ----
        const uint8_t *from = pieces.data();
        for (uint64_t i = 0; i < np; ++i) {
            check(offs[i] + ct.sizes[i] <= cap, "a piece ends behind the bound");
            memcpy(out.data() + offs[i], from, ct.sizes[i]);
            from += ct.sizes[i];
        }
    }
    check(total <= cap, "the run is longer than the bound");
    for (uint64_t i = total; i < out.size(); ++i) check(out[i] == 0xA5, "a byte behind the run was written");
    if (ct.stored == ct.pieces) check(total == (n || emit_empty ? cap : 0), "stored pieces alone do not reach the bound exactly");

    // ---- the same from dz_core.h's host function ----
    {
        std::vector<uint8_t> want(cap + 1);
        const uint64_t got = blocked_run(pieces.data(), ct.sizes.data(), plain_crc.data(), n, emit_empty, want.data());
        check(got == total && !memcmp(want.data(), out.data(), total), "the restated kernels and dz::blocked_run differ");
    }
    // ---- against the ordinary member of the same pieces ----
    const uint64_t ordinary = kMemberHead + pieces.size() + kMemberTail;
    if (n) check(total == ordinary - 20 + kBlockedFrame * n_members(n), "not the ordinary member's size - 20 + 28 a member");

    // ---- BGZF's rules, member by member, and the project's batch plan ----
    {
        uint64_t at = 0, seen = 0, in_at = 0;
        while (at < total) {
            size_t hdr = 0, mt = 0;
            check(bz::parse_header(out.data() + at, total - at, hdr, mt), "bz::parse_header refuses a member");
            check(hdr == 18 && mt <= bz::kMaxMember && at + mt <= total, "a member's header or size");
            const uint8_t *t = out.data() + at + mt - 8;
            const uint32_t crc = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
            const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
            check(isize <= kBlockedInput && in_at + isize <= n && (isize == kBlockedInput || in_at + isize == n), "a member's ISIZE");
            check(crc == crc_bytes(crc_table, data.data() + in_at, isize), "a member's CRC-32");
            in_at += isize;
            at += mt;
            ++seen;
        }
        check(at == total && seen == members && in_at == n, "the members do not tile the run");
        std::vector<bz::Member> plan(members + 1);
        const bz::Plan pl = bz::plan_batch(out.data(), total, true, (size_t)total + 1, (size_t)n + 1, 0, plan.data(), plan.size());
        check(pl.stop == bz::kStopEnd && pl.n_members == members && pl.resume == total && pl.out_bytes == n, "bz::plan_batch does not walk the whole run");
    }
    if (n == 0 && emit_empty) {
        const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        check(total == 28 && !memcmp(out.data(), eof, 28), "an empty run is not BGZF's end-of-file block");
    }
    FILE *f = fopen(argv[2], "wb");
    check(f && fwrite(out.data(), 1, total, f) == total, "cannot write the output");
    fclose(f);
    printf("%llu %llu %llu %llu %llu\n", (unsigned long long)ct.pieces, (unsigned long long)ct.stored, (unsigned long long)total, (unsigned long long)members,
           (unsigned long long)ordinary);
    return 0;
}
