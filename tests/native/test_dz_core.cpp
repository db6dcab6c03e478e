// Host driver for hast_amd/csrc/dz_core.h (the device deflate encoder's per-piece code): the steps a wave of k_dz_piece takes are
// restated here with plain loops over the SAME functions -- 64 "lanes" one after the other where the kernel has them side by side.
//   test_dz_core IN OUT      compresses IN into one gzip member OUT; checks on the way that every code is complete and within its
//                            length limit, that the member is no longer than dz::bound, that gz_core.h's decode_chunk reads it back
//                            to IN's bytes (the project's decoder against its encoder, no zlib in between) and that the trailer's
//                            CRC-32 (slices + GF(2) operators, as on the device) is the bytewise one.  Prints "pieces stored bytes limited"
//                            (limited: pieces whose literal/length code had to be brought under 15 bits).
//   test_dz_core -H IN OUT   the same without the match search (what HAST_DZ_LITERALS_ONLY asks of the kernel): the symbol
//                            histogram is the input's byte histogram, which is how a test gets at a chosen histogram
//   test_dz_core -v [-H] IN OUT   either of them with a second line of output: the bytes every piece takes in the member, in order (a
//                            stored piece: its bytes + 5).  The member is 10 bytes of header, these, 10 bytes of trailer: a test that
//                            compares the member with the kernel's can name the piece a difference lies in.
//   test_dz_core -s          len_symbol over 3 .. 258 and dist_symbol over 1 .. 32768 against gz_core.h's base / extra-bit tables (what the
//                            decoder adds up): also the distances no 16-KB piece can hold (codes 28, 29), for the day the piece grows
//   test_dz_core -P          prints the piece size
//   test_dz_core -k N        code lengths for a Fibonacci-like histogram of N symbols (unlimited lengths pass 15 from N = 17 on):
//                            checks the limit and completeness, prints the longest length
// (the caller inflates OUT with zlib and compares)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../hast_amd/csrc/dz_core.h"

using namespace hast;
using namespace hast::dz;

static void fail(const char *what) {
    fprintf(stderr, "test_dz_core: %s\n", what);
    exit(2);
}

static void check_code(const uint8_t *lens, uint32_t n, uint32_t maxbits, const char *what) {
    uint32_t used = 0;
    for (uint32_t s = 0; s < n; ++s) {
        if (lens[s] > maxbits) fail((std::string(what) + ": a code longer than its limit").c_str());
        used += lens[s] != 0;
    }
    if (used < 2 || !gz::complete(lens, (int)n, false)) fail((std::string(what) + ": not a complete code").c_str());
}

static uint32_t popc_below(uint64_t m, uint32_t lane) { return (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1)); }

static bool g_literals_only = false;

struct Counters {
    uint64_t pieces = 0, stored = 0, limited = 0;
    std::vector<uint32_t> sizes;                        // bytes of every piece in the member
};

// one piece -> its bytes, appended to out
static void piece(const uint8_t *src, uint32_t n, std::vector<uint8_t> &outb, Counters &ct) {
    static uint8_t in[kPiece + 8];
    static uint32_t table[kHashSize], freq[kNumLit + kNumDist], matches[kMaxMatches], out[kOutWords + 2];
    static uint64_t startm[kPiece / 64], matchm[kPiece / 64];
    static uint8_t lens[kNumLit + kNumDist];
    static uint16_t codes[kNumLit + kNumDist];
    static CodeScratch cs;
    static HeaderScratch hs;
    memcpy(in, src, n);
    memset(in + n, 0, 8);
    memset(table, 0, sizeof table);
    memset(freq, 0, sizeof freq);
    uint32_t pos = 0, nm = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        uint32_t len[64], dist[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            len[lane] = dist[lane] = 0;
            if (base + lane < n && !g_literals_only) probe(in, n, table, base + lane, len[lane], dist[lane]);
        }
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (base + lane < n) enter(in, n, table, base + lane);
        uint64_t sm = 0, mm = 0;
        const uint32_t end = base + 64 < n ? base + 64 : n;
        while (pos < end) {
            const uint32_t i = pos - base;
            sm |= 1ull << i;
            if (len[i]) {
                mm |= 1ull << i;
                pos += len[i];
            } else ++pos;
        }
        for (uint32_t lane = 0; lane < 64; ++lane) {
            if (!((sm >> lane) & 1)) continue;
            const bool is_match = (mm >> lane) & 1;
            if (is_match) {
                // every candidate was verified: say so again here, where a wrong match would become wrong output
                if (dist[lane] == 0 || dist[lane] > base + lane || len[lane] < kMinMatch || len[lane] > kMaxMatch) fail("a match out of range");
                for (uint32_t k = 0; k < len[lane]; ++k)
                    if (in[base + lane + k] != in[base + lane + k - dist[lane]]) fail("a match that does not match");
                if (nm + popc_below(mm, lane) >= kMaxMatches) fail("more matches than a piece can hold");
                matches[nm + popc_below(mm, lane)] = pack_match(len[lane], dist[lane]);
            }
            tally(freq, in[base + lane], is_match ? len[lane] : 0, dist[lane]);
        }
        nm += (uint32_t)__builtin_popcountll(mm);
        startm[base / 64] = sm;
        matchm[base / 64] = mm;
    }
    if (pos != n) fail("the parse does not end at the piece's end");
    freq[256] = 1;
    uint16_t added_lit[2], added_dist[2];
    at_least_two(freq, kNumLit, added_lit);
    at_least_two(freq + kNumLit, kNumDist, added_dist);
    for (uint32_t lane = 0; lane < 64; ++lane) rank_symbols(freq, kNumLit, cs, lane, 64);
    ct.limited += build_lengths(freq, kNumLit, 15, lens, cs) != 0;
    for (uint32_t lane = 0; lane < 64; ++lane) rank_symbols(freq + kNumLit, kNumDist, cs, lane, 64);
    build_lengths(freq + kNumLit, kNumDist, 15, lens + kNumLit, cs);
    forget_added(freq, added_lit);
    forget_added(freq + kNumLit, added_dist);
    make_codes(lens, kNumLit, codes, cs);
    make_codes(lens + kNumLit, kNumDist, codes + kNumLit, cs);
    plan_header(lens, hs, cs);
    check_code(lens, kNumLit, 15, "literal/length");
    check_code(lens + kNumLit, kNumDist, 15, "distance");
    check_code(hs.cl_lens, kNumCl, 7, "code-length");
    uint32_t sym_bits = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) sym_bits += body_bits(freq, lens, lane, 64);
    const uint32_t cb = coded_bytes(hs.bits, sym_bits);
    ct.pieces++;
    if (cb >= n) {
        ct.stored++;
        const uint8_t h[5] = {0, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
        outb.insert(outb.end(), h, h + 5);
        outb.insert(outb.end(), src, src + n);
        ct.sizes.push_back(n + 5);
        return;
    }
    memset(out, 0, sizeof out);
    put_bits(out, 0, 4, 3);                             // BFINAL = 0, BTYPE = 10b
    uint32_t at = write_header(hs, out, 3);
    if (at != 3 + hs.bits) fail("the header is not as long as planned");
    nm = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint64_t sm = startm[base / 64], mm = matchm[base / 64];
        uint32_t nb[64];
        uint64_t v[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            nb[lane] = 0;
            v[lane] = 0;
            if (!((sm >> lane) & 1)) continue;
            if ((mm >> lane) & 1) v[lane] = match_bits(matches[nm + popc_below(mm, lane)], lens, codes, nb[lane]);
            else v[lane] = literal_bits(in[base + lane], lens, codes, nb[lane]);
            if (nb[lane] == 0) fail("a symbol without a code");
        }
        uint32_t run = at;                              // (the wave's prefix sum)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            put_bits(out, run, v[lane], nb[lane]);
            run += nb[lane];
        }
        at = run;
        nm += (uint32_t)__builtin_popcountll(mm);
    }
    put_bits(out, at, codes[256], lens[256]);
    at += lens[256];
    if (at != 3 + hs.bits + sym_bits) fail("the symbols are not as long as counted");
    at = (at + 3 + 7) & ~7u;                            // the empty stored block: 000b, padding ...
    put_bits(out, at, 0xFFFF0000u, 32);                 // ... LEN = 0, NLEN = FFFF
    at += 32;
    if (at != cb * 8) fail("the piece is not as long as planned");
    const uint8_t *ob = reinterpret_cast<const uint8_t *>(out);
    outb.insert(outb.end(), ob, ob + cb);
    ct.sizes.push_back(cb);
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "-P")) {
        printf("%u\n", kPiece);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "-s")) {
        uint32_t used_len = 0, used_dist = 0;
        for (uint32_t len = 3; len <= kMaxMatch; ++len) {
            uint32_t c, ne, ex;
            len_symbol(len, c, ne, ex);
            if (c > 28 || ne != gz::len_extra((int)c) || ex >= (1u << ne) || gz::len_base((int)c) + ex != len || (len == 258) != (c == 28)) fail("len_symbol");
            used_len |= 1u << c;
        }
        for (uint32_t dist = 1; dist <= 32768; ++dist) {
            uint32_t c, ne, ex;
            dist_symbol(dist, c, ne, ex);
            if (c > 29 || ne != gz::dist_extra((int)c) || ex >= (1u << ne) || gz::dist_base((int)c) + ex != dist) fail("dist_symbol");
            used_dist |= 1u << c;
            if (match_distance(pack_match(3 + dist % 256, dist)) != dist || match_length(pack_match(3 + dist % 256, dist)) != 3 + dist % 256) fail("pack_match");
        }
        if (used_len != (1u << 29) - 1 || used_dist != (1u << 30) - 1) fail("a length or distance code that nothing maps to");
        printf("ok\n");
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "-k")) {
        const uint32_t n = (uint32_t)atoi(argv[2]);
        if (n < 2 || n > kNumLit) fail("-k: 2 .. 286");
        static uint32_t freq[kNumLit];
        static uint8_t lens[kNumLit];
        static CodeScratch cs;
        uint64_t a = 1, b = 1;
        for (uint32_t s = 0; s < n; ++s) {              // 1, 1, 2, 3, 5, ...: the deepest Huffman tree there is; capped where u32 ends
            freq[s] = a > 0x7FFFFFull ? 0x7FFFFFu + s : (uint32_t)a;
            const uint64_t c = a + b;
            a = b;
            b = c;
        }
        for (uint32_t lane = 0; lane < 64; ++lane) rank_symbols(freq, kNumLit, cs, lane, 64);
        build_lengths(freq, kNumLit, 15, lens, cs);
        check_code(lens, kNumLit, 15, "skewed");
        uint32_t longest = 0;
        for (uint32_t s = 0; s < n; ++s) longest = lens[s] > longest ? lens[s] : longest;
        printf("%u\n", longest);
        return 0;
    }
    bool piece_sizes = false;
    if (argc >= 4 && !strcmp(argv[1], "-v")) {
        piece_sizes = true;
        ++argv;
        --argc;
    }
    if (argc == 4 && !strcmp(argv[1], "-H")) {
        g_literals_only = true;
        ++argv;
        --argc;
    }
    if (argc != 3) fail("usage: test_dz_core [-v] [-H] IN OUT | -P | -s | -k N");
    std::vector<uint8_t> data;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) fail("cannot open the input");
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
        fclose(f);
    }
    const uint64_t n = data.size();
    std::vector<uint8_t> gzb = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    Counters ct;
    uint32_t crc_table[256];
    for (uint32_t i = 0; i < 256; ++i) crc_table[i] = gz::crc_table_entry(i);
    uint32_t crc = 0;
    for (uint64_t off = 0; off < n; off += kPiece) {
        const uint32_t m = (uint32_t)(n - off < kPiece ? n - off : kPiece);
        piece(data.data() + off, m, gzb, ct);
        // the piece's CRC: 64 slices (a lane each), combined; then the piece's term of the member's CRC
        const uint32_t slice = (m + 63) / 64;
        uint32_t pc = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t lo = lane * slice < m ? lane * slice : m, hi = lo + slice < m ? lo + slice : m;
            pc ^= crc_term(crc_bytes(crc_table, data.data() + off + lo, hi - lo), m - hi);
        }
        crc ^= crc_term(pc, n - off - m);
    }
    if (crc != crc_bytes(crc_table, data.data(), (uint32_t)n) && n < (1ull << 32)) fail("CRC-32 by slices differs from the bytewise one");
    gzb.push_back(3);
    gzb.push_back(0);
    for (int k = 0; k < 4; ++k) gzb.push_back((uint8_t)(crc >> (8 * k)));
    for (int k = 0; k < 4; ++k) gzb.push_back((uint8_t)(n >> (8 * k)));
    if (gzb.size() > bound(n)) fail("the member is longer than the bound");
    {   // the project's own decoder
        std::vector<uint32_t> w((gzb.size() + 3) / 4 + 8, 0);
        memcpy(w.data(), gzb.data(), gzb.size());
        std::vector<uint32_t> tabs(gz::kTabWords);
        std::vector<uint16_t> sym(n + 1024);
        gz::ChunkJob job;
        memset(&job, 0, sizeof job);
        job.from_bit = job.start_bit = kMemberHead * 8;
        job.stop_bit = ~0ull;
        job.sym_cap = (uint32_t)sym.size();
        job.flags = gz::kJobKnown | gz::kJobNoHistory;
        gz::decode_chunk(job, w.data(), (uint64_t)gzb.size() * 8, tabs.data(), sym.data());
        if (!(job.status & gz::kStFinal) || (job.status & gz::kStError)) fail("decode_chunk does not reach the final block");
        if (job.n_out != n) fail("decode_chunk: another length");
        for (uint64_t i = 0; i < n; ++i)
            if (sym[i] != data[i]) fail("decode_chunk: other bytes");
        if ((job.end_bit + 7) / 8 + 8 != gzb.size()) fail("decode_chunk: the trailer is not where the final block ends");
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(gzb.data(), 1, gzb.size(), f) != gzb.size()) fail("cannot write the output");
    fclose(f);
    printf("%llu %llu %llu %llu\n", (unsigned long long)ct.pieces, (unsigned long long)ct.stored, (unsigned long long)gzb.size(), (unsigned long long)ct.limited);
    if (piece_sizes) {
        for (size_t i = 0; i < ct.sizes.size(); ++i) printf(i ? " %u" : "%u", ct.sizes[i]);
        printf("\n");
    }
    return 0;
}
