// test_bz_core.cpp -- bz_core.h on the CPU: a blocked-gzip file is walked piece by piece as bz_api.cpp's producer does (plan_batch,
// a cut member carried to the front of the next piece), every planned member is decoded with gz_core.h's lane decoder from its known
// start with no history, and held to ISIZE and CRC-32 with the helpers k_bz_crc uses (256 slices, crc_x2nmodp / crc_combine_op).
//   test_bz_core FILE BATCH_IN BATCH_OUT PIECE
// stdout: the bytes of the members in front of the first bad one; stderr: one line "verdict ok members=N batches=B carried=C" or
// "verdict bad member=I reason=R offset=O".  Built by tests/test_bz_core_cpu.py with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/bz_core.h"
#include "../../hast_amd/csrc/gz_core.h"

using namespace hast;

static uint32_t crc_by_slices(const uint8_t *s, uint32_t n) {      // k_bz_crc, lane by lane
    if (!n) return 0;
    uint32_t tab[256], part[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = gz::crc_table_entry(i);
    const uint32_t slice = (n + 255) / 256;
    for (uint32_t tid = 0; tid < 256; ++tid) {
        const long long hi = (long long)n - (long long)(255 - tid) * slice, lo = hi - slice;
        uint32_t v = 0xFFFFFFFFu;
        for (long long i = lo < 0 ? 0 : lo; i < hi; ++i) v = tab[(v ^ s[i]) & 0xFF] ^ (v >> 8);
        part[tid] = hi <= 0 ? 0u : v ^ 0xFFFFFFFFu;
    }
    uint32_t xk = gz::crc_x2nmodp(slice, 3);
    for (uint32_t st = 1; st < 256; st <<= 1) {
        for (uint32_t tid = 0; tid < 256; tid += 2 * st) part[tid] = gz::crc_combine_op(part[tid], part[tid + st], xk);
        xk = gz::crc_multmodp(xk, xk);
    }
    return part[0];
}

static const char *decode_member(const bz::Member &m, const uint32_t *w, std::vector<uint32_t> &tabs, std::vector<uint16_t> &sym, std::vector<uint8_t> &bytes) {
    gz::ChunkJob job;
    memset(&job, 0, sizeof job);
    job.from_bit = job.start_bit = m.first_bit;
    job.stop_bit = ~0ull;
    job.sym_cap = m.isize + 264;                   // (the lane decoder wants 260 symbols of room in front of every token)
    job.flags = gz::kJobKnown | gz::kJobNoHistory;
    sym.assign(job.sym_cap + 8, 0);
    gz::decode_chunk(job, w, m.end_bit, tabs.data(), sym.data());
    if (job.status & gz::kStError) return job.err_code == gz::kErrTooFar ? "too_far" : "deflate";
    if ((job.status & gz::kStNoRoom) || job.n_out > m.isize) return "too_long";
    if (job.status & gz::kStStarved) return "cut_short";
    if (!(job.status & gz::kStFinal)) return "deflate";
    if (job.end_bit > m.end_bit) return "cut_short";
    if (job.n_out < m.isize) return "too_short";
    bytes.resize(m.isize);
    for (uint32_t i = 0; i < m.isize; ++i) {
        if (sym[i] > 0xFF) return "too_far";       // (a marker: cannot be, with no history)
        bytes[i] = (uint8_t)sym[i];
    }
    if (crc_by_slices(bytes.data(), m.isize) != m.crc) return "crc";
    return nullptr;
}

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: test_bz_core FILE BATCH_IN BATCH_OUT PIECE\n");
        return 2;
    }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> file;
    {
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, fp)) > 0) file.insert(file.end(), buf, buf + n);
        fclose(fp);
    }
    const size_t batch_in = (size_t)atol(argv[2]), batch_out = (size_t)atol(argv[3]), piece = (size_t)atol(argv[4]);
    {   // the open's rule
        size_t hdr, total;
        if (!bz::parse_header(file.data(), file.size(), hdr, total)) {
            fprintf(stderr, "verdict unsupported_at_open\n");
            return 0;
        }
    }
    std::vector<uint8_t> buf, bytes;
    std::vector<bz::Member> mem(1 << 16);
    std::vector<uint32_t> tabs(gz::kTabWords), words;
    std::vector<uint16_t> sym;
    size_t file_pos = 0, members = 0, batches = 0, carried = 0;
    bool eof = false;
    for (;;) {
        const uint64_t batch_off = file_pos - buf.size();
        if (!eof) {
            const size_t n = std::min(piece, file.size() - file_pos);
            buf.insert(buf.end(), file.begin() + (long)file_pos, file.begin() + (long)(file_pos + n));
            file_pos += n;
            eof = file_pos >= file.size();
        }
        const bz::Plan pl = bz::plan_batch(buf.data(), buf.size(), eof, batch_in, batch_out, 0, mem.data(), mem.size());
        // the batch's words: exactly the bytes its members take, zeros behind them
        words.assign(pl.resume / 4 + 64, 0);
        if (pl.resume) memcpy(words.data(), buf.data(), pl.resume);
        uint64_t expect_off = 0;
        for (size_t i = 0; i < pl.n_members; ++i) {
            const bz::Member &m = mem[i];
            if (m.out_off != expect_off || m.isize > bz::kMaxIsize || m.end_bit < m.first_bit || m.end_bit + 64 > (uint64_t)pl.resume * 8) {
                fprintf(stderr, "the plan is wrong at member %zu\n", members + i);
                return 1;
            }
            expect_off += m.isize;
            if (const char *why = decode_member(m, words.data(), tabs, sym, bytes)) {
                fflush(stdout);
                fprintf(stderr, "verdict bad member=%zu reason=%s offset=%llu\n", members + i, why, (unsigned long long)(batch_off + (m.first_bit >> 3)));
                return 0;
            }
            if (m.isize) fwrite(bytes.data(), 1, m.isize, stdout);
        }
        if (expect_off != pl.out_bytes) return 1;
        if (pl.n_members > 1 && (pl.resume > std::max(batch_in, bz::kMaxMember) || pl.out_bytes > std::max<size_t>(batch_out, bz::kMaxIsize))) {
            fprintf(stderr, "a batch is over its limits\n");
            return 1;
        }
        members += pl.n_members;
        batches += pl.n_members ? 1 : 0;
        const uint64_t stop_off = batch_off + pl.resume;
        const char *bad = nullptr;
        switch (pl.stop) {
        case bz::kStopFull: break;
        case bz::kStopCut:
            if (eof) return 1;                      // (at the end of the input a cut member is a truncated one)
            carried += pl.resume < buf.size();
            break;
        case bz::kStopEnd:
        case bz::kStopNotGzip:
            fflush(stdout);
            fprintf(stderr, "verdict ok members=%zu batches=%zu carried=%zu\n", members, batches, carried);
            return 0;
        case bz::kStopTruncated: bad = "truncated"; break;
        case bz::kStopTooLarge: bad = "too_large"; break;
        case bz::kStopNotBgzf: bad = "not_bgzf"; break;
        }
        if (bad) {
            fflush(stdout);
            fprintf(stderr, "verdict bad member=%zu reason=%s offset=%llu\n", members, bad, (unsigned long long)stop_off);
            return 0;
        }
        buf.erase(buf.begin(), buf.begin() + (long)pl.resume);
    }
}
