// Host driver of the read rows (hast_amd/csrc/rr_core.h against the model of rr_host.h).
//   test_rr_core -s N SEED
//       the density text of rr_core.h against snprintf("%0.6f") over: every v, t in 1..3000; v in 1..200000 over every t = 2^k, k < 32;
//       the extremes; N pairs of random 32-bit words.  Per case also row_bytes against the text's length, and q against an exact
//       128-bit restatement, which also says whether the case is a tie.  One line on stdout:
//           cases <n> diffs <n> ties_down <n> ties_up <n>
//   test_rr_core -D grid | ties | extremes | rand N SEED
//       the same cases, one at a time in a fixed order (grid: t outer, v inner; ties: k outer, v inner), the text of D per line
//   test_rr_core -f fasta|fastq -t T0,T1 file...
//       every file framed as one last view (rs_host.h; the FASTQ tail behind it), the votes of its records from <file>.votes (uint32
//       pairs, record order): the rows by rr_core.h to <file>.rows, which must be byte for byte what format_rows of rr_host.h gives.
//       One status line per file on stdout:  <status> <count0> <count1> <count2> <records> <bytes> : <file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/rr_core.h"
#include "../../hast_amd/csrc/rr_host.h"
#include "../../hast_amd/csrc/rs_host.h"

using namespace hast;

static uint64_t splitmix64(uint64_t *s) {
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the text of D by the integer rule
static uint32_t density_text(uint32_t v, uint32_t t, char *out) {
    uint8_t row[rr::kMaxTail + 1];
    const uint64_t q = rr::fixed6(rb::density(v, (double)t));
    const uint32_t n = rr::put_tail(row, rb::kHap0, q);
    memcpy(out, row + 12, n - 13);                   // between "\thaplotype0\t" and '\n'
    out[n - 13] = 0;
    return n - 13;
}

struct Tally {
    unsigned long long cases = 0, diffs = 0, ties_down = 0, ties_up = 0;
};

static void check(uint32_t v, uint32_t t, Tally *ta) {
    const double d = (double)v / (double)t;
    char want[64], got[64];
    snprintf(want, sizeof(want), "%0.6f", d);
    density_text(v, t, got);
    const uint64_t q = rr::fixed6(d);
    bool bad = strcmp(want, got) != 0;
    // exactly: d = m 2^-s
    uint64_t bits;
    memcpy(&bits, &d, 8);
    const unsigned s = 1075 - (unsigned)((bits >> 52) & 0x7ff);
    const unsigned __int128 P = (unsigned __int128)((bits & ((1ull << 52) - 1)) | (1ull << 52)) * 1000000u;
    if (s >= 1 && s < 128) {
        const unsigned __int128 one = 1, fl = P >> s, r = P & ((one << s) - 1), h = one << (s - 1);
        const uint64_t exact = (uint64_t)fl + ((r > h || (r == h && (fl & 1))) ? 1 : 0);
        bad |= exact != q;
        if (r == h) ++((fl & 1) ? ta->ties_up : ta->ties_down);
    } else {
        bad = true;
    }
    for (uint32_t cls = 0; cls < 3; ++cls) {
        uint8_t row[rr::kMaxTail + 1];
        const uint32_t n = rr::put_tail(row, cls, cls == rb::kAmbiguous ? 0 : q);
        bad |= n != rr::tail_bytes(cls, q) || n > rr::kMaxTail || rr::row_bytes(7, cls, q) != 7 + (uint64_t)n;
        if (cls != rb::kAmbiguous) bad |= n != 13 + strlen(want);
    }
    ++ta->cases;
    if (bad) {
        if (ta->diffs < 10) fprintf(stderr, "differs: %u / %u: snprintf %s, rr_core %s\n", v, t, want, got);
        ++ta->diffs;
    }
}

static const uint32_t kExtremes[][2] = {{0xffffffffu, 1}, {1, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {1, 1}, {0xfffffffeu, 0xffffffffu}, {1, 0x80000000u},
                                        {0xffffffffu, 2}, {999999, 1000000}, {9999995, 10000000}, {1, 2000000}, {3, 2000000}, {1, 128}, {3, 128}};

template <class F> static void each_case(const char *set, unsigned long long n_rand, uint64_t seed, F f) {
    const bool all = !strcmp(set, "all");
    if (all || !strcmp(set, "grid"))
        for (uint32_t t = 1; t <= 3000; ++t)
            for (uint32_t v = 1; v <= 3000; ++v) f(v, t);
    if (all || !strcmp(set, "ties"))
        for (uint32_t k = 0; k < 32; ++k)
            for (uint32_t v = 1; v <= 200000; ++v) f(v, 1u << k);
    if (all || !strcmp(set, "extremes"))
        for (const auto &e : kExtremes) f(e[0], e[1]);
    if (all || !strcmp(set, "rand"))
        for (unsigned long long i = 0; i < n_rand; ++i) {
            const uint64_t x = splitmix64(&seed);
            const uint32_t v = (uint32_t)x, t = (uint32_t)(x >> 32);
            f(v ? v : 1, t ? t : 1);
        }
}

static bool slurp(const std::string &path, std::vector<uint8_t> *out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out->clear();
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

static bool rows_of_file(int format, uint32_t t0, uint32_t t1, const char *path) {
    std::vector<uint8_t> data, vraw;
    if (!slurp(path, &data) || !slurp(std::string(path) + ".votes", &vraw)) return false;
    std::vector<uint32_t> votes(vraw.size() / 4);
    if (!votes.empty()) memcpy(votes.data(), vraw.data(), votes.size() * 4);
    rs::Framed fr;
    rs::frame(format, data.data(), data.size(), true, false, &fr);
    const char *status = fr.flags & RS_FORMAT_ERROR ? "format_error" : "ok";
    // names back to back, as k_rs_names leaves them
    std::vector<uint8_t> names;
    std::vector<uint32_t> name_off(1, 0);
    for (const rs::Record &r : fr.recs) {
        names.insert(names.end(), data.begin() + r.name_pos, data.begin() + r.name_pos + r.name_len);
        name_off.push_back((uint32_t)names.size());
    }
    if (!strcmp(status, "ok") && format == RS_FASTQ) {
        rs::Tail t;
        if (!rs::fq_tail(data.data() + fr.consumed, data.size() - (size_t)fr.consumed, &t)) status = "format_error";
        else if (t.record) {
            names.insert(names.end(), t.name.begin(), t.name.end());
            name_off.push_back((uint32_t)names.size());
        }
    }
    size_t n = name_off.size() - 1;
    if (strcmp(status, "ok") != 0) n = 0;
    if (2 * n > votes.size()) status = "votes_short", n = 0;
    std::string text, model;
    unsigned long long count[3] = {0, 0, 0};
    uint64_t sized = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t cls;
        uint64_t q;
        rr::row_of(votes[2 * i], votes[2 * i + 1], t0, t1, &cls, &q);
        uint8_t tail[rr::kMaxTail + 1];
        const uint32_t k = rr::put_tail(tail, cls, q);
        text.append(reinterpret_cast<const char *>(names.data()) + name_off[i], name_off[i + 1] - name_off[i]);
        text.append(reinterpret_cast<const char *>(tail), k);
        sized += rr::row_bytes(name_off[i + 1] - name_off[i], cls, q);
        ++count[cls];
    }
    const int totals[2] = {(int)t0, (int)t1};
    names.push_back(0);                              // (never an empty buffer's null pointer)
    format_rows(model, names.data(), name_off.data(), votes.data(), n, totals);
    if (text != model || sized != text.size()) status = "model_differs";
    const std::string out_path = std::string(path) + ".rows";
    FILE *out = fopen(out_path.c_str(), "wb");
    if (!out || fwrite(text.data(), 1, text.size(), out) != text.size() || fclose(out) != 0) return false;
    printf("%s %llu %llu %llu %llu %llu : %s\n", status, count[0], count[1], count[2], (unsigned long long)n, (unsigned long long)text.size(), path);
    return true;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "-s")) {
        Tally ta;
        each_case("all", strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), [&](uint32_t v, uint32_t t) { check(v, t, &ta); });
        printf("cases %llu diffs %llu ties_down %llu ties_up %llu\n", ta.cases, ta.diffs, ta.ties_down, ta.ties_up);
        return ta.diffs ? 1 : 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "-D")) {
        const bool rnd = !strcmp(argv[2], "rand");
        if (rnd && argc != 5) return 2;
        std::string buf;
        each_case(argv[2], rnd ? strtoull(argv[3], nullptr, 10) : 0, rnd ? strtoull(argv[4], nullptr, 10) : 0, [&](uint32_t v, uint32_t t) {
            char text[64];
            const uint32_t n = density_text(v, t, text);
            buf.append(text, n);
            buf += '\n';
            if (buf.size() > (1u << 20)) {
                fwrite(buf.data(), 1, buf.size(), stdout);
                buf.clear();
            }
        });
        fwrite(buf.data(), 1, buf.size(), stdout);
        return fflush(stdout) == 0 ? 0 : 1;
    }
    unsigned t0 = 0, t1 = 0;
    int format = -1, i = 1;
    bool have_t = false;
    for (; i + 1 < argc && argv[i][0] == '-'; i += 2) {
        if (!strcmp(argv[i], "-f")) format = !strcmp(argv[i + 1], "fastq") ? RS_FASTQ : !strcmp(argv[i + 1], "fasta") ? RS_FASTA : -1;
        else if (!strcmp(argv[i], "-t")) have_t = sscanf(argv[i + 1], "%u,%u", &t0, &t1) == 2;
        else break;
    }
    if (format < 0 || !have_t || !t0 || !t1 || i >= argc) {
        fprintf(stderr, "usage: test_rr_core -s N SEED | -D grid|ties|extremes|rand [N SEED] | -f fasta|fastq -t T0,T1 file...\n");
        return 2;
    }
    for (; i < argc; ++i)
        if (!rows_of_file(format, t0, t1, argv[i])) {
            fprintf(stderr, "test_rr_core: cannot read %s and its .votes, or write its .rows\n", argv[i]);
            return 1;
        }
    return 0;
}
