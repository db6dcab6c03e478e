// The reader of hast_amd/csrc/switches.h, kind by kind, on the real table: flags, integers, counts, numbers and words set with
// setenv / unsetenv, both out-of-range policies, the "ignored" line once per variable, and the rows themselves.  Stand-alone (its own
// main; tests/test_switches_cpu.py builds it plain and under ASan + UBSan).  The "ignored" lines go to stderr, which the program
// points at a file to count them.
#include <unistd.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../../hast_amd/csrc/switches.h"

namespace sw = hast::sw;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            ++g_failed;                                                        \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
        }                                                                      \
    } while (0)

static void set(sw::Id id, const char *v) {
    if (v) setenv(sw::kRows[id].name, v, 1);
    else unsetenv(sw::kRows[id].name);
}
// the first row of the table with this kind (and, for numbers, this policy; bounded: with an upper bound)
static sw::Id first(sw::Kind kind, int policy = -1, bool bounded = false) {
    for (int i = 0; i < sw::kCount; ++i) {
        const sw::Row &r = sw::kRows[i];
        if (r.kind == kind && (policy < 0 || r.policy == policy) && (!bounded || r.hi < sw::NOLIM)) return (sw::Id)i;
    }
    printf("FAILED: the table has no row of kind %d, policy %d\n", (int)kind, policy);
    exit(1);
}
static std::string num(double v) {
    char b[64];
    snprintf(b, sizeof(b), "%.0f", v);
    return b;
}
// lines of the stderr file that name this variable
static int ignored_lines(const char *path, sw::Id id) {
    fflush(stderr);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int n = 0;
    char line[1024];
    const std::string want = std::string("hast: ") + sw::kRows[id].name + "=";
    while (fgets(line, sizeof(line), f))
        if (!strncmp(line, want.c_str(), want.size()) && strstr(line, "; ignored\n")) ++n;
    fclose(f);
    return n;
}

static void flags() {
    const sw::Id f = first(sw::Flag), d = first(sw::FlagDefaultOn);
    const struct { const char *v; bool flag, default_on; } cases[] = {{nullptr, false, true}, {"", false, true}, {"0", false, false}, {"1", true, true},
                                                                      {"yes", true, true}, {"00", true, true}, {"0 ", true, true}};
    for (const auto &c : cases) {
        set(f, c.v);
        set(d, c.v);
        CHECK(sw::flag(f) == c.flag);
        CHECK(sw::flag(d) == c.default_on);
    }
    set(f, nullptr);
    set(d, nullptr);
}

// an Int row and a Size row under each policy: lo - 1, lo, hi, hi + 1
template <class Read>
static void bounds(sw::Id id, Read read) {
    const sw::Row &r = sw::kRows[id];
    const long long lo = (long long)r.lo, hi = (long long)r.hi;
    long long v = -7;
    set(id, num(r.lo).c_str());
    CHECK(read(id, &v) && v == lo);
    set(id, num(r.hi).c_str());
    CHECK(read(id, &v) && v == hi);
    v = -7;
    set(id, num(r.hi + 1).c_str());
    if (r.policy == sw::Clamp) CHECK(read(id, &v) && v == hi);
    else CHECK(!read(id, &v) && v == -7);
    v = -7;
    if (r.kind == sw::Int || lo > 0) {                      // (a count below 0 is no count at all)
        set(id, num(r.lo - 1).c_str());
        if (r.policy == sw::Clamp) CHECK(read(id, &v) && v == lo);
        else CHECK(!read(id, &v) && v == -7);
    }
    set(id, nullptr);
}

static void numbers() {
    auto rd_int = [](sw::Id id, long long *v) { return sw::integer(id, v); };
    auto rd_size = [](sw::Id id, long long *v) { return sw::size(id, v); };
    // an integer row that takes 12 and -1 (HAST_PARK_SITES: -1 is its default), and a count without an upper bound
    const sw::Id i = sw::HAST_PARK_SITES, s = sw::HAST_GZ_RING_BYTES;
    CHECK(sw::kRows[i].kind == sw::Int && sw::kRows[i].lo == -1 && sw::kRows[s].kind == sw::Size && sw::kRows[s].lo == 0 && sw::kRows[s].hi == sw::NOLIM);
    long long v = -7;
    uint64_t u = 7;
    set(i, nullptr);
    set(s, nullptr);
    CHECK(!sw::integer(i, &v) && v == -7 && !sw::size(s, &u) && u == 7);
    set(i, "12");
    set(s, "12");
    CHECK(sw::integer(i, &v) && v == 12 && sw::size(s, &u) && u == 12);
    set(i, "-1");
    set(s, "-1");
    CHECK(sw::integer(i, &v) && v == -1);
    u = 7;
    CHECK(!sw::size(s, &u) && u == 7);
    for (const char *bad : {"12abc", " 12", "", "1e3", "0x10", "99999999999999999999999999", "12 "}) {
        set(i, bad);
        set(s, bad);
        v = -7;
        u = 7;
        CHECK(!sw::integer(i, &v) && v == -7);
        CHECK(!sw::size(s, &u) && u == 7);
    }
    set(i, "12K");                                               // (a suffix is the grammar of a count alone)
    CHECK(!sw::integer(i, &v));
    const struct { const char *t; bool ok; uint64_t v; } sizes[] = {{"16M", true, 16ull << 20}, {"16m", true, 16ull << 20}, {"2G", true, 2ull << 30}, {"3k", true, 3072},
                                                                    {"1Q", false, 0}, {"16MM", false, 0}, {"1.5G", false, 0}, {"+5", false, 0},
                                                                    {"18446744073709551615", true, ~0ull}, {"18446744073709551616", false, 0},
                                                                    {"17179869184G", false, 0}, {"17179869183G", true, 17179869183ull << 30}};
    for (const auto &c : sizes) {
        set(s, c.t);
        u = 7;
        CHECK(sw::size(s, &u) == c.ok && u == (c.ok ? c.v : 7));
        uint64_t p = 7;
        CHECK(hast::parse_count(c.t, &p) == c.ok && p == (c.ok ? c.v : 7));    // (the flags' parser is the same function)
    }
    set(i, nullptr);
    set(s, nullptr);
    bounds(first(sw::Int, sw::Clamp, true), rd_int);
    bounds(first(sw::Int, sw::Ignore, true), rd_int);
    bounds(first(sw::Size, sw::Clamp, true), rd_size);
    bounds(first(sw::Size, sw::Ignore, true), rd_size);
    // the rows the dispatch tests read: out of range is ignored, not clamped
    CHECK(sw::kRows[sw::HAST_KC_TILE].policy == sw::Ignore && sw::kRows[sw::HAST_MINIMIZER].policy == sw::Ignore && sw::kRows[sw::HAST_MINIMIZER].lo == 1);

    const sw::Id rc = first(sw::Real, sw::Clamp, true);
    double x = -7;
    set(rc, nullptr);
    CHECK(!sw::real(rc, &x) && x == -7);
    set(rc, "0.5");
    CHECK(sw::real(rc, &x) && x == 0.5);
    set(rc, "1e-1");
    CHECK(sw::real(rc, &x) && x == 0.1);
    for (const char *bad : {"0.5x", " 0.5", "", "nan", "inf", "1e999", "half"}) {
        set(rc, bad);
        x = -7;
        CHECK(!sw::real(rc, &x) && x == -7);
    }
    set(rc, "1e9");
    CHECK(sw::real(rc, &x) && x == sw::kRows[rc].hi);
    set(rc, "-3");
    CHECK(sw::real(rc, &x) && x == sw::kRows[rc].lo);
    set(rc, nullptr);
}

static void words() {
    const sw::Id w = sw::HAST_INFLATE;
    CHECK(sw::kRows[w].kind == sw::Word && !strcmp(sw::kRows[w].words, "device|host|zlib"));
    set(w, nullptr);
    CHECK(sw::word(w) == -1 && !sw::word_is(w, "zlib"));
    set(w, "device");
    CHECK(sw::word(w) == 0 && sw::word_is(w, "device") && !sw::word_is(w, "zlib"));
    set(w, "zlib");
    CHECK(sw::word(w) == 2 && sw::word_is(w, "zlib"));
    for (const char *bad : {"sideways", "", "zli", "zlibs", "host|zlib", "Host", "|"}) {
        set(w, bad);
        CHECK(sw::word(w) == -1 && !sw::word_is(w, "host"));
    }
    set(w, "zlibs");
    CHECK(!strcmp(sw::text(w), "zlibs"));                        // (the text as it stands, for the programs that validate it themselves)
    set(w, nullptr);
    CHECK(sw::text(w) == nullptr);
}

// the same bad text read twice: one line; another variable: its own line; a good value: none
static void ignored_once(const char *err_path) {
    const sw::Id a = sw::HAST_GZ_AHEAD, b = sw::HAST_KC_FLUSH, c = sw::HAST_GZ_THREADS;
    CHECK(ignored_lines(err_path, a) == 0 && ignored_lines(err_path, b) == 0 && ignored_lines(err_path, c) == 0);
    int v = 0;
    set(a, "2x");
    CHECK(!sw::integer(a, &v) && !sw::integer(a, &v));
    CHECK(ignored_lines(err_path, a) == 1);
    set(a, "3y");                                                // (once per variable, not per text)
    CHECK(!sw::integer(a, &v));
    CHECK(ignored_lines(err_path, a) == 1);
    set(b, "sideways");
    CHECK(sw::word(b) == -1 && sw::word(b) == -1 && !sw::word_is(b, "sweep"));
    CHECK(ignored_lines(err_path, b) == 1);
    set(c, "4");
    CHECK(sw::integer(c, &v) && v == 4);
    set(c, "100000");                                            // (clamped: taken, nothing to say)
    CHECK(sw::integer(c, &v) && v == (int)sw::kRows[c].hi);
    CHECK(ignored_lines(err_path, c) == 0);
    fflush(stderr);
    FILE *f = fopen(err_path, "r");
    char line[1024] = "";
    CHECK(f && fgets(line, sizeof(line), f) && !strcmp(line, "hast: HAST_GZ_AHEAD=2x is not an integer in [0, 2]; ignored\n"));
    if (f) fclose(f);
    set(a, nullptr);
    set(b, nullptr);
    set(c, nullptr);
}

static void table() {
    std::set<std::string> names;
    for (int i = 0; i < sw::kCount; ++i) {
        const sw::Row &r = sw::kRows[i];
        CHECK(r.name && !strncmp(r.name, "HAST_", 5) && names.insert(r.name).second);
        CHECK(r.desc && *r.desc && r.reader && *r.reader && r.dflt && *r.dflt);
        CHECK(r.lo <= r.hi);
        CHECK((r.kind == sw::Word) == (r.words && *r.words));
        if (r.kind == sw::Word) CHECK(r.words[0] != '|' && r.words[strlen(r.words) - 1] != '|' && !strstr(r.words, "||"));
        if (r.kind == sw::Int || r.kind == sw::Size || r.kind == sw::Real) CHECK(r.policy == sw::Clamp || r.policy == sw::Ignore);
        if (r.kind == sw::Size) CHECK(r.lo >= 0);
    }
    CHECK((int)names.size() == sw::kCount && sw::kCount > 40);
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: test_switches STDERR_FILE\n"), 2;
    // whatever the caller's environment holds of the table is not this test's
    for (int i = 0; i < sw::kCount; ++i) unsetenv(sw::kRows[i].name);
    const int saved = dup(2);
    if (saved < 0 || !freopen(argv[1], "w", stderr)) return printf("cannot write %s\n", argv[1]), 2;
    ignored_once(argv[1]);                                       // (first: the lines of the other tests are not counted)
    flags();
    numbers();
    words();
    table();
    fflush(stderr);
    dup2(saved, 2);
    close(saved);
    printf("checks %d failed %d rows %d\n", g_checks, g_failed, (int)sw::kCount);
    return g_failed ? 1 : 0;
}
