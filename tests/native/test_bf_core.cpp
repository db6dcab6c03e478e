// test_bf_core.cpp -- bf_core.h's field rule and bf_host.h's streaming model, stand-alone (built by tests/test_bf_core_cpu.py, also
// under ASan + UBSan).  Prints "ok <checks>" and returns 0, or says what differs and returns 1.
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/bf_host.h"

using namespace hast;

static long checks = 0;
static int fail(const char *what, const std::string &on) {
    fprintf(stderr, "FAIL %s on \"", what);
    for (unsigned char c : on) fprintf(stderr, c >= 32 && c < 127 ? "%c" : "\\x%02x", c);
    fprintf(stderr, "\"\n");
    return 1;
}

// the rule, naively: cut the line into fields at every separator, take the second
static bool naive_field2(const std::string &line, std::string &key) {
    std::vector<std::string> f(1);
    for (char c : line) {
        if (c == '#' || c == '/') f.emplace_back();
        else f.back().push_back(c);
    }
    if (f.size() < 2) return false;
    key = f[1];
    return true;
}

static bool same(const bf::Model &a, const bf::Model &b) {
    return a.counts == b.counts && a.header_lines == b.header_lines && a.counted == b.counted && a.no_field == b.no_field;
}

int main() {
    std::mt19937 rng(11);
    const char alphabet[] = {'a', 'b', '#', '/', '_', '1', '\t', '\r'};
    // (1) the field rule and the text record on random headers
    for (int it = 0; it < 20000; ++it) {
        std::string h;
        const int n = (int)(rng() % 24);
        for (int i = 0; i < n; ++i) h.push_back(alphabet[rng() % sizeof alphabet]);
        // (an exact-size heap copy: a read past the line is the sanitizer's to catch)
        std::vector<uint8_t> line(h.begin(), h.end());
        std::string want;
        const bool has = naive_field2(h, want);
        uint64_t start = 0, len = 0;
        const bool got = bf::field2(line.data(), line.size(), start, len);
        ++checks;
        if (got != has) return fail("has a field 2", h);
        if (!has) continue;
        if (start + len > line.size() || std::string(h, (size_t)start, (size_t)len) != want) return fail("field 2", h);
        if (len <= bf::kMaxText) {
            uint32_t w[4];
            bf::text_record(line.data() + start, (uint32_t)len, w);
            uint8_t rec[16];
            memcpy(rec, w, 16);                                       // (little-endian words: byte 0 the length, then the text)
            uint8_t expect[16] = {0};
            expect[0] = (uint8_t)len;
            memcpy(expect + 1, want.data(), want.size());
            if (memcmp(rec, expect, 16) != 0) return fail("text record", h);
        }
    }
    {
        uint32_t a[4], b[4];
        bf::long_record(a);
        bf::nofield_record(b);
        if ((a[0] & 0xFF) != 0xFF || (b[0] & 0xFF) != 0xFF || !memcmp(a, b, 16)) return fail("marks", "");
    }
    // (2) streams of random lines, with every kind of end, fed in pieces of 1 .. 64 bytes equal the stream fed whole
    for (int it = 0; it < 400; ++it) {
        std::string s;
        const int lines = (int)(rng() % 40);
        for (int l = 0; l < lines; ++l) {
            const int n = (int)(rng() % 30);
            for (int i = 0; i < n; ++i) s.push_back(alphabet[rng() % sizeof alphabet]);
            s.push_back('\n');
        }
        if (rng() % 2)                                                // an unterminated last line
            for (int i = (int)(rng() % 20); i >= 0; --i) s.push_back(alphabet[rng() % sizeof alphabet]);
        std::vector<uint8_t> bytes(s.begin(), s.end());
        bf::Model whole, pieces, by_line;
        whole.whole(bytes.data(), bytes.size());
        pieces.begin();
        for (size_t at = 0; at < bytes.size();) {
            const size_t n = std::min<size_t>(1 + rng() % 64, bytes.size() - at);
            std::vector<uint8_t> piece(bytes.begin() + (long)at, bytes.begin() + (long)(at + n));
            pieces.feed(piece.data(), piece.size());
            at += n;
        }
        pieces.finish();
        // ... and the rule applied line by line
        size_t ln = 0;
        for (size_t at = 0; at < s.size(); ++ln) {
            size_t e = s.find('\n', at);
            if (e == std::string::npos) e = s.size();
            if (ln % 4 == 0) {
                std::string key;
                ++by_line.header_lines;
                if (naive_field2(s.substr(at, e - at), key)) { ++by_line.counted; by_line.counts[key]++; }
                else ++by_line.no_field;
            }
            at = e + 1;
        }
        ++checks;
        if (!same(whole, pieces)) return fail("pieces against whole", s);
        if (!same(whole, by_line)) return fail("whole against line by line", s);
        if (whole.counted + whole.no_field != whole.header_lines) return fail("the counts add up", s);
    }
    // (3) rows: merged by key, byte-wise order, plain 64-bit decimal
    {
        bf::Rows rows = {{"b", 1}, {std::string("a\0b", 3), 2}, {"a", 3}, {"b", 1ull << 33}, {"", 7}, {"\xff", 1}, {"a\t", 1}};
        bf::merge_rows(rows);
        std::string out;
        bf::print_rows(rows, out);
        static const char expect[] = "\t7\na\t3\na\0b\t2\na\t\t1\nb\t8589934593\n\xff\t1\n";
        const std::string want(expect, sizeof expect - 1);
        ++checks;
        if (out != want) return fail("rows", out);
    }
    printf("ok %ld\n", checks);
    return 0;
}
