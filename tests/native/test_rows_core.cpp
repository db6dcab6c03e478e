// test_rows_core.cpp -- the host model of the output table (hast_amd/csrc/rows_host.h over rows_core.h) as a stand-alone program, for
// tests/test_rows_core_cpu.py: it is built once plain and once under ASan + UBSan.
//
//   test_rows_core FILE...      every FILE is a case: u64 n, n0, n1; f64 w0, w1; n text records of 16 bytes; n x 4 u64 counters.
//                               Writes FILE.table, FILE.list1 .. FILE.list3, FILE.cls (a byte per id), FILE.order (u32 per row),
//                               FILE.keys ("hi lo" in hex per id) and FILE.haps (row_hap per id, a line each); prints
//                               "FILE any_sep past_int" per case.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../hast_amd/csrc/rows_host.h"

using namespace hast;

static bool read_file(const char *path, std::vector<uint8_t> *out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}
static bool write_file(const std::string &path, const void *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        std::vector<uint8_t> in;
        if (!read_file(argv[a], &in) || in.size() < 40) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        uint64_t head[3];
        double w[2];
        memcpy(head, in.data(), 24);
        memcpy(w, in.data() + 24, 16);
        const size_t n = (size_t)head[0];
        if (in.size() != 40 + n * 48) {
            fprintf(stderr, "%s: %zu bytes for %zu rows\n", argv[a], in.size(), n);
            return 2;
        }
        std::vector<uint8_t> text(in.begin() + 40, in.begin() + 40 + (long)(16 * n));
        std::vector<uint64_t> counts(4 * n);
        if (n) memcpy(counts.data(), in.data() + 40 + 16 * n, 32 * n);
        rows::Tables t;
        rows::build(text.data(), counts.data(), n, head[1], head[2], w[0], w[1], &t);
        std::string keys, haps;
        for (size_t i = 0; i < n; ++i) {
            char line[64];
            const rows::Key k = rows::row_key(text.data() + 16 * i);
            snprintf(line, sizeof line, "%016llx %016llx\n", (unsigned long long)k.hi, (unsigned long long)k.lo);
            keys += line;
            snprintf(line, sizeof line, "%d\n", rows::row_hap(text.data() + 16 * i, counts[4 * i], counts[4 * i + 1], head[1], head[2], w[0], w[1]));
            haps += line;
        }
        const std::string base = argv[a];
        bool ok = write_file(base + ".table", t.table.data(), t.table.size());
        for (int l = 0; l < 3; ++l) ok = ok && write_file(base + ".list" + std::to_string(l + 1), t.list[l].data(), t.list[l].size());
        ok = ok && write_file(base + ".cls", t.cls.data(), t.cls.size()) && write_file(base + ".order", t.order.data(), 4 * t.order.size());
        ok = ok && write_file(base + ".keys", keys.data(), keys.size()) && write_file(base + ".haps", haps.data(), haps.size());
        if (!ok) {
            fprintf(stderr, "cannot write the results of %s\n", argv[a]);
            return 2;
        }
        printf("%s %d %d\n", argv[a], t.any_sep ? 1 : 0, t.past_int ? 1 : 0);
    }
    return 0;
}
