// test_dz_members.cpp -- dz::member_layout (hast_amd/csrc/dz_core.h), the check hast_fq_next_routed and hast_rs_next_binned make of an
// encoder's Result before they copy its members: back to back from 0 on, inside cap, empty runs skipped.  Built with ASan + UBSan by
// tests/test_dz_core_cpu.py.  Prints "ok cases=N".
#include <stdio.h>
#include <stdlib.h>

#include "../../hast_amd/csrc/dz_core.h"

using namespace hast::dz;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

// the members of sizes[0 .. n) as the encoder lays them out: back to back, an empty run's offset left at a value nobody may read
static Result laid_out(const uint64_t *sizes, int n) {
    Result r{};
    uint64_t at = 0;
    for (int c = 0; c < kMaxRuns; ++c) {
        r.out_bytes[c] = c < n ? sizes[c] : 0;
        r.member_off[c] = r.out_bytes[c] ? at : ~0ull;
        at += r.out_bytes[c];
    }
    return r;
}

int main() {
    size_t cases = 0;
    const uint64_t some[3] = {0, 20, 4097};
    for (int n = 1; n <= kMaxRuns; ++n) {
        int pick[kMaxRuns] = {0, 0, 0, 0};
        for (int code = 0; code < 81; ++code) {       // every run empty, small or large: empty runs in every position
            bool skip = false;
            for (int c = 0, x = code; c < kMaxRuns; ++c, x /= 3) {
                pick[c] = x % 3;
                if (c >= n && pick[c]) skip = true;
            }
            if (skip) continue;
            uint64_t sizes[kMaxRuns], sum = 0, want_off[kMaxRuns];
            for (int c = 0; c < n; ++c) {
                want_off[c] = sum;
                sum += sizes[c] = some[pick[c]];
            }
            const Result r = laid_out(sizes, n);
            uint64_t off[kMaxRuns], total = ~0ull;
            // the last member ends exactly at cap
            CHECK(member_layout(r, n, sum, off, &total) == kLayoutOk && total == sum);
            for (int c = 0; c < n; ++c) CHECK(off[c] == want_off[c]);
            CHECK(member_layout(r, n, sum + 1000, off, &total) == kLayoutOk && total == sum);
            ++cases;
            if (!sum) continue;
            // ... and one byte past it
            CHECK(member_layout(r, n, sum - 1, off, &total) == kLayoutPastCap);
            CHECK(member_layout(r, n, 0, off, &total) == kLayoutPastCap);
            for (int c = 0; c < n; ++c) {
                if (!sizes[c]) continue;
                Result bad = r;
                ++bad.member_off[c];                  // a gap in front of member c
                CHECK(member_layout(bad, n, sum + 1000, off, &total) == kLayoutGap);
                if (r.member_off[c]) {
                    bad.member_off[c] = r.member_off[c] - 1;      // it overlaps the member before
                    CHECK(member_layout(bad, n, sum + 1000, off, &total) == kLayoutGap);
                }
                bad = r;
                bad.out_bytes[c] = ~0ull - 3;         // a size that wraps: past cap, not a wrapped sum
                CHECK(member_layout(bad, n, sum + 1000, off, &total) != kLayoutOk);
                ++cases;
            }
            // runs behind n_runs are not looked at
            if (n < kMaxRuns) {
                Result more = r;
                more.out_bytes[n] = 5;
                more.member_off[n] = 12345;
                CHECK(member_layout(more, n, sum, off, &total) == kLayoutOk && total == sum);
                CHECK(member_layout(more, n + 1, sum + 1000, off, &total) == kLayoutGap);
            }
        }
    }
    printf("ok cases=%zu\n", cases);
    return 0;
}
