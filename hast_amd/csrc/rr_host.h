// rr_host.h -- the host model of stage 03's rows: what `classify_read` prints with --rows host, what every fallback of --rows device
// prints, and what the integer rule of rr_core.h is checked against (tests/native/test_rr_core.cpp): the density goes through snprintf.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstdio>
#include <string>

#include "rb_core.h"

namespace hast {

// the rows of n reads: names[name_off[i], name_off[i + 1]) and votes[2 i], votes[2 i + 1] -> "name \t haplotypeN|ambiguous \t density"
inline void format_rows(std::string &out, const uint8_t *names, const uint32_t *name_off, const uint32_t *votes, size_t n, const int *total_kmers) {
    char row[96];
    for (size_t i = 0; i < n; i++) {
        const double d0 = hast::rb::density(votes[2 * i], total_kmers[0]), d1 = hast::rb::density(votes[2 * i + 1], total_kmers[1]);   // s03:215-216
        // s03:110-133 for two haplotypes: both zero -> ambiguous 0.0; else the larger density, ties to haplotype0 (rb_core.h: the bins' rule)
        const uint32_t cls = hast::rb::class_of(d0, d1);
        if (cls == hast::rb::kAmbiguous) snprintf(row, sizeof(row), "\tambiguous\t0.0\n");
        else if (cls == hast::rb::kHap1) snprintf(row, sizeof(row), "\thaplotype1\t%0.6f\n", d1);
        else snprintf(row, sizeof(row), "\thaplotype0\t%0.6f\n", d0);
        out.append(reinterpret_cast<const char *>(names) + name_off[i], name_off[i + 1] - name_off[i]);
        out += row;
    }
}

}  // namespace hast
