// kc_geometry.cpp -- prints the record geometry of stage 00's counter (hast_amd/csrc/kc_common.h) for one (k, m), so that
// tests/test_kc_geometry_gpu.py and tests/test_kc_dispatch_cpu.py can say which counters take the partitioned path and where a
// minimizer run is cut without restating kc_rec_off_bits and kc_run_max.
//   kc_geometry <k> <m> [<k> <m> ...]   ->  one line "<k> <m> <W> <kc_rec_off_bits> <kc_run_max>" per pair
#include <stdio.h>
#include <stdlib.h>

#include "../../hast_amd/csrc/kc_common.h"

int main(int argc, char **argv) {
    if (argc < 3 || argc % 2 != 1) {
        fprintf(stderr, "usage: kc_geometry k m [k m ...]\n");
        return 2;
    }
    for (int i = 1; i + 1 < argc; i += 2) {
        const int k = atoi(argv[i]), m = atoi(argv[i + 1]);
        if (k < 1 || k > 32 || m < 1 || m > k) {
            fprintf(stderr, "kc_geometry: (%d, %d) is no (k, m) with 1 <= m <= k <= 32\n", k, m);
            return 2;
        }
        printf("%d %d %d %u %u\n", k, m, k - m + 1, hast::kc_rec_off_bits(k, m), hast::kc_run_max(k, m));
    }
    return 0;
}
