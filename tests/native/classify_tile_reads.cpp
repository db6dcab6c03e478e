// classify_tile_reads.cpp -- prints the reads a workgroup's tile holds (hast_amd/csrc/classify_plan.h) for one row shape, so that
// tests/test_classify_tile_gpu.py can size its batches to three full tiles and a partial one without restating the plan.
//   classify_tile_reads <k> <m> <read_len> <strict> <use_filter> <filter t> <filter dense> <tile_lds>   ->  "<tile_reads> <smem> <fits>"
#include <stdio.h>
#include <stdlib.h>

#include "../../hast_amd/csrc/classify_plan.h"

int main(int argc, char **argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: classify_tile_reads k m read_len strict use_filter t dense tile_lds\n");
        return 2;
    }
    hast::FilterGeom fg{};
    fg.t = atoi(argv[6]);
    fg.dense = atoi(argv[7]);
    const hast::classify::Plan p = hast::classify::plan_for(atoi(argv[1]), atoi(argv[2]), (uint32_t)strtoul(argv[3], nullptr, 10), atoi(argv[4]) != 0,
                                                            atoi(argv[5]) != 0, fg, (size_t)strtoull(argv[8], nullptr, 10), 256, 1);
    printf("%u %zu %d\n", p.tile_reads, p.smem, p.fits ? 1 : 0);
    return 0;
}
