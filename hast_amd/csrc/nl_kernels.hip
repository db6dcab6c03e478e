// nl_kernels.hip -- gfx950 device code: the newline index (nl_index.h) of ranges the host knows, for rs_, sq_, sq_fasta_ (one range a
// launch) and tx_kernels.hip (two); blockIdx.y = the side:
//   k_nl_count   newlines per 4-KB tile
//   k_nl_index   offsets of all newlines from the side's first byte, in order, once the family's scan has run
#include "nl_index.h"

namespace hast {

__global__ void __launch_bounds__(256) k_nl_count(NlSides in) {
    const NlRange &r = in.r[blockIdx.y];
    const uint32_t c = nl_tile_count(r.base16, blockIdx.x, r.lo, r.hi);
    if (threadIdx.x == 0) in.tile_cnt[blockIdx.y][blockIdx.x] = c;
}
__global__ void __launch_bounds__(256) k_nl_index(NlSides in) {
    const NlRange &r = in.r[blockIdx.y];
    nl_tile_index(r.base16, blockIdx.x, r.lo, r.hi, r.lo, in.tile_cnt[blockIdx.y], in.nl[blockIdx.y]);
}

void launch_nl_count(const NlSides &in, uint32_t sides, uint32_t grid, hipStream_t s) { hipLaunchKernelGGL(k_nl_count, dim3(grid, sides), dim3(256), 0, s, in); }
void launch_nl_index(const NlSides &in, uint32_t sides, uint32_t grid, hipStream_t s) { hipLaunchKernelGGL(k_nl_index, dim3(grid, sides), dim3(256), 0, s, in); }

}  // namespace hast
