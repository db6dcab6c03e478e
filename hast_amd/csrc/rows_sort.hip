// rows_sort.hip -- one stable pass of the output table's LSD sort: 64-bit keys with the barcode ids as payload, by the library's radix
// sort.  A translation unit of its own: the library's kernels use scratch memory, which no kernel of rows_kernels.hip may (Makefile).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "rows_device.h"

namespace hast {
namespace rows {

hipError_t sort_pass(void *d_tmp, size_t *tmp_bytes, const uint64_t *d_keys_in, uint64_t *d_keys_out, const uint32_t *d_ids_in, uint32_t *d_ids_out, size_t n,
                     hipStream_t s) {
    return rocprim::radix_sort_pairs(d_tmp, *tmp_bytes, d_keys_in, d_keys_out, d_ids_in, d_ids_out, n, 0u, 64u, s);
}

}  // namespace rows
}  // namespace hast
