// radix_sort_limit.cpp -- prints the size up to which the installed library's radix sort, with the default configuration that
// rows::sort_pass (rows_sort.hip) takes, sorts by its merge sort; past it the sort is Onesweep.  tests/test_rows_caps_cpu.py holds
// tests/rows_corpus.py's SORT_MERGE_LIMIT to it.  Host code only: nothing here touches a GPU.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort_config.hpp>

#include <cstdio>

int main() {
    printf("%zu\n", (size_t)rocprim::radix_sort_config<>::merge_sort_limit);
    return 0;
}
