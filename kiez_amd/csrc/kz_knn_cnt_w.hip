// Count sweep of the fp16 tier (kz_knn_cnt16.h), the wide-row builds of 32 .. 64 slices (d = 497 .. 1024): one workgroup per CU.
#include "kz_common.h"
#include "kz_knn_cnt16.h"

KzCountKernel kz_count_lookup_w(int n_slices) {
    return kz_count_table<1>(n_slices, std::integer_sequence<int, 32, 40, 48, 56, 64>{});
}
