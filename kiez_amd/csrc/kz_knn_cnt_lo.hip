// Count sweep of the fp16 tier (kz_knn_cnt16.h), builds of 2 .. 13 slices: three workgroups per CU.
#include "kz_common.h"
#include "kz_knn_cnt16.h"

KzCountKernel kz_count_lookup_lo(int n_slices) {
    return kz_count_table<3>(n_slices, std::integer_sequence<int, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13>{});
}
