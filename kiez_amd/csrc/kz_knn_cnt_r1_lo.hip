// Rank-one count sweep of the fp16 tier (kz_knn_cnt_r1_16.h), builds of 2 .. 13 slices: three workgroups per CU.
#include "kz_common.h"
#include "kz_knn_cnt_r1_16.h"

KzCountKernel kz_count_r1_lookup_lo(int n_slices) {
    return kz_count_r1_table<3>(n_slices, std::integer_sequence<int, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13>{});
}
