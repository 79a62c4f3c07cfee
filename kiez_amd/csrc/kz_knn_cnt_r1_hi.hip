// Rank-one count sweep of the fp16 tier (kz_knn_cnt_r1_16.h), builds of 14 .. 24 slices: two workgroups per CU.
#include "kz_common.h"
#include "kz_knn_cnt_r1_16.h"

KzCountKernel kz_count_r1_lookup_hi(int n_slices) {
    return kz_count_r1_table<2>(n_slices, std::integer_sequence<int, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24>{});
}
