// Count sweep of the fp16 tier, the parity-split builds of 80 .. 128 slices (d = 1025 .. 2048, kz_knn_cntx16.h): one workgroup per CU,
// two workgroups per work item.
#include "kz_common.h"
#include "kz_knn_cntx16.h"

KzCountKernel kz_count_lookup_x(int n_slices) {
    return kz_cntx_table<false>(n_slices, std::integer_sequence<int, 80, 96, 112, 128>{});
}
