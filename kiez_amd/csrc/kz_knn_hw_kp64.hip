// wide-row builds (32 .. 64 slices) of the fp16 fused kernel, list length 64 (kz_knn_h_inst.h)
#define KZ_H_KP 64
#define KZ_H_WIDE_ROWS 1
#include "kz_knn_h_inst.h"
