// parity-split builds (65 .. 128 slices, d = 1025 .. 2048) of the fp16 fused kernel, list length 128 (kz_knn_hx_inst.h)
#define KZ_H_KP 128
#include "kz_knn_hx_inst.h"
