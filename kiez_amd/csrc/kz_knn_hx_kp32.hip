// parity-split builds (65 .. 128 slices, d = 1025 .. 2048) of the fp16 fused kernel, list length 32 (kz_knn_hx_inst.h)
#define KZ_H_KP 32
#include "kz_knn_hx_inst.h"
