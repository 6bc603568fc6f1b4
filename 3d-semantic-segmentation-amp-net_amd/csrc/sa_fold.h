// sa_fold.h -- the BatchNorm fold shared by the fused PointNet++ forwards (set_abstraction.hip defines it, feature_propagation.hip uses it).
#pragma once
#include "common.h"

namespace ampnet {

constexpr int SA_MAX_LAYERS = AMPNET_SA_MAX_LAYERS;

struct SaFold {
    int L, cout[SA_MAX_LAYERS], off[SA_MAX_LAYERS];
    const float *bias[SA_MAX_LAYERS], *gamma[SA_MAX_LAYERS], *beta[SA_MAX_LAYERS], *mean[SA_MAX_LAYERS], *var[SA_MAX_LAYERS];
    float eps[SA_MAX_LAYERS];
};

// launches sa_fold_kernel on `st`: fold[off_l .. off_l + cout_l) = scale_l = gamma / sqrt(var + eps), the next cout_l floats
// shift_l = (b - mean) * scale + beta
int sa_fold_launch(const SaFold &f, float *fold, hipStream_t st);

}  // namespace ampnet
