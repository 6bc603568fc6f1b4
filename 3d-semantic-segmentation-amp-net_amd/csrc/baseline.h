// baseline.h -- launch wrappers of the baseline single-window PointNet's kernels (baseline.hip: eval forward; baseline_train.hip: train
// forward and backward).  Each wrapper owns its kernel's grid and block; the product entry points call them, and so does the baseline test
// hook of layer_probe.hip, which therefore launches exactly what the product launches.  The wrappers only enqueue: the caller asks
// check_launch() when its sequence is complete, as the entry points always did.
#pragma once
#include "kernels.h"

namespace ampnet {

// ---- eval forward (baseline.hip) ------------------------------------------------------------------------------------------------------
struct BlLayer {               // six device pointers per layer, any of b / BatchNorm may be null
    const float *W, *b, *g, *be, *rm, *rv;
};
// scale / shift [C] of "conv bias, then eval BatchNorm": y = (z + b - rm) * g / sqrt(rv + eps) + be
void bl_fold(const BlLayer &l, int C, float eps, float *scale, float *shift, hipStream_t st);
// in place on z [n / C, C]: z = act((z + add[row / per]) * scale + shift)
void bl_affine(float *z, size_t n, int C, const float *scale, const float *shift, const float *add, int per, int relu, hipStream_t st);
void bl_rowmax(const float *a, int B, int N, int C, float *out, hipStream_t st);                  // [B, N, C] -> [B, C]
void bl_mix(const float *x, const float *T, int R, int N, int k, float *out, hipStream_t st);     // cat([x[:, :, :k] @ T, x[:, :, k:]], 2)
void bl_logits(const float *z, int B, int N, int C, float *logits, hipStream_t st);               // z [B * N, C] -> logits [B, C, N]

// ---- train forward and backward (baseline_train.hip) ----------------------------------------------------------------------------------
struct TLayer {                // device pointers of one layer: weight, bias, BatchNorm weight / bias / running mean / running var
    const float *W, *b, *g, *be;
    float *rm, *rv;
};
struct TGrad {                 // gradients of the same (nullptr where the layer has no such parameter)
    float *dW, *db, *dg, *dbe;
};
struct Rec {                   // one linear (+ BatchNorm + ReLU) layer on the tape
    float *z, *a;              // [M, cout] pre-BatchNorm (with bias / addend) and activation; a == z for layers without BatchNorm
    float *mean, *invstd;      // [cout]
    int M, K, cout;
};

void bt_bias(float *z, size_t n, int C, const float *bias, const float *add, int per, hipStream_t st);   // z[row][c] += bias[c] + add[row / per][c]
void bt_stats(const float *z, int M, int C, float eps, float momentum, float *mean, float *invstd, float *rm, float *rv, hipStream_t st);
void bt_running_stats(const float *rm, const float *rv, int C, float eps, float *mean, float *invstd, hipStream_t st);
void bt_bn_act(const float *z, size_t n, int C, const float *mean, const float *invstd, const float *g, const float *be, float *a, hipStream_t st);
void bt_bn_bwd_sums(const float *da, const float *a, const float *z, int M, int C, const float *mean, const float *invstd, float *dg, float *dbe,
                    hipStream_t st);
void bt_bn_bwd_apply(float *da, const float *a, const float *z, size_t n, int M, int C, const float *mean, const float *invstd, const float *gamma,
                     const float *dg, const float *dbe, hipStream_t st);
void bt_rowmax(const float *a, int B, int N, int C, float *out, int *arg, hipStream_t st);        // value + first argmax row
void bt_pool_scatter(const float *d_pool, const int *arg, int B, int N, int C, float *d_a, hipStream_t st);   // on a zeroed d_a
void bt_mix(const float *x, const float *T, int R, int N, int k, float *out, hipStream_t st);
void bt_mix_bwd(const float *x, const float *d_xin, int B, int N, int k, float *dT, hipStream_t st);
void bt_segsum(const float *dz, int B, int N, int C, float *out, hipStream_t st);                 // [B, N, C] -> [B, C] sums
void bt_logits(const float *z, int B, int N, int C, float *logits, hipStream_t st);               // z [B * N, C] -> logits [B, C, N]
void bt_logits_to_rows(const float *logits, int B, int N, int C, float *z, hipStream_t st);       // and back
void bt_fill(float *p, size_t n, float v, hipStream_t st);
void bt_add(float *y, const float *x, size_t n, hipStream_t st);
// out = keep(i) ? a * 1 / (1 - p) : 0 with the hash base of (seed, stream 0); out == a is allowed
void bt_dropout(const float *a, size_t n, uint32_t seed, float p, float *out, hipStream_t st);
void bt_log_softmax(const float *z, int B, int C, float *out, hipStream_t st);                    // C <= 64
void bt_log_softmax_bwd(const float *z, const float *d_out, int B, int C, float *dz, hipStream_t st);

// forward of one layer: r.z = A[:, :K] W[:, w0 : w0 + K]^T + b (+ add[row / per]); statistics (the running ones when `running`); r.a
int fwd_layer(const TLayer &l, Rec &r, bool running, const float *A, int lda, int ldw, int w0, const float *add, int per, hipStream_t st);
// backward of one layer: `da` [M, cout] (overwritten with dz) -> parameter gradients; dA [M, K] (=, or += when accumulate) unless nullptr.
// dgs / dbs [cout]: scratch for the BatchNorm sums where g.dg / g.dbe is nullptr
int bwd_layer(const TLayer &l, const TGrad &g, const Rec &r, float *dgs, float *dbs, float *da, const float *A, int lda, int ldw, int w0, float *dA,
              int ld_dA, int accumulate, hipStream_t st);

}  // namespace ampnet
