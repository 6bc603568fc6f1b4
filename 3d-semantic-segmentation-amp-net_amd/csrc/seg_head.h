// seg_head.h -- what the forward and the backward of the PointNet++ segmentation head share (seg_head.hip, seg_head_bwd.hip; C ABI:
// ampnet_seg_head_forward_f32, ampnet_seg_head_backward_f32): the shape rules, and the device code a wave runs on its 32 rows between
// conv1's activations h and the log-probabilities.  conv1 itself is the shared MLP core (fused_mlp.h) with one layer.
//
//   * W2 [n_classes][hidden] is staged ONCE per workgroup into LDS as [32][hidden + 1], the rows past n_classes zeros: mlp_accumulate reads 32
//     weight rows per column tile without a guard, and nothing past the caller's n_classes * hidden floats is ever read.
//   * z = W2 h + b2 leaves the accumulator (class r in lane r, 16 rows per lane half) through an LDS tile, so that ONE lane holds a row's
//     classes: the max, the lowest arg-max and the sum S over c ascending are then plain loops, the same in both kernels -- the
//     backward finds the forward's bits again.
#pragma once
#include "fp_bwd_tiles.h"
#include "sa_tiles.h"

namespace ampnet {

struct SegPlan {
    int n_classes, hidden;
    int w2_off;                           // float offset of the staged W2 [32][hidden + 1] behind the waves' tiles (MlpLds::s_w)
    const float *w2, *b2;
};

// what both entry points and the two sizing functions derive from the shape
struct SegShape {
    int n_tiles, grid, chunk_rows, chunks, ldxs0;
    size_t fold_floats;                   // the BatchNorm fold at the start of either workspace
    MlpBwdLayout lay;                     // the backward's: conv1 as one layer of the shared layout
    size_t off_hs, off_dz2, off_parts2, off_dw2, floats;
};

// checks the limits (`what` opens every message) and fills sh
int seg_shape(const char *what, int cin, int hidden, int n_classes, long long M, SegShape &sh);
// the arguments both entry points take the same way: the input rows, the 8 parameters, the limits, the workspace
int seg_check_entry(const char *what, const float *x, int ld, int cin, int hidden, int n_classes, long long M, const float *const *params_host,
                    SegShape &sh);

// W2 -> s_w2 [32][hidden + 1], the rows past n_classes zeros.  The caller's barrier publishes it.
__device__ __forceinline__ void seg_stage_w2(float *s_w2, const float *__restrict__ w2, int n_classes, int hidden, int tid, int nthreads)
{
    const int ldw = hidden + 1, have = n_classes * hidden;
    for (int e = tid; e < 32 * hidden; e += nthreads) {
        const int o = e / hidden, k = e - o * hidden;
        s_w2[o * ldw + k] = e < have ? w2[e] : 0.0f;
    }
}

// rows < rows of x [.][ldg], cin columns -> the wave's tile [32][ld], kp columns: the columns past cin and the rows past `rows` are zeros
// and nothing is read for them.  Consecutive lanes take consecutive columns (kp <= 32: a lane half per row, two rows at a time).
__device__ __forceinline__ void seg_load_rows(float *tile, int ld, int kp, const float *__restrict__ x, int ldg, int cin, int rows, int lane)
{
    if (kp <= 32) {
        const int c = lane & 31;
        if (c < kp)
            for (int t = lane >> 5; t < 32; t += 2) tile[t * ld + c] = t < rows && c < cin ? x[(size_t)t * ldg + c] : 0.0f;
        return;
    }
    for (int t = 0; t < 32; ++t)
        for (int c = lane; c < kp; c += 64) tile[t * ld + c] = t < rows && c < cin ? x[(size_t)t * ldg + c] : 0.0f;
}

// z = W2 h + b2 of the wave's rows h [32][ldh] -> zt [32][ldz], columns < 32 (the columns past n_classes hold zeros: their weight rows are).
// The contraction is the forward core's: hidden ascending in blocks of 8, k = k0 + 4 half + i, one fmaf chain per element; then + b2.
__device__ __forceinline__ void seg_logits(const float *ht, int ldh, const float *s_w2, int hidden, const float *__restrict__ b2, int n_classes,
                                           float *zt, int ldz, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[1];
    mlp_accumulate<1, K_QUADS, false>(acc, mlp_operand<K_QUADS>(ht, ldh, r, h), s_w2, hidden + 1, hidden, hidden, 0, r, h);
    const float b = r < n_classes ? b2[r] : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) zt[mlp_acc_row(i, h) * ldz + r] = acc[0][i] + b;
}

// One row of z -> its log-probabilities in place; returns the lowest class that attains the max.  m = max_c z_c, S = sum over c ascending
// of expf(z_c - m), logp_c = (z_c - m) - logf(S).
__device__ __forceinline__ int seg_log_softmax_row(float *z, int n_classes)
{
    float m = z[0];
    int arg = 0;
    for (int c = 1; c < n_classes; ++c) {
        const float v = z[c];
        if (v > m) {
            m = v;
            arg = c;
        }
    }
    float S = 0.0f;
    for (int c = 0; c < n_classes; ++c) S += expf(z[c] - m);
    const float ls = logf(S);
    for (int c = 0; c < n_classes; ++c) z[c] = (z[c] - m) - ls;
    return arg;
}

}  // namespace ampnet
