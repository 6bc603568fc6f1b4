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
#include "kernels.h"
#include "sa_tiles.h"

namespace ampnet {

struct SegPlan {
    int n_classes, hidden;
    int w2_off;                           // float offset of the staged W2 [32][hidden + 1] behind the waves' tiles (MlpLds::s_w)
    const float *w2, *b2;
};

// train mode's dropout of conv1's activations (seg_head_train.hip): element i = row * hidden + channel of h is kept when
// mix32(i ^ base) >= thr and then scaled by `scale`; thr = 0 keeps everything and is never hashed (the host sends DROP = false)
struct SegDrop {
    uint32_t base, thr;
    float scale;
};

// what both entry points and the two sizing functions derive from the shape
struct SegShape {
    int n_tiles, grid, chunk_rows, chunks, ldxs0;
    size_t fold_floats;                   // the BatchNorm fold at the start of either workspace
    MlpBwdLayout lay;                     // the backward's: conv1 as one layer of the shared layout
    size_t off_hs, off_dz2, off_parts2, off_dw2, floats;
    // train mode (seg_head_train.hip, seg_head_train_bwd.hip), behind the eval layouts: the forward's partial rows of the statistics
    // [grid][3 hidden] behind the fold, the backward's two coefficients per channel behind dW2
    size_t off_stats, train_fwd_floats, off_coef, train_floats;
};

// the plan of a backward kernel (eval: seg_head_bwd.hip; train: phase 1 of seg_head_train_bwd.hip), one wave per workgroup
struct SegBwdPlan {
    int off_h, off_d, off_g, off_w2;      // float offsets of the tiles in LDS (X is at 0); D and G have the row stride 33
    int ld_x, ld_h, ldxs0;
    float *xs0, *dz1, *hs, *dz2, *parts, *parts2;
};

constexpr int SEG_LD_D = 33;

// fills b from the plan and the workspace laid out by sh; returns the dynamic LDS bytes: X, H, D, G and the staged W2
inline size_t seg_bwd_plan(const MlpPlan &p, const SegShape &sh, float *ws, SegBwdPlan &b)
{
    const int hidden = p.cout[0];
    b = {};
    b.ld_x = p.kp[0] + 1;
    b.ld_h = hidden + 1;
    b.off_h = 32 * b.ld_x;
    b.off_d = b.off_h + 32 * b.ld_h;
    b.off_g = b.off_d + 32 * SEG_LD_D;
    b.off_w2 = b.off_g + 32 * SEG_LD_D;
    b.ldxs0 = sh.ldxs0;
    b.parts = ws + sh.lay.off_parts;
    b.xs0 = ws + sh.lay.off_xs[0];
    b.dz1 = ws + sh.lay.off_dz[0];
    b.hs = ws + sh.off_hs;
    b.dz2 = ws + sh.off_dz2;
    b.parts2 = ws + sh.off_parts2;
    return (size_t)(b.off_w2 + 32 * (hidden + 1)) * sizeof(float);
}

// checks the limits (`what` opens every message) and fills sh
int seg_shape(const char *what, int cin, int hidden, int n_classes, long long M, SegShape &sh);
// the arguments both entry points take the same way: the input rows, the 8 parameters, the limits, the workspace
int seg_check_entry(const char *what, const float *x, int ld, int cin, int hidden, int n_classes, long long M, const float *const *params_host,
                    SegShape &sh);
// train mode's two checks on top of the eval head's (seg_head_train.hip): seg_shape and 2 <= M <= AMPNET_SEG_HEAD_TRAIN_MAX_ROWS; 0 <= drop_p < 1
int segt_shape(const char *what, int cin, int hidden, int n_classes, long long M, SegShape &sh);
int segt_check_drop(const char *what, float drop_p);
// The plan of seg_head_forward_kernel (tile A also carries z, tile B conv1's activations; W2 staged, then W1 if it fits) from the 8
// parameters; slots 4 and 5 are running_mean and running_var (eval) or save_mean and save_invstd (train: fold with fpt_fold_launch).
// lds: the launch's dynamic LDS bytes.
int seg_forward_plan(const char *what, int cin, int hidden, const float *const *params_host, float eps, MlpPlan &p, MlpFold &f, size_t &lds);
// seg_head_forward_kernel on `st` with the fold already in place; drop == nullptr: eval mode
int seg_forward_launch(const char *what, const MlpPlan &p, size_t lds, const SegPlan &s, const SegDrop *drop, const float *x, int ld, long long M,
                       const float *fold, int n_tiles, float *logp, long long *preds, hipStream_t st);
// what both backwards end with (seg_head_bwd.hip): dW1 = dz1^T x, dW2 = dz^T h through the workspace copy [32][hidden], db2 from the
// workgroups' partials; ws is the workspace laid out by sh
int seg_weight_grads_launch(const char *what, const SegShape &sh, float *ws, int cin, int hidden, int n_classes, long long M,
                            float *const *grads_host, hipStream_t st);

// keep-and-scale of the first `rows` rows of conv1's activations h [32][ldh] in place; row0: the tile's first row among all M.  Each lane
// hashes the elements it rewrites (consecutive lanes, consecutive channels); the caller orders it with wave_lds_sync() on either side.
__device__ __forceinline__ void seg_dropout(float *h, int ldh, int hidden, long long row0, int rows, const SegDrop &d, int lane)
{
    const uint32_t e0 = (uint32_t)row0 * (uint32_t)hidden;      // (M * hidden <= 2^32: the counter of the last element fits)
    for (int e = lane; e < rows * hidden; e += 64) {
        const int t = e / hidden, c = e - t * hidden;
        const float v = h[t * ldh + c];
        h[t * ldh + c] = mix32((e0 + (uint32_t)e) ^ d.base) >= d.thr ? v * d.scale : 0.0f;
    }
}

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
