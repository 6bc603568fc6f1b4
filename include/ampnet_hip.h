/* ampnet_hip.h -- C ABI of libampnet_hip.so: the MI355X (gfx950) implementation of the AMP-Net
 * per-window hot path of marionacaros/3D-semantic-segmentation-AMP-Net.
 *
 * The reference has no FFI: its boundary for this path is Python (nn.Module.forward signatures,
 * function signatures, state_dict keys).  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root); the Python package
 * `3d-semantic-segmentation-amp-net_amd/` binds them with ctypes behind modules of the reference's
 * names (see INTEGRATION.md for the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; caller owns every buffer;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and never synchronised;
 *   - return value 0 = ok, negative = error (AMPNET_E_*); ampnet_last_error() gives the text
 *     (thread-local).  No exception crosses the ABI;
 *   - state the library keeps between calls: the thread-local error string; the process-wide default matrix precision
 *     (ampnet_set_matrix_precision); each thread's stack of scoped precision overrides (ampnet_precision_scope_begin / _end);
 *     the host-side tags that record which precision a train-mode forward wrote its workspace in; the collective callback
 *     (ampnet_set_collective) and the event profiler.  Nothing else survives a call.
 *   - float tensors are fp32, row-major, point-major: activations are [rows, channels].
 *
 * Window batching: the reference calls its encoder W times per step, each time on the B windows that
 * occupy cluster slot w (train_pointnet-attention.py:396-410); BatchNorm statistics are therefore
 * per slot.  Here all Q = B*W windows go through one launch sequence; window q = b*W + w (sample-major,
 * the order of lo_feats in the reference, train_pointnet-attention.py:415-417) and `n_slots` = W tells
 * the kernels that windows with equal q % n_slots share batch statistics.  Eval mode ignores slots.
 */
#ifndef AMPNET_HIP_H
#define AMPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMPNET_ABI_VERSION 18

enum {
    AMPNET_OK = 0,
    AMPNET_E_ARG = -1,        /* bad shape / null pointer / unsupported size */
    AMPNET_E_LAUNCH = -2,     /* hipGetLastError() after a launch            */
    AMPNET_E_WORKSPACE = -3,  /* workspace too small                         */
    AMPNET_E_DEVICE = -4      /* not a gfx950 device / no device             */
};

int ampnet_abi_version(void);
const char *ampnet_last_error(void);

/* ---- a1: farthest-point sampling ---------------------------------------------------------------
 * replaces utils/utils.py:889-933 `fps(pc, n_samples)` (driver data_proc/sample_fps.py:23-31).
 * xyz: [n_clouds, n, ld] fp32, columns 0..2 = x,y,z (ld >= 3 lets the caller pass whole rows).
 * idx: [n_clouds, s] int32, selection order; idx[c][0] == 0 (utils.py:907-908).
 * Bit-exact with the reference: float32 ((dx*dx + dy*dy) + dz*dz), running minimum, first maximum.
 * 1 <= s <= n <= AMPNET_FPS_MAX_POINTS.  Clouds of up to AMPNET_FPS_RESIDENT_MAX points are register-resident and need no
 * workspace (workspace may be NULL); larger clouds (the raw 100 x 100 m tiles of data_proc/sample_fps.py:23-26) stream
 * their coordinates and running minima from a structure-of-arrays copy in `workspace` (ampnet_fps_workspace_bytes(n_clouds, n) bytes).  */
#define AMPNET_FPS_RESIDENT_MAX 16384
#define AMPNET_FPS_MAX_POINTS (1 << 24)
size_t ampnet_fps_workspace_bytes(int n_clouds, int n);
int ampnet_fps_f32(const float *xyz, int n_clouds, int n, int ld, int s, int32_t *idx, void *workspace,
                   size_t workspace_bytes, void *stream);

/* The same sampling for a RAGGED batch -- what one stage of data_proc/sample_fps.py:12-34 does to a directory of files of unequal size,
 * in ONE launch: cloud b = rows cloud_off[b] .. cloud_off[b + 1] of rows [total_rows, ld]; its out_off[b + 1] - out_off[b] samples (clamped
 * to the cloud's size) go to idx[out_off[b] ..) as indices RELATIVE to the cloud, selection order, first = 0.  cloud_off / out_off:
 * DEVICE int32 arrays of n_clouds + 1 ascending offsets; max_n = the largest cloud (picks the kernel: every cloud of the launch runs the
 * variant built for max_n, so callers bucket files by size class -- data_proc/sample_fps.py of the package does).  Same arithmetic, same
 * tie rule, bit-identical to ampnet_fps_f32 cloud by cloud.  max_n > AMPNET_FPS_RESIDENT_MAX needs ampnet_fps_ragged_workspace_bytes().
 * HARD PRECONDITION: max_n >= every cloud of the launch (registers and LDS are sized for it; the offsets live on the device, so the host
 * cannot check).  A cloud that breaks it is refused inside the kernel: the first index of its output range reads -1, nothing else is written. */
size_t ampnet_fps_ragged_workspace_bytes(int total_rows, int max_n);
int ampnet_fps_ragged_f32(const float *rows, int ld, const int32_t *cloud_off, const int32_t *out_off, int n_clouds, int total_rows,
                          int max_n, int32_t *idx, void *workspace, size_t workspace_bytes, void *stream);

/* diagnostic build of the 8192-point kernel (one cloud): stamps[4 r + {0,1,2,3}] = s_memtime of thread 0 after the update,
 * after the barrier, after the slot fold and after the winner's coordinates landed in round r (FPS round anatomy).
 * The stamps go to a buffer nothing else reads; idx is the ordinary result.                                              */
int ampnet_fps_round_stamps(const float *xyz, int n, int ld, int s, int32_t *idx, unsigned long long *stamps, void *stream);

/* rows gather: out[c][i][:] = src[c][idx[c][i]][:]  (the `pc[sample_inds]` of utils.py:933)         */
int ampnet_gather_rows_f32(const float *src, const int32_t *idx, int n_clouds, int n, int ld, int s,
                           float *out, void *stream);

/* ---- parameter tables -----------------------------------------------------------------------------
 * Model parameters cross the ABI as HOST arrays of DEVICE pointers, one entry per state_dict tensor of the
 * reference modules, in the fixed order below (the order of `params.ENC_PARAMS` / `ENC_BUFFERS` /
 * `HEAD_PARAMS` / `HEAD_BUFFERS` in the Python package; ampnet_*_name(i) returns the state_dict key):
 *   encoder params  (52): input_transform.{conv_1,conv_2,conv_3}.weight, bn_1..5.{weight,bias},
 *                         fc_1.weight, fc_2.weight, fc_3.{weight,bias}; feature_transform.<same 17>;
 *                         conv_1..6.weight; bn_1..6.{weight,bias}          (pointnetAtt.py:14-26, 66-78)
 *   encoder buffers (32): (running_mean, running_var) of input_transform.bn_1..5, feature_transform.bn_1..5,
 *                         bn_1..6
 *   head params     (18): fc1.{weight,bias}, fc2.{weight,bias}, attention.in_proj_{weight,bias},
 *                         attention.out_proj.{weight,bias}, conv_2.{weight,bias}, conv_3.{weight,bias},
 *                         conv_4.{weight,bias}, bn_2.{weight,bias}, bn_3.{weight,bias}   (pointnetAtt.py:160-174)
 *   head buffers     (4): (running_mean, running_var) of bn_2, bn_3
 * Only the AMP-Net configuration is built: point_dimension 3, 9 features, global 256, local 64,
 * 8 heads, <= 8 classes (train_pointnet-attention.py:110-118).                                      */
int ampnet_table_count(int table);                 /* table: 0 enc params, 1 enc buffers, 2 head params, 3 head buffers */
const char *ampnet_table_name(int table, int i);
long ampnet_table_numel(int table, int i);

/* ---- a2/a3: encoder forward ---------------------------------------------------------------------
 * replaces BasePointNet.forward (pointNet/model/pointnetAtt.py:80-112; TransformationNet.forward :28-47) for the
 * W encoder calls of one step (train_pointnet-attention.py:396-410) at once.
 *   x          [total_rows, 9]      the windows back to back; window q = rows win_off[q] .. win_off[q+1]
 *   win_off    [Q + 1] int32 (device); max_rows = the largest window
 *   n_slots    windows q with equal q % n_slots share BatchNorm batch statistics (train); Q = B * n_slots with
 *              q = b * n_slots + w.  Ignored in eval mode (running statistics).
 *   local      [total_rows, 64]     local_point_features (:97)
 *   global_feat[Q, 256]             max-pooled global feature (:104-106), row q
 *   feat_T     [Q, 64, 64]          feature_transform (:94); in_T [Q, 3, 3] input_transform (:84), may be NULL.
 *              Row order of feat_T / in_T: eval: q.  train: slot-major, row (q % n_slots) * (Q / n_slots) + q / n_slots,
 *              so the LAST slot's B matrices (what the reference's reg loss uses, train_pointnet-attention.py:463)
 *              are the last B rows.
 *   train != 0: batch statistics, running statistics updated in place (momentum 0.1, one update per slot in
 *              slot order, like W encoder calls); the workspace then holds what ampnet_encoder_bwd_f32 needs.
 * Eval logits built on these outputs match the reference CPU forward within 1e-3 (tests/test_forward_gpu.py). */
size_t ampnet_encoder_workspace_bytes(int Q, int n_slots, int total_rows, int max_rows, int train);
int ampnet_encoder_fwd_f32(const float *const *params_host, float *const *buffers_host, const float *x,
                           const int32_t *win_off, int Q, int n_slots, int total_rows, int max_rows, int train,
                           float *local, float *global_feat, float *feat_T, float *in_T, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---- a2/a3 backward -----------------------------------------------------------------------------------
 * replaces autograd's backward through BasePointNet.forward (the reference: loss.backward(),
 * train_pointnet-attention.py:467) for all windows of a step.  Must follow a train-mode
 * ampnet_encoder_fwd_f32 on the same x / win_off / Q / n_slots with `fwd_workspace` untouched in between.
 *   grads_host [52] device pointers, same order as params_host; every gradient is WRITTEN (not accumulated)
 *   local, feat_T   the forward's outputs (read)
 *   d_local  [total_rows, 64] or NULL; d_global [Q, 256] (row q); d_feat_T [Q, 64, 64] (slot-major rows, like
 *            feat_T in train mode) or NULL: gradients of the loss wrt the three forward outputs.         */
size_t ampnet_encoder_bwd_workspace_bytes(int Q, int n_slots, int total_rows, int max_rows);
int ampnet_encoder_bwd_f32(const float *const *params_host, float *const *grads_host, const float *x,
                           const int32_t *win_off, int Q, int n_slots, int total_rows, int max_rows,
                           const float *local, const float *d_local, const float *d_global, const float *d_feat_T,
                           const float *feat_T, void *fwd_workspace, size_t fwd_workspace_bytes, void *bwd_workspace,
                           size_t bwd_workspace_bytes, void *stream);

/* ---- a4 (+a6 forward): attention head -------------------------------------------------------------
 * replaces SegmentationWithAttention.forward (pointNet/model/pointnetAtt.py:176-209) and, optionally, the
 * loss / prediction lines of train_loop (train_pointnet-attention.py:138,445-450).
 *   gl         [B * W, 256]   window tokens, row q = b * W + w (the reference's gl_feats[w, b, :])
 *   lo         [total_rows, 64] local features; sample b owns rows of windows b*W .. b*W + W - 1 back to back
 *                             (the reference's lo_feats[b]); every sample has the same np_cluster list, so
 *                             total_rows = B * P and window (b, w) has np_cluster[w] rows (win_off says so)
 *   centroids  [B, W, 2]
 *   key_pad_mask [B, W] bytes, non-zero = ignore that cluster token as a key; NULL = no mask (:189)
 *   logits     [B, n_classes, P]                                                             (:207-209)
 *   train != 0: batch statistics for bn_2 / bn_3 (over all B * P rows), running stats updated, dropout with
 *              probability drop_p on the attention weights and after both ReLUs (:204-206) from the
 *              counter-based generator keyed by `seed`; eval: running statistics, no dropout.
 *   targets    [B, P] int64 (-1 = ignore), class_w [n_classes], preds [B, P] int64, loss_out [2]
 *              (weighted-mean CE, sum of weights): all optional (NULL).                              */
size_t ampnet_head_workspace_bytes(int B, int W, int total_rows, int max_rows, int n_classes, int train);
/* The eval forward for SEVERAL FILES in one launch sequence (the reference's test loop, test_pointnet_att_segmen.py:127-181, runs one file
 * of <= W ragged clusters per step at batch 1): file f owns the window slots f * W .. f * W + W - 1, its real clusters first; unused slots
 * are windows of zero rows (win_off repeats its value) with key_pad_mask[f, w] = 1, so a file's attention sees exactly its own clusters.
 * Files differ in their point counts: logits [n_classes, total_rows] and preds [total_rows] run over the concatenated rows.
 * workspace: ampnet_head_workspace_bytes(n_files, W, total_rows, max_rows, n_classes, 0).  Results are identical, file by file, to
 * ampnet_head_fwd_f32 with B = 1 (tests/test_inference_gpu.py).                                                                   */
int ampnet_head_fwd_files_f32(const float *const *params_host, float *const *buffers_host, const float *gl, const float *lo,
                              const float *centroids, const int32_t *win_off, const uint8_t *key_pad_mask, int n_files, int W,
                              int total_rows, int max_rows, int n_classes, float *logits, long long *preds, void *workspace,
                              size_t workspace_bytes, void *stream);
int ampnet_head_fwd_f32(const float *const *params_host, float *const *buffers_host, const float *gl,
                        const float *lo, const float *centroids, const int32_t *win_off,
                        const uint8_t *key_pad_mask, int B, int W, int total_rows, int max_rows, int n_classes,
                        int train, float drop_p, uint32_t seed, float *logits, const long long *targets,
                        const float *class_w, long long *preds, float *loss_out, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ---- a4 backward ---------------------------------------------------------------------------------------
 * autograd backward of SegmentationWithAttention.forward given dlogits [B, n_classes, P].  Must follow a
 * train-mode ampnet_head_fwd_f32 with the same arguments (drop_p, seed included) and an untouched fwd_workspace.
 *   grads_host [18] device pointers in the order of the head parameters; every gradient is WRITTEN
 *   d_lo [total_rows, 64] = dL/d(lo), d_gl [B * W, 256] = dL/d(gl) (row b * W + w); centroids get no gradient. */
size_t ampnet_head_bwd_workspace_bytes(int B, int W, int total_rows, int max_rows, int n_classes);
int ampnet_head_bwd_f32(const float *const *params_host, float *const *grads_host, const float *lo,
                        const float *centroids, const int32_t *win_off, int B, int W, int total_rows, int max_rows,
                        int n_classes, float drop_p, uint32_t seed, const float *dlogits, float *d_lo, float *d_gl,
                        void *fwd_workspace, size_t fwd_workspace_bytes, void *bwd_workspace,
                        size_t bwd_workspace_bytes, void *stream);

/* ---- f4: the GRU variant of the sequence model ---------------------------------------------------------------
 * replaces SegmentationWithGRU.forward (pointNet/model/pointnetAtt.py:212-258: nn.GRU(256 -> 64, batch_first, h0 = 0) over the W window
 * tokens of a sample, the hidden state of step w repeated over the points of window w, cat with the local features, conv_2 / bn_2 /
 * conv_3 / bn_3 / conv_4 with two dropouts) as pointNet/rnn/train_pointnetGRU.py:335-441 drives it; the repeat + cat is never built.
 *   params_host  [14] device pointers in state_dict order: gru_global.weight_ih_l0 [192,256], weight_hh_l0 [192,64], bias_ih_l0 [192],
 *                bias_hh_l0 [192], conv_2.weight [128,128], conv_2.bias, conv_3.weight [64,128], conv_3.bias, conv_4.weight [C,64],
 *                conv_4.bias, bn_2.weight, bn_2.bias, bn_3.weight, bn_3.bias
 *   buffers_host [4]  bn_2.running_mean, bn_2.running_var, bn_3.running_mean, bn_3.running_var (updated in train mode)
 *   gl [B * W, 256] window tokens (row b * W + w = global_seq[b, w, :]); lo, win_off, logits, targets, class_w, preds, loss_out,
 *   train, drop_p, seed: as ampnet_head_fwd_f32.  There is no key-padding mask: the reference runs the GRU over every window.   */
size_t ampnet_gru_head_workspace_bytes(int B, int W, int total_rows, int max_rows, int n_classes, int train);
int ampnet_gru_head_fwd_f32(const float *const *params_host, float *const *buffers_host, const float *gl, const float *lo,
                            const int32_t *win_off, int B, int W, int total_rows, int max_rows, int n_classes, int train, float drop_p,
                            uint32_t seed, float *logits, const long long *targets, const float *class_w, long long *preds,
                            float *loss_out, void *workspace, size_t workspace_bytes, void *stream);
/* autograd backward of the above given dlogits [B, n_classes, P] (must follow a train-mode forward with the same arguments and an
 * untouched fwd_workspace): grads_host [14] are WRITTEN; d_lo [total_rows, 64], d_gl [B * W, 256].                                */
size_t ampnet_gru_head_bwd_workspace_bytes(int B, int W, int total_rows, int max_rows, int n_classes);
int ampnet_gru_head_bwd_f32(const float *const *params_host, float *const *grads_host, const float *gl, const float *lo,
                            const int32_t *win_off, int B, int W, int total_rows, int max_rows, int n_classes, float drop_p, uint32_t seed,
                            const float *dlogits, float *d_lo, float *d_gl, void *fwd_workspace, size_t fwd_workspace_bytes,
                            void *bwd_workspace, size_t bwd_workspace_bytes, void *stream);

/* ---- f4: classification head on the window tokens ------------------------------------------------------------------------
 * replaces ClassificationWithAttention.forward (pointNet/model/pointnetAtt.py:115-151): MultiheadAttention over the W tokens of a sample,
 * conv_1 (Conv1d(num_w -> 1, 1)) over the attention output RE-VIEWED as [B, W, 256] (the reference views the sequence-first tensor, it
 * does not transpose it; restated literally), fc_2 -> bn_2 (over the B rows) -> ReLU -> fc_3.  No reference script reaches this module
 * (train_pointnet-attention.py:440-442 leaves the classification branch without a model call); built for the module's own contract.
 *   params_host  [12] attention.in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, conv_1.weight [1, W, 1], conv_1.bias [1],
 *                fc_2.weight [128, 256], fc_2.bias, fc_3.weight [C, 128], fc_3.bias, bn_2.weight, bn_2.bias
 *   buffers_host [2]  bn_2.running_mean, bn_2.running_var
 *   gl [B * W, 256] (row b * W + w = gl_feats[w, b, :]); key_pad_mask [B, W] or NULL; out [B, n_classes];
 *   attn_weights [B, W, W] or NULL: the attention probabilities averaged over the heads (after dropout in train mode), need_weights=True */
size_t ampnet_cls_head_workspace_bytes(int B, int W);
int ampnet_cls_head_fwd_f32(const float *const *params_host, float *const *buffers_host, const float *gl, const uint8_t *key_pad_mask, int B,
                            int W, int n_classes, int train, float drop_p, uint32_t seed, float *out, float *attn_weights, void *workspace,
                            size_t workspace_bytes, void *stream);
/* autograd backward given d_out [B, n_classes] (after a train-mode forward with the same arguments): grads_host [12] WRITTEN, d_gl [B * W, 256] */
size_t ampnet_cls_head_bwd_workspace_bytes(int B, int W);
int ampnet_cls_head_bwd_f32(const float *const *params_host, float *const *grads_host, const float *gl, int B, int W, int n_classes, float drop_p,
                            uint32_t seed, const float *d_out, float *d_gl, void *fwd_workspace, size_t fwd_workspace_bytes,
                            void *bwd_workspace, size_t bwd_workspace_bytes, void *stream);

/* ---- a6: loss recipe (train_pointnet-attention.py:138,445,463-467) ------------------------------------
 * reg = || I - F F^T ||_F over the whole stack feat_T [n, 64, 64] (torch.norm of a 3-D tensor = Frobenius over
 * all elements).  G [n, 64, 64] (optional) receives I - F F^T for the backward; part [n] is scratch.
 * ampnet_reg_loss_bwd_f32:  d_feat_T += coef * d(reg)/d(feat_T).
 * ampnet_ce_bwd_f32:        dlogits = grad_scale * d(ce)/d(logits) for the weighted-mean CE the head forward
 *                           returned in loss2 = {ce, sum of weights} (ignore_index -1).                     */
int ampnet_reg_loss_fwd_f32(const float *feat_T, int n, float *reg_out, float *G, float *part, void *stream);
int ampnet_reg_loss_bwd_f32(const float *feat_T, const float *G, const float *reg, float coef, int n, float *d_feat_T,
                            void *stream);
/* the same gradient WRITTEN into a stack d_feat_T_stack [n_total, 64, 64] whose last n matrices are the regularised ones (the reference
 * regularises the feature transform of the last cluster only, train_pointnet-attention.py:445): zeros in the first n_total - n, the
 * gradient (no accumulate) in the rest -- the gradient tensor of all feature transforms without a separate zero fill.                */
int ampnet_reg_loss_bwd_stack_f32(const float *feat_T, const float *G, const float *reg, float coef, int n, int n_total,
                                  float *d_feat_T_stack, void *stream);
int ampnet_ce_bwd_f32(const float *logits, const long long *targets, const float *class_w, const float *loss2,
                      float grad_scale, int B, int C, int P, float *dlogits, void *stream);

/* ---- a11 on the device: the counts behind get_accuracy / get_iou_obj (utils/get_metrics.py:6-31) ----------------------------------
 * counts[t * C + p] = number of points with target t and prediction p, counts[C * C] = number of ignored points (target -1 = padding,
 * what rm_padding removes, utils/utils.py:14-19); counts is WRITTEN ([C * C + 1] int64).  accuracy = trace / kept; IoU of label c =
 * counts[c][c] / (row sum c + column sum c - counts[c][c]).  Lets a training driver keep predictions on the device: no 2 x 9.4 MB
 * download and no synchronisation per step.                                                                                      */
/* the key-padding mask of train_loop (train_pointnet-attention.py:428-431): targets [B, P] int64 (cluster-major, -1 = padded point),
 * mask[b, w] = 1 iff targets[b, i * W + w] == -1 for every i -- the reference's literal `(targets_pc.view(B, -1, W) == -1).all(dim=1)`.
 * W <= 32, P % W == 0.  One launch instead of five torch launches per step.                                                         */
int ampnet_pad_mask_i64(const long long *targets, int B, int P, int W, uint8_t *mask, void *stream);
int ampnet_confusion_i64(const long long *preds, const long long *targets, long long n, int n_classes, long long *counts, void *stream);

/* ---- the token-level products of the backward (one row per window: the attention projections, the T-Net FC layers) ---------------------
 * C [M, N] (+)= op(A) op(B), op(A) = A [M, K] (trans_a = 0) or A^T with A [K, M]; op(B) = B [K, N] (trans_b = 0) or B^T with B [N, K];
 * row-major with leading dimensions lda / ldb / ldc; accumulate != 0 adds to C.  k_scale (optional, [K]): op(A)[m][k] is multiplied by k_scale[k]
 * as it is loaded, i.e. C = op(A) diag(k_scale) op(B) (the per-slot matrices W^T diag(P2) W of the pooled layers' backward); it also scales the
 * row sums.  row_sums (optional, [M]) receives sum_k op(A)[m][k]:
 * the bias gradient G^T 1 that rides in a weight-gradient product dW = G^T X (reference: autograd of nn.Linear / nn.MultiheadAttention
 * as train_pointnet-attention.py:463-467 calls it; this is not a reference interface, it is exported so that the kernel the backward
 * calls ~11 times per step can be tested on its own).  fp32 matrix cores, K split over the 16 waves of a workgroup in a fixed order:
 * bitwise reproducible.                                                                                                             */
int ampnet_small_gemm_f32(int trans_a, int trans_b, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C,
                          int ldc, int accumulate, float *row_sums, const float *k_scale, void *stream);

/* ---- a8 on the device: the input pipeline of train_loop in one kernel --------------------------------------------
 * replaces the host augmentation of train_pointnet-attention.py:390-405 (shuffle_clusters utils/utils.py:620-632,
 * rotate_point_cloud_z :582-604, shuffle_data :607-617) and the [B, N, 9, W] -> [B, W, N, 9] re-layout.
 *   pc [B, N, 9, W] float32 and targets [B, N, W] int64 (may be NULL with t_out) as collate_seq_padd returns them, on the device
 *   cluster_perm [W], point_perm [W, N] (NULL = identity) int32 on the device: x_out[b, w, n] = pc[b, point_perm[w, n], :, cluster_perm[w]]
 *   rotate != 0: (x, y, z) <- (x c - y s, x s + y c, z) in float64, rounded to float32 (numpy's float64 dot of the reference)
 *   x_out [B, W, N, 9], t_out [B, W, N]                                                                         */
int ampnet_augment_f32(const float *pc, const long long *targets, const int32_t *cluster_perm, const int32_t *point_perm,
                       double cos_a, double sin_a, int rotate, int B, int N, int W, float *x_out, long long *t_out, void *stream);

/* ---- a9 + a8 on the device: collate_seq_padd's resampling / padding fused into the augmentation kernel --------------------
 * replaces, together with the package's collate_seq_ragged (pointNet/collate_fns.py), the host work of pointNet/collate_fns.py:33-45
 * (every sample gathered to exactly N = 2048 points, the cluster axis padded to W = 9 by replicating the last cluster, targets padded
 * with -1) -- in the reference this runs in the DataLoader workers on 42 MB per batch of 64 and is what a train epoch waits for
 * (bench.py: train_att_epoch).  The workers hand over the RAGGED samples and the resampling map instead:
 *   pts     float32: sample b = [n_b, 9, w_b] (as LidarKmeansDataset returns it) at element offset meta[b][2]
 *   labels  int8   : sample b = [n_b, w_b] segmentation labels 0 .. 4 at element offset meta[b][3]
 *   idx     int32 [B, N]: padded row p of sample b is its own row idx[b][p] (the draws of collate_seq_padd: torch.randint when
 *                         n_b < N, random.sample when n_b > N, the identity when n_b == N)
 *   meta    int32 [B, 4]: n_b, w_b, pts offset, labels offset
 * and the kernel writes what ampnet_augment_f32 would have written for the padded batch, bit for bit (tests/test_augment_gpu.py):
 *   x_out[b, w, n, f] = pts_b[idx[b][pp], f, min(cw, w_b - 1)],  t_out[b, w, n] = cw < w_b ? labels_b[idx[b][pp], cw] : -1,
 *   cw = cluster_perm[w], pp = point_perm[w, n] (NULL = n), then the z-rotation as above.  All arrays on the device.          */
int ampnet_collate_augment_f32(const float *pts, const signed char *labels, const int32_t *idx, const int32_t *meta,
                               const int32_t *cluster_perm, const int32_t *point_perm, double cos_a, double sin_a, int rotate,
                               int B, int N, int W, float *x_out, long long *t_out, void *stream);

/* ---- the input pipeline of pn2_step.train_loop_clouds in one kernel: clouds of unequal size (BUILD-DEFINED, within ABI 18) ----------
 * What ampnet_augment_f32 is for the window batch, for the clusters of `<name>_clusters_list.pkl` files at their native sizes.  The
 * reference augments a batch with rotate_point_cloud_z (utils/utils.py:582-604, one angle per step) and shuffle_data (:607-617); it
 * has no ragged batch, so the layout and the shuffle below are this project's.
 *   raw      [total_in, 10] float32: the Q clouds back to back as they were uploaded, columns 0 .. 8 the features, column 9 the ASPRS
 *            class code; 8-byte aligned
 *   in_off   int32 [Q + 1]: cloud b is rows in_off[b] .. in_off[b + 1] of raw, n_b = in_off[b + 1] - in_off[b] >= 1, in_off[Q] = total_in
 *   out_off  int32 [Q + 1]: the same for the output, p_b = out_off[b + 1] - out_off[b] >= n_b (the package pads to
 *            p_b = max(n_b, npoint), utils.pad_cloud_sizes), out_off[Q] = total_out.  Both arrays on the device; they are TRUSTED (built
 *            by the caller on the host), as the meta of ampnet_collate_augment_f32 is
 *   rows     [total_out, 9] float32, 16-byte aligned; targets int64 [total_out]; src int32 [total_out] or NULL
 * Output row j of cloud b copies row s = in_off[b] + perm_b(j % n_b) of raw: rows[out_off[b] + j] = raw[s, 0:9], src[..] = s,
 *   targets[..] = j < n_b ? lut(raw[s, 9]) : -1     (the padding rows are ignored by the loss)
 *   lut(code): k = (long)code (truncated towards zero) clamped to [0, 255]; 15 -> 1, 14 -> 2, 3 and 4 -> 3, 5 -> 4, everything else 0
 *              (amp_test._label_lut; computed in the kernel, no table is read)
 *   rotate != 0: (x, y, z) <- (x c - y s, x s + y c, z) exactly as ampnet_augment_f32 does it -- the float64 product of the float32
 *              coordinates with [[c, s, 0], [-s, c, 0], [0, 0, 1]] column by column, no fused multiply-add, rounded to float32 once --
 *              bit for bit utils.rotate_point_cloud_z with the angle whose cosine and sine are cos_a, sin_a
 *   permute == 0: perm_b is the identity.  Otherwise perm_b is a STATELESS bijection of [0, n_b), never stored, a function of
 *              (seed, step, b, n_b) alone -- the convention of the dropout masks (a counter hash), with u32 wrapping arithmetic:
 *       mix32(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16           (the dropout hash)
 *       base = mix32(seed + step * 0x9E3779B9);   ck = mix32(base + b * 0x85EBCA6B)
 *       bits = max(bit_length(n - 1), 1);   half = (bits + 1) / 2;   mask = (1 << half) - 1            (a domain of 2^(2 half) <= 4 n)
 *       F(x):  L = x >> half, R = x & mask;  four rounds r = 0 .. 3: (L, R) <- (R, L ^ (mix32(ck ^ ((R << 2) | r)) & mask));
 *              F(x) = (L << half) | R                                          (a Feistel network: a bijection of the domain)
 *       perm_b(j) = the first of F(j), F(F(j)), ... that is < n                 (cycle walking: it ends because F is a bijection)
 *     An augmentation shuffle, not a uniform sampler: at n = 8 the least likely (position, source) pair came up 444 times in 4096 steps
 *     against 512 for a uniform draw.  The angle of a step is chosen by the caller; the package takes
 *     2 pi * mix32(base ^ 0x3C6EF372) / 2^32, so a step is reproducible from (seed, step) and draws from no global generator.
 * Every element of rows, targets and src is written (no memset needed), no atomics, deterministic.  Q >= 1, Q <= total_in <= total_out
 * < 2^31.                                                                                                                        */
int ampnet_cloud_input_f32(const float *raw, const int32_t *in_off, const int32_t *out_off, int Q, long long total_in,
                           long long total_out, uint32_t seed, uint32_t step, int permute, int rotate, double cos_a, double sin_a,
                           float *rows, long long *targets, int32_t *src, void *stream);

/* ---- k-NN grouping of FPS centres (BUILD-DEFINED; BASELINE.json north_star / config 5) ------------------------------
 * The reference has no k-NN or ball query: nothing is replaced, parity against it is "unpinned"; the spec
 * below is pinned by oracle/fps_oracle.py:knn_indices.
 *   xyz      [n_clouds, n, ld] float32 (first 3 columns used), n * 12 bytes <= 144 KB (n <= 12288)
 *   centres  [n_clouds, s] int32 point indices (e.g. the output of ampnet_fps_f32)
 *   out      [n_clouds, s, k] int32: for each centre the k points with the smallest (distance, index), ascending;
 *            distance = float32 ((dx*dx + dy*dy) + dz*dz), no fused multiply-add; the centre itself comes first   */
int ampnet_knn_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, int k, int32_t *out,
                   void *stream);

/* ---- ball-query grouping of FPS centres (BUILD-DEFINED like ampnet_knn_f32: the reference has no ball query) --------
 * The grouping of a PointNet++ set-abstraction layer (the reference imports it from a package it does not ship, pointnetAtt.py:4); the
 * spec below is pinned by the build's CPU restatement tests/sa_ref.py:ball_query.
 *   xyz      [n_clouds, n, ld] float32 (first 3 columns used), n * 12 bytes <= 144 KB (n <= 12288)
 *   centres  [n_clouds, s] int32 point indices (e.g. the output of ampnet_fps_f32)
 *   radius   >= 0; r2 = float32 (radius * radius), computed once on the host
 *   d(j)     = float32 ((dx*dx + dy*dy) + dz*dz), no fused multiply-add (the distance of ampnet_knn_f32);
 *              point j is a member of the ball when d(j) <= r2 (the boundary is included)
 *   out      [n_clouds, s, nsample] int32, 1 <= nsample <= AMPNET_SA_MAX_NSAMPLE: the first nsample members in ascending index order;
 *            with fewer members the remaining slots repeat the first member (the query_ball_point rule)
 *   count    [n_clouds, s] int32 = min(members, nsample); may be NULL.  A centre is a member of its own ball (finite coordinates),
 *            so count >= 1.                                                                                                       */
#define AMPNET_SA_MAX_NSAMPLE 64
int ampnet_ball_query_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, float radius, int nsample,
                          int32_t *out, int32_t *count, void *stream);

/* ---- ball query at K radii around the same centres (multi-scale grouping; added within ABI 17: a new symbol, nothing else moved) -----
 *   xyz, n_clouds, n, ld, centres, s   as in ampnet_ball_query_f32
 *   radii_host, nsample_host           HOST arrays [K], 1 <= K <= AMPNET_SA_MSG_MAX_SCALES; the radii in any order, equal ones allowed
 *   out_host                           HOST array of K DEVICE pointers, out_host[k] is [n_clouds, s, nsample_host[k]] int32
 *   count_host                         NULL, or a HOST array of K DEVICE pointers [n_clouds, s] int32 of which any may be NULL
 * For every k, out_host[k] and count_host[k] are bit for bit what ampnet_ball_query_f32 (.., radii_host[k], nsample_host[k], ..) writes:
 * the same d(j), r2_k = float32 (radius_k * radius_k) computed once per scale on the host, the boundary included, ascending index order,
 * the padding repeating the list's own first member.  One launch stages the cloud once and walks it once per centre: d(j) is formed
 * once per candidate and compared with every r2_k, and the walk ends with the step after which EVERY list is full.
 * Limits per scale are those of ampnet_ball_query_f32; a message names the offending scale.                                        */
#define AMPNET_SA_MSG_MAX_SCALES 4
int ampnet_ball_query_msg_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const float *radii_host,
                              const int *nsample_host, int K, int32_t *const *out_host, int32_t *const *count_host, void *stream);

/* ---- ball query of clouds of UNEQUAL size in one launch (new symbol within ABI 18: nothing else moved, AMPNET_ABI_VERSION stays 18) ----
 *   rows        [total, ld] float32 (first 3 columns used): the clouds back to back
 *   cloud_off   DEVICE int32 [n_clouds + 1], ascending, cloud_off[0] = 0, cloud_off[n_clouds] = total (the table of ampnet_fps_ragged_f32):
 *               cloud b is the rows cloud_off[b] .. cloud_off[b + 1], n_b of them
 *   total, max_n  HOST ints: the rows of `rows` and the largest n_b; 1 <= n_b <= max_n <= 12288 (max_n * 12 bytes <= 144 KB)
 *   centres     [n_clouds, s] int32, RELATIVE to their cloud (in [0, n_b)): the same s for every cloud
 *   radius, nsample   as in ampnet_ball_query_f32
 *   out         [n_clouds, s, nsample] int32;  count [n_clouds, s] int32 or NULL
 *   global_index   0: out[b] and count[b] are bit for bit what ampnet_ball_query_f32 writes for cloud b alone (n_clouds = 1, n = n_b) -- the
 *               same d(j), r2 formed once on the host, the boundary included, ascending index order, the padding repeating the list's
 *               first member.  1: the same lists with cloud_off[b] added to every stored index, padding included: they address `rows` as ONE
 *               cloud of `total` points (ampnet_sa_forward_f32 with n_clouds = 1, n = total, s = n_clouds * s).  count is the same.
 * One launch, cloud = blockIdx.y, the plan of ampnet_ball_query_f32 (one wave per centre, the cloud's coordinate planes in LDS); the
 * dynamic LDS is sized by max_n, so the LARGEST cloud sets the workgroups per CU of the whole call.  The kernel clamps a cloud's length
 * to max_n and a centre into its cloud and skips a cloud whose rows leave [0, total): a wrong table or centre gives wrong lists, never an
 * access outside `rows`.  Limits (AMPNET_E_ARG): max_n <= 12288, 1 <= nsample <= AMPNET_SA_MAX_NSAMPLE, n_clouds <= 65535; the host
 * cannot see cloud_off -- the Python binding checks the sizes and names the offending cloud.                                          */
int ampnet_ball_query_ragged_f32(const float *rows, int ld, const int32_t *cloud_off, int n_clouds, int total, int max_n,
                                 const int32_t *centres, int s, float radius, int nsample, int global_index, int32_t *out, int32_t *count,
                                 void *stream);

/* ---- one set-abstraction layer, eval mode, fused (stands in for PointNetSetAbstraction.forward of pointnetAtt.py:4,285-287) ---------
 *   xyz, centres          as in ampnet_ball_query_f32 (no limit on n here)
 *   group_idx             [n_clouds, s, nsample] int32 point indices (the output of ampnet_ball_query_f32), 1 <= nsample <= 64
 *   feats                 [n_clouds, n, D] float32, or NULL with D = 0
 *   params_host           HOST array of 6 L DEVICE pointers, per layer l < L <= AMPNET_SA_MAX_LAYERS: weight [cout_l, cin_l], conv bias,
 *                         BatchNorm weight, bias, running_mean, running_var (each [cout_l]); cin_0 = 3 + D, cin_l = cout_{l-1}
 *   cout_host, eps_host   HOST arrays [L]: the widths and the BatchNorm eps
 *   out                   [n_clouds, s, cout_{L-1}] float32
 *   workspace             AMPNET_SA_WORKSPACE_BYTES device bytes (the folded BatchNorm scale and shift)
 * Row t of centre i's group is [xyz[idx_t] - xyz[centre_i] (3 values), feats[idx_t] (D values)]; every layer computes
 * relu(bn_eval(W row + b)) with bn_eval folded into fma(W row, scale, shift), scale = gamma / sqrt(var + eps),
 * shift = (b - mean) * scale + beta; out is the per-channel max over the nsample rows.  Neither the grouped rows nor any intermediate
 * activation is written to memory.  Limits (anything else is refused with AMPNET_E_ARG, there is no other path):
 * cin_0 <= AMPNET_SA_MAX_CIN, every cout_l a multiple of 32 and <= AMPNET_SA_MAX_COUT.
 * Arithmetic: exact fp32 MFMA (v_mfma_f32_32x32x2_f32) whatever the matrix precision is -- neither ampnet_set_matrix_precision nor a
 * precision scope changes what this entry point computes.                                                                         */
#define AMPNET_SA_MAX_LAYERS 3
#define AMPNET_SA_MAX_CIN 320
#define AMPNET_SA_MAX_COUT 256
#define AMPNET_SA_WORKSPACE_BYTES (AMPNET_SA_MAX_LAYERS * 2 * AMPNET_SA_MAX_COUT * 4)
int ampnet_sa_forward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                          int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                          const float *eps_host, int L, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- K set-abstraction branches around the same centres in ONE launch (multi-scale grouping; added within ABI 17: new symbols) -------
 *   xyz .. s, feats, D    as in ampnet_sa_forward_f32; every branch has cin_0 = 3 + D and that entry point's row [relative xyz, feats]
 *   group_idx_host        HOST array of K DEVICE pointers, group_idx_host[k] is [n_clouds, s, nsample_host[k]] int32
 *   nsample_host, L_host  HOST arrays [K]: branch k's group size and its number of layers; 1 <= K <= AMPNET_SA_MSG_MAX_SCALES
 *   params_host (6 device pointers per layer), cout_host, eps_host   the branches' tables of ampnet_sa_forward_f32 laid end to end in
 *                         branch order: sum_k L_host[k] layers
 *   out                   [n_clouds, s, C] float32, C = sum_k cout_last_k; branch k owns the columns [off_k, off_k + cout_last_k),
 *                         off_k = sum_{j<k} cout_last_j
 *   workspace             ampnet_sa_msg_forward_workspace_bytes(K) = K * AMPNET_SA_WORKSPACE_BYTES device bytes (0 = K is refused):
 *                         branch k's BatchNorm fold lies in the k-th region
 * Branch k's column slice is bit for bit the `out` of ampnet_sa_forward_f32 on group_idx_host[k] with that branch's layers: the same
 * plan, gather and layer code, only the destination row differs (out + g C + off_k).  After the K fold launches ONE kernel runs every
 * branch: a workgroup belongs to one branch (taken from its index, so wave-uniform), stages that branch's weights once and walks that
 * branch's groups; the dynamic LDS is the largest of the branches' needs.  No atomics; nothing grouped and no activation reaches memory;
 * exact fp32 MFMA whatever the matrix precision is.  Limits per branch are those of ampnet_sa_forward_f32 (AMPNET_E_ARG otherwise); a
 * message names the offending branch.                                                                                              */
size_t ampnet_sa_msg_forward_workspace_bytes(int K);
int ampnet_sa_msg_forward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                              const int32_t *const *group_idx_host, const int *nsample_host, const float *feats, int D,
                              const float *const *params_host, const int *cout_host, const float *eps_host, const int *L_host, int K,
                              float *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- 3 nearest coarse points of every fine point (BUILD-DEFINED like ampnet_knn_f32) ---------------------------------------------------
 * The neighbour search of a PointNet++ feature-propagation layer (the reference imports the layer from a package it does not ship,
 * pointnetAtt.py:4); the spec below is pinned by the build's CPU restatement tests/fp_ref.py:three_nn.
 *   fine     [n_clouds, n, ld1] float32 (first 3 columns used), no limit on n
 *   coarse   [n_clouds, s, ld2] float32 (first 3 columns used), 1 <= s <= AMPNET_THREE_NN_MAX_S (s * 12 bytes <= 144 KB of LDS, the limit
 *            of ampnet_knn_f32)
 *   d(i, j)  = float32 ((dx*dx + dy*dy) + dz*dz), one rounding per operation, no fused multiply-add (the distance of ampnet_knn_f32 and
 *              ampnet_ball_query_f32); coordinates are finite and d does not overflow
 *   idx      [n_clouds, n, k] int32, k = min(3, s): for fine point i the k coarse points with the smallest (d, index), ascending
 *   dist2    [n_clouds, n, k] float32: their d values themselves
 * The usual implementation computes -2 x.y + |x|^2 + |y|^2 as a matrix product and sorts: which of several NEARLY equal neighbours it picks,
 * and the order of exactly equal ones, depends on the library.  Here equal distances go to the lower index, always.                  */
#define AMPNET_THREE_NN_MAX_S 12288
int ampnet_three_nn_f32(const float *fine, int n_clouds, int n, int ld1, const float *coarse, int s, int ld2, int32_t *idx, float *dist2,
                        void *stream);

/* ---- the same search from fine clouds of UNEQUAL size (new symbol within ABI 18: nothing else moved) ------------------------------------
 *   fine        [total, ld1] float32 (first 3 columns used): the fine clouds back to back, cloud b = rows cloud_off[b] .. cloud_off[b + 1]
 *   cloud_off, total, max_n   as in ampnet_ball_query_ragged_f32 (no limit on max_n here)
 *   coarse      [n_clouds, s, ld2] float32: s coarse points for EVERY cloud, 1 <= s <= AMPNET_THREE_NN_MAX_S
 *   idx, dist2  [total, k] int32 / float32, k = min(3, s)
 *   global_index   0: the rows of cloud b are bit for bit the idx and dist2 of ampnet_three_nn_f32 on that cloud alone -- the same distance
 *               form, one lane per fine point, strict `<` insertion, equal distances to the lower index.  1: idx holds b * s + j instead of
 *               j: it addresses coarse as ONE cloud of n_clouds * s points (ampnet_fp_forward_f32 with n_clouds = 1, n = total,
 *               s = n_clouds * s).  dist2 is the same.
 * One launch, grid (ceil(max_n / 256), n_clouds): a workgroup wholly past its cloud's end returns before it stages anything.  The kernel
 * clamps a cloud's length to max_n and skips a cloud whose rows leave [0, total).  Limits (AMPNET_E_ARG): n_clouds <= 65535, s as above. */
int ampnet_three_nn_ragged_f32(const float *fine, int ld1, const int32_t *cloud_off, int n_clouds, int total, int max_n, const float *coarse,
                               int s, int ld2, int global_index, int32_t *idx, float *dist2, void *stream);

/* ---- one feature-propagation layer, eval mode, fused (stands in for PointNetFeaturePropagation.forward of pointnetAtt.py:4,290-292) --
 *   points1               [n_clouds, n, D1] float32 features of the fine points, or NULL with D1 = 0
 *   points2               [n_clouds, s, D2] float32 features of the coarse points, D2 >= 1
 *   idx, dist2            [n_clouds, n, k] the output of ampnet_three_nn_f32, k in {1, 2, 3}, k <= s; indices are clamped into [0, s)
 *   params_host, cout_host, eps_host, workspace   as in ampnet_sa_forward_f32 with cin_0 = D1 + D2; AMPNET_FP_WORKSPACE_BYTES device bytes
 *   out                   [n_clouds, n, cout_{L-1}] float32
 * The input row of fine point i is [points1[i] (D1 values), sum_k w_k points2[idx_k] (D2 values)] -- the column order of the usual
 * cat([points1, interpolated]) -- with w_k = r_k / sum_k r_k, r_k = 1 / (dist2_k + 1e-8f) computed in the kernel (k = 1: weight 1, the
 * usual "repeat" branch for s = 1).  Every layer computes relu(bn_eval(W row + b)), bn_eval folded as in ampnet_sa_forward_f32; the last
 * layer's activations are the output.  Neither the interpolated features, the concatenated rows nor any intermediate activation is
 * written to memory.  Limits (anything else is refused with AMPNET_E_ARG, there is no other path): 1 <= L <= AMPNET_FP_MAX_LAYERS,
 * 1 <= D1 + D2 <= AMPNET_FP_MAX_CIN, every cout_l a multiple of 32 in [32, AMPNET_FP_MAX_COUT].
 * Arithmetic: exact fp32 MFMA (v_mfma_f32_32x32x2_f32) whatever the matrix precision is, as ampnet_sa_forward_f32.                  */
#define AMPNET_FP_MAX_LAYERS 3
#define AMPNET_FP_MAX_CIN 512
#define AMPNET_FP_MAX_COUT 256
#define AMPNET_FP_WORKSPACE_BYTES (AMPNET_FP_MAX_LAYERS * 2 * AMPNET_FP_MAX_COUT * 4)
int ampnet_fp_forward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                          const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                          float *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the two eval forwards with their matrix products in bf16 (inference; added within ABI 17: new symbols, nothing else moved) --------
 * ampnet_sa_forward_bf16 takes the arguments of ampnet_sa_forward_f32 and ampnet_fp_forward_bf16 those of ampnet_fp_forward_f32; inputs
 * and outputs stay float32, and the groups, the neighbours and the interpolation weights are the caller's, as there.  They are entry
 * points of their own: neither ampnet_set_matrix_precision nor a precision scope selects them, and the *_f32 entry points stay exact
 * fp32 whatever the mode is.
 * THE ROUNDING MODEL.  For a row x_0 -- set abstraction: [relative xyz, feats]; feature propagation: [points1, interpolated points2] --
 * formed in fp32 exactly as the *_f32 entry point forms it:
 *   xb_0 = bf16(x_0) and Wb_l = bf16(W_l), round to nearest even, once;
 *   a_l  = sum_k Wb_l[., k] xb_l[k], every product exact and the sum accumulated in fp32 by v_mfma_f32_32x32x16_bf16, k ascending in
 *          blocks of 16 (the contraction padded to a multiple of 16 with zeros).  The order is a function of the shape alone: no atomics,
 *          the same bits run to run;
 *   y_l  = relu(fma(a_l, scale_l, shift_l)) in fp32, scale and shift the folded BatchNorm constants of ampnet_sa_forward_f32;
 *   xb_{l+1} = bf16(y_l); the LAST layer's y stays fp32 and goes to the *_f32 entry point's epilogue: the max over the group's rows (set
 *          abstraction: filler slots and the rows that pad a tile repeat a row of the group and cannot change it), or the store.
 * tests/pn2_bf16_ref.py restates this in float64 with the roundings switchable.
 *   workspace   ampnet_*_forward_bf16_workspace_bytes(..) device bytes, 16-byte aligned: the fold of the *_f32 entry point and behind it
 *               every layer's weights as bf16 rows [cout_l][cin_l padded to 16], written once per call.  The size functions answer on the
 *               host from the shape (D, n_clouds, s, nsample | D1, D2, n_clouds, n) and the widths; 0 = the shape is outside the limits
 *               (ampnet_last_error says which).
 * Limits are those of the *_f32 entry points (AMPNET_E_ARG otherwise, there is no other path).                                        */
size_t ampnet_sa_forward_bf16_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L);
int ampnet_sa_forward_bf16(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                           int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                           const float *eps_host, int L, float *out, void *workspace, size_t workspace_bytes, void *stream);
size_t ampnet_fp_forward_bf16_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L);
int ampnet_fp_forward_bf16(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                           const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                           float *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the backward of ampnet_fp_forward_f32 with BatchNorm's running statistics frozen (decoder fine-tuning) --------------------------
 *   points1 .. eps_host, L   the forward's arguments, unchanged (the forward keeps nothing: the backward recomputes it)
 *   dout                  [n_clouds, n, cout_{L-1}] float32, the gradient of the forward's `out`
 *   dpoints1              [n_clouds, n, D1] out, NULL exactly when D1 = 0
 *   dpoints2              [n_clouds, s, D2] out; the row of a coarse point that is nobody's neighbour is written as zeros
 *   grads_host            HOST array of 4 L DEVICE pointers, per layer: dW [cout_l, cin_l], dbias, dgamma, dbeta (each [cout_l]), all out
 *   workspace             ampnet_fp_backward_workspace_bytes(D1, D2, n_clouds, n, cout_host, L) device bytes (0 = the shape is refused,
 *                         ampnet_last_error says why); contents undefined before and after
 * Per layer l, over the rows i of all clouds, with x_l the layer's input row (x_0 as in the forward), a = W_l x_l,
 * scale = gamma / sqrt(var + eps), y = fma(a, scale, shift) exactly as the forward forms them (so the ReLU mask is the forward's):
 *     dy = dx_{l+1} [y > 0]   (dx_L = dout)          dbeta = sum_i dy          G = sum_i dy a
 *     dgamma = (G + (b - mean) dbeta) / sqrt(var + eps)          dbias = scale dbeta
 *     dz = dy scale          dW_l = dz^T x_l          dx_l = dz W_l
 * dpoints1 = columns [0, D1) of dx_0; dpoints2[j] = sum over the entries (i, q) with idx[i, q] = j (clamped as in the forward) of
 * w_q(i) dx_0[i, D1:], w the forward's interpolation weights.  running_mean and running_var are constants; xyz, dist2 and the weights w
 * get no gradient.  gamma = 0 needs no special case.
 * Summation orders (each a function of the shape alone, so two calls on the same inputs return the same bits; no atomics):
 *   a, y      the forward's: k ascending in blocks of 8, k-step i < 4 of lane half h takes k = k0 + 4 h + i, one fmaf chain per element
 *   dx_l      o ascending in blocks of 8, k-step i < 4 of lane half h takes o = o0 + 2 i + h, one fmaf chain per element
 *   dW_l      the rows in chunks of max(64, ceil(rows / 256) rounded up to 8) rows: inside a chunk one fmaf chain over the rows
 *             in the order k0 + 2 i + h as above, then the chunks' partial sums ascending
 *   dbeta, G  per 32-row tile the rows in the accumulator's order (i & 3) + 8 (i >> 2), i < 16, lane half 0 then + half 1; a workgroup adds
 *             its tiles (tile = workgroup + t * min(tiles, 1024)) ascending; lane t of a wave adds workgroups t, t + 64, .. ascending and
 *             the 64 lane sums go through a halving tree
 *   dpoints2  the entries (i, q) ascending, fmaf(w, dx_0, sum)
 * Limits: the forward's (anything else is refused with AMPNET_E_ARG).  Exact fp32 MFMA whatever the matrix precision is.            */
size_t ampnet_fp_backward_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L);
int ampnet_fp_backward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                           const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                           const float *dout, float *dpoints1, float *dpoints2, float *const *grads_host, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---- ampnet_fp_forward_f32 and its backward with TRAIN-mode BatchNorm: batch statistics (decoder training; new in ABI 13) -------------
 * Forward.  The arguments of ampnet_fp_forward_f32, and:
 *   params_host           per layer W, b, gamma, beta, running_mean, running_var as before; running_mean and running_var are READ AND WRITTEN
 *   momentum              a float in [0, 1] (anything else, NaN included, is refused)
 *   save_mean, save_invstd   [sum_l cout_l] float32 out each, layer l at offset sum_{j<l} cout_j: the batch mean of the raw accumulator
 *                         (WITHOUT the conv bias) and 1 / sqrt(var + eps).  The backward takes them; it never recomputes statistics.
 *   workspace             ampnet_fp_train_forward_workspace_bytes(D1, D2, n_clouds, n, cout_host, L) device bytes (0 = the shape is refused)
 * Per layer l over the M = n_clouds n rows of the call, with a = W x the raw accumulator in the eval forward's contraction order:
 *     mu = mean_rows a      var = mean_rows (a - mu)^2 (biased)      invstd = 1 / sqrt(var + eps)      scale = gamma invstd
 *     shift = fma(-mu, scale, beta)   (the conv bias cancels)      y = fma(a, scale, shift)      x_{l+1} = relu(y)
 *     running_mean <- fma(m, mu + b, (1 - m) running_mean)      running_var <- fma(m, var M / (M - 1), (1 - m) running_var)
 * The variance is CENTRED: per column and 32-row tile the count, the mean and sum (a - tile mean)^2 of the tile's valid rows (rows in
 * the accumulator's order (i & 3) + 8 (i >> 2), i < 16, lane half 0 + half 1); tiles are merged with Chan's formula
 *     n = nA + nB,  d = meanB - meanA,  mean = fma(d, nB / n, meanA),  M2 = fma(d d, nA nB / n, M2A + M2B)
 * first into P = min(tiles, 1024) partial rows (row r: the tiles r, r + P, .. ascending), then over the rows: lane t of a wave merges
 * rows t, t + 64, .. ascending and the 64 lane results go through a halving tree (lane t takes lane t + 32, 16, .. 1).  The last
 * launch is the eval forward's own kernel on the fold (scale, shift) so formed.
 * Backward.  The arguments of ampnet_fp_backward_f32 with, per layer, save_mean_l and save_invstd_l (pointers into the forward's two
 * arrays) in slots 4 and 5 of params_host in place of running_mean and running_var; b (slot 1) is not read.  From dx_L = dout:
 *     dy = dx_{l+1} [y > 0]      dbeta = sum_rows dy      G = sum_rows dy a      dgamma = invstd fma(-mu, dbeta, G)      dbias = 0 (exact zeros)
 *     dz = scale fma(-(a - mu), dgamma invstd / M, dy - dbeta / M)      dW_l = dz^T x_l      dx_l = dz W_l
 * dpoints1, dpoints2, the summation orders of a, dx_l, dW_l, dbeta, G and dpoints2: as in ampnet_fp_backward_f32.
 * Limits and refusals: those of the eval entry points, plus M < 2, M > AMPNET_FP_TRAIN_MAX_ROWS (the statistics carry row counts as
 * floats, exact up to there) and the momentum range (AMPNET_E_ARG).  No float atomics: two calls
 * return the same bits.  Exact fp32 MFMA whatever the matrix precision is.  Caller's stream, no host synchronisation.               */
#define AMPNET_FP_TRAIN_MAX_ROWS (1 << 24)
size_t ampnet_fp_train_forward_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L);
int ampnet_fp_train_forward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                                const float *dist2, int k, float *const *params_host, const int *cout_host, const float *eps_host, int L,
                                float momentum, float *out, float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes,
                                void *stream);
size_t ampnet_fp_train_backward_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L);
int ampnet_fp_train_backward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                                 const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host,
                                 int L, const float *dout, float *dpoints1, float *dpoints2, float *const *grads_host, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* ---- the backward of ampnet_sa_forward_f32 with BatchNorm's running statistics frozen (encoder fine-tuning) --------------------------
 *   xyz .. eps_host, L    the forward's arguments, unchanged (the forward keeps nothing: the backward recomputes it)
 *   dout                  [n_clouds, s, cout_{L-1}] float32, the gradient of the forward's `out`
 *   dfeats                [n_clouds, n, D] out, or NULL when the caller does not want it (layer 0's dx and the gather are then skipped); must
 *                         be NULL when D = 0.  The row of a point that is in no group is written as zeros.
 *   grads_host            HOST array of 4 L DEVICE pointers, per layer: dW [cout_l, cin_l], dbias, dgamma, dbeta (each [cout_l]), all out
 *   arg_out               [n_clouds, s, cout_{L-1}] int32 out, or NULL: the row of the group that the max selected (below)
 *   workspace             ampnet_sa_backward_workspace_bytes(D, n_clouds, s, nsample, cout_host, L) device bytes (0 = the shape is refused,
 *                         ampnet_last_error says why); contents undefined before and after.  It holds x_l and dz_l of all
 *                         M = n_clouds s nsample rows and dx_0's feature columns: 4 M (sum_l (cin_l rounded up to 32) + sum_l cout_l + D)
 *                         bytes -- the M D floats of dx_0 are reserved whether or not dfeats is requested -- plus the split-K partials
 *                         of dW (chunks x the largest cout_l x padded cin_l) and the workgroups' channel sums.
 * Per layer l, over the M rows (g, t), t < nsample, with x_l the layer's input row (x_0 = [xyz[idx_t] - xyz[centre_g], feats[idx_t]] as in the
 * forward), a = W_l x_l and y = fma(a, scale, shift) exactly as the forward forms them, the formulas of ampnet_fp_backward_f32:
 *     dy = dx_{l+1} [y > 0]     dbeta = sum dy     G = sum dy a     dgamma = (G + (b - mean) dbeta) / sqrt(var + eps)     dbias = scale dbeta
 *     dz = dy scale          dW_l = dz^T x_l          dx_l = dz W_l
 * The max over the group: dx_L[(g, t), c] = dout[g, c] for ONE row t = arg(g, c), 0 elsewhere.  arg(g, c) is the lowest t in [0, nsample)
 * whose float32 relu(y) attains the group's maximum (the forward's own bits); the gradient passes only if that y > 0.  Slots that the ball
 * query filled by repeating its first member are bit-identical to that member's row, so their gradient goes to the first occurrence and
 * all their dz and dx are exact zeros.  When every row's y <= 0, arg = 0 and no gradient flows.
 * dfeats[j] = sum over the entries (g, t) with group_idx[g, t] = j (clamped as in the forward) of dx_0[(g, t), 3:]; columns 0 .. 2 of dx_0
 * (the relative coordinates) are dropped: xyz gets no gradient.  running_mean and running_var are constants.
 * Summation orders (each a function of the shape alone, so two calls on the same inputs return the same bits; no atomics):
 *   a, y      the forward's: k ascending in blocks of 8, k-step i < 4 of lane half h takes k = k0 + 2 i + h, one fmaf chain per element
 *   dx_l      o ascending in blocks of 8, k-step i < 4 of lane half h takes o = o0 + 2 i + h, one fmaf chain per element
 *   dW_l      as in ampnet_fp_backward_f32 over the M rows in the order (g, t)
 *   dbeta, G  per group the rows of each 32-row tile in the accumulator's order (i & 3) + 8 (i >> 2), i < 16, tiles ascending, lane half 0
 *             then + half 1 (the last layer: its one term); a workgroup adds its groups (group = workgroup + t * min(groups, 2048))
 *             ascending; lane t of a wave adds workgroups t, t + 64, .. ascending and the 64 lane sums go through a halving tree
 *   dfeats    the entries (g, t) ascending, plain sums
 * Limits: the forward's (nsample <= 64, L <= 3, cin_0 = 3 + D <= 320, widths multiples of 32 up to 256), and a wave's L + 1 tiles of
 * R = 32 (nsample <= 32) or 64 rows -- 4 R (((cin_0 + 7) / 8 * 8 + 1) + sum_l (cout_l + 1)) bytes -- must fit the 160 KB LDS: at R = 32 every
 * such shape does (cin_0 = 320 with three layers of 256: 140 KB), at R = 64 wide stacks do not (the same shape: 280 KB) and are refused
 * by both entry points with AMPNET_E_ARG.  Exact fp32 MFMA whatever the matrix precision is.                                      */
size_t ampnet_sa_backward_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L);
int ampnet_sa_backward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                           int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                           const float *eps_host, int L, const float *dout, float *dfeats, float *const *grads_host, int32_t *arg_out,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ---- set abstraction with ONE group of all n points per cloud (group_all=True of the usual implementation; new in ABI 17) -----------
 * Forward, eval mode.  Row j of cloud b is [xyz[b, j, 0:3], feats[b, j, :]]: the coordinates as they are, no centre (a centre at the origin).
 *   xyz                   [n_clouds, n, ld] float32 (first 3 columns used), n >= 1, n_clouds * n <= 2^31 - 1
 *   feats                 [n_clouds, n, D] float32, or NULL with D = 0
 *   params_host, cout_host, eps_host, L   as in ampnet_sa_forward_f32, cin_0 = 3 + D
 *   out                   [n_clouds, cout_{L-1}] float32: out[b, c] = max_j relu(bn_eval(...)) over the layers
 *   arg_out               [n_clouds, cout_{L-1}] int32 out, or NULL: the LOWEST row j of cloud b whose float32 value attains out[b, c]
 *                         (row 0 when every row's y <= 0), the rule of ampnet_sa_backward_f32's arg_out
 *   workspace             ampnet_sa_all_forward_workspace_bytes(D, n_clouds, n, cout_host, L) device bytes (0 = the shape is refused,
 *                         ampnet_last_error says why); contents undefined before and after.  It holds the BatchNorm fold and, per cloud,
 *                         min(ceil(n / 32), 256) partial rows of cout_{L-1} (max, row) pairs.
 * A wave owns a tile of 32 consecutive rows (rows past n repeat the tile's first row), a cloud's tiles are dealt to at most 256 runs of
 * consecutive tiles, and an ordered reduce combines the runs: ascending rows with a strict > everywhere, no atomics, so two calls return
 * the same bits.  The value of a row is formed exactly as ampnet_sa_forward_f32 forms it (k ascending in blocks of 8, k-step i < 4 of lane
 * half h takes k = k0 + 2 i + h): on the same rows, with a centre at the origin, the two entry points agree bit for bit.
 * Limits (AMPNET_E_ARG otherwise): L <= AMPNET_SA_MAX_LAYERS, cin_0 <= AMPNET_SA_MAX_CIN, every cout_l a multiple of 32 and
 * <= AMPNET_SA_MAX_COUT; every such shape is accepted for every n.  Exact fp32 MFMA whatever the matrix precision is.
 *
 * Backward, BatchNorm's running statistics frozen.
 *   xyz .. eps_host, L    the forward's arguments
 *   arg                   [n_clouds, cout_{L-1}] int32, an INPUT: the forward's arg_out (values are clamped to [0, n))
 *   dout                  [n_clouds, cout_{L-1}] float32
 *   dfeats                [n_clouds, n, D] out, or NULL when it is not wanted; must be NULL when D = 0.  Zero outside the rows in `arg`.
 *   grads_host            as in ampnet_sa_backward_f32: per layer dW, dbias, dgamma, dbeta, all out
 *   workspace             ampnet_sa_all_backward_workspace_bytes(D, n_clouds, n, cout_host, L) device bytes (0 = refused)
 * Only the rows in `arg` carry a gradient (eval BatchNorm is a per-row map): at most cout_{L-1} distinct rows per cloud.  They are sorted
 * into ascending order and compacted into cout_{L-1} / 32 chunks of 32 rows (a chunk is padded by repeating its first member, an empty
 * chunk repeats the cloud's first winner), chunk k gets dout where arg's row lies in chunk k and 0 elsewhere, and the chunks go through
 * ampnet_sa_backward_f32 as groups of nsample = 32 around an all-zero centre: its formulas, summation orders and bits over
 * M = n_clouds * cout_{L-1} rows.  Inside a chunk the recomputed max selects the cloud's winner again (same value, ascending order, the
 * padding repeats an earlier row).  The work after one pass over `arg` does not depend on n, the zero fill of dfeats apart.        */
size_t ampnet_sa_all_forward_workspace_bytes(int D, int n_clouds, int n, const int *cout_host, int L);
int ampnet_sa_all_forward_f32(const float *xyz, int n_clouds, int n, int ld, const float *feats, int D, const float *const *params_host,
                              const int *cout_host, const float *eps_host, int L, float *out, int32_t *arg_out, void *workspace,
                              size_t workspace_bytes, void *stream);
size_t ampnet_sa_all_backward_workspace_bytes(int D, int n_clouds, int n, const int *cout_host, int L);
int ampnet_sa_all_backward_f32(const float *xyz, int n_clouds, int n, int ld, const float *feats, int D, const float *const *params_host,
                               const int *cout_host, const float *eps_host, int L, const int32_t *arg, const float *dout, float *dfeats,
                               float *const *grads_host, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the window token of pointnet_2: one linear layer and a segmented max over clouds of unequal size, fused, with its backward (new
 * symbols within ABI 18: nothing else moved, AMPNET_ABI_VERSION stays 18) -----------------------------------------------------------------
 * Forward.
 *   rows                  [total, cin] float32, point-major, 16-byte aligned: the clouds back to back
 *   cloud_off             [Q + 1] int32 on the DEVICE: cloud q is the rows cloud_off[q] .. cloud_off[q + 1]; cloud_off[0] = 0,
 *                         cloud_off[Q] = total < 2^31, every cloud holds at least one row (the caller's promise: the table is not read back)
 *   W, bias               [cout, cin] (16-byte aligned) and [cout] float32 on the device: nn.Conv1d(cin, cout, 1)'s tensors, squeezed
 *   out                   [Q, cout] float32: out[q, c] = max over the rows r of cloud q of y[r, c] = (W[c, :] . rows[r, :]) + bias[c].
 *                         No BatchNorm, no ReLU: a maximum below zero stays below zero, the running maximum starts from a row's value
 *   arg_out               [Q, cout] int32, or NULL: the index INSIDE cloud q of the LOWEST row whose float32 value attains out[q, c], the
 *                         rule of ampnet_sa_all_forward_f32
 *   workspace             ampnet_token_pool_forward_workspace_bytes(cin, cout, Q, total) device bytes, 16-byte aligned (0 = the shape is
 *                         refused, ampnet_last_error says why); contents undefined before and after
 * Every element of out and arg_out is written.  Non-finite inputs are out of contract.
 * The value of a row: exact fp32 on v_mfma_f32_32x32x2_f32, whatever the matrix precision is -- neither ampnet_set_matrix_precision nor a
 * precision scope is consulted.  The accumulator starts at 0 and takes the products rows[r, k] W[c, k] one fused multiply-add at a time, k
 * in blocks of 8 from 0 upwards and inside a block in the order k0 + 0, + 4, + 1, + 5, + 2, + 6, + 3, + 7 (k-step i < 4 of lane half h takes
 * k = k0 + 4 h + i, a lane's four weights are 16 contiguous bytes); the bias is added last, one float32 add.  The value is a function of
 * the row's cin numbers and the weights alone: it does not depend on the row's place in its tile, on its cloud or on the launch.  So the
 * same rows cut into other clouds give the same y, equal rows tie exactly, and the lowest wins.
 * Work: a cloud of n rows owns ceil(n / 32) tiles of 32 consecutive rows (a tile never mixes two clouds; the rows past n repeat the tile's
 * first row).  The tiles of all clouds, in order, are cut into items of G consecutive tiles, G = ceil(ceil((total + 31 Q) / 32) / 4096); a
 * wave finds an item's first cloud by bisection of the tile prefix sums (computed on the device from cloud_off) and walks its tiles, cloud
 * after cloud.  A cloud that lies inside one item is finished there; the runs of a cloud that spans several items go as (max, row)
 * partials to the workspace, and an ordered reduce combines them: ascending rows with a strict > everywhere, no atomics, so two calls
 * return the same bits.  The weights are staged in LDS once per workgroup when they fit beside the four waves' tiles
 * (4 (cin + 1) (128 + cout) <= 160 KB: 128 x 128 does, 256 x 256 does not and is read through L2).
 * Limits (AMPNET_E_ARG otherwise, the message names the entry point and the value): cin and cout multiples of 32 in [32, 256], Q >= 1,
 * Q <= total <= 2^31 - 1, Q cout <= 2^31 - 1.
 *
 * Backward.
 *   rows, cloud_off, Q, total, W, cin, cout   the forward's arguments
 *   arg                   [Q, cout] int32, an INPUT: the forward's arg_out (values are clamped into their cloud)
 *   dout                  [Q, cout] float32
 *   dx                    [total, cin] out, or NULL: EVERY element is written, zero outside the winners;
 *                         dx[cloud q's row r, k] = sum over the channels c with arg[q, c] = r, ascending c, of dout[q, c] W[c, k]
 *   dW                    [cout, cin] out, or NULL: dW[c, k] = sum over q ascending of dout[q, c] rows[cloud q's row arg[q, c], k]
 *   db                    [cout] out, or NULL: db[c] = sum over q ascending of dout[q, c]
 *   workspace             ampnet_token_pool_backward_workspace_bytes(cin, cout, Q, total) device bytes (0 = refused)
 * float32 accumulators: dx and dW are fmaf chains from 0 in the stated order, db plain float32 adds.  No atomics: two calls return the same
 * bits.  Apart from the zero fill of dx the work is O(Q cout cin) whatever total is.  Tie rule: the LOWEST row takes the whole
 * gradient, where torch.amax's backward splits it evenly among equal maxima; equal maxima arise from exact duplicate rows (cyclic
 * padding), and there both rules give the same dW and db.                                                                           */
size_t ampnet_token_pool_forward_workspace_bytes(int cin, int cout, int Q, long long total);
int ampnet_token_pool_forward_f32(const float *rows, const int32_t *cloud_off, int Q, long long total, const float *W, const float *bias,
                                  int cin, int cout, float *out, int32_t *arg_out, void *workspace, size_t workspace_bytes, void *stream);
size_t ampnet_token_pool_backward_workspace_bytes(int cin, int cout, int Q, long long total);
int ampnet_token_pool_backward_f32(const float *rows, const int32_t *cloud_off, int Q, long long total, const float *W, int cin, int cout,
                                   const int32_t *arg, const float *dout, float *dx, float *dW, float *db, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ---- ampnet_sa_forward_f32 and its backward with TRAIN-mode BatchNorm: batch statistics (encoder training; new in ABI 14) -------------
 * Forward.  The arguments of ampnet_sa_forward_f32, and (as in ampnet_fp_train_forward_f32):
 *   params_host           per layer W, b, gamma, beta, running_mean, running_var as before; running_mean and running_var are READ AND WRITTEN
 *   momentum              a float in [0, 1] (anything else, NaN included, is refused)
 *   save_mean, save_invstd   [sum_l cout_l] float32 out each, layer l at offset sum_{j<l} cout_j: the batch mean of the raw accumulator
 *                         (WITHOUT the conv bias) and 1 / sqrt(var + eps).  The backward takes them; it never recomputes statistics.
 *   workspace             ampnet_sa_train_forward_workspace_bytes(D, n_clouds, s, nsample, cout_host, L) device bytes (0 = the shape is
 *                         refused): the fold and min(n_clouds s, 1024) partial rows of 3 max_l cout_l floats, whatever M is
 * Rows.  M = n_clouds s nsample; the rows (g, t), t < nsample, are those of the eval forward.  A slot that ball query filled by repeating
 * its first member is a row like any other: it enters the statistics, it gets a (generally nonzero) dz from the correction terms below and
 * it contributes to dW and dfeats -- what BatchNorm2d over [B, C, nsample, npoint] does.  The rows t >= nsample that pad a group to 32 or 64
 * enter nothing.
 * Per layer l over the M rows, with a = W x the raw accumulator in the eval forward's contraction order (k ascending in blocks of 8, k-step
 * i < 4 of lane half h takes k = k0 + 2 i + h, one fmaf chain per element), the formulas of ampnet_fp_train_forward_f32:
 *     mu = mean_rows a      var = mean_rows (a - mu)^2 (biased)      invstd = 1 / sqrt(var + eps)      scale = gamma invstd
 *     shift = fma(-mu, scale, beta)   (the conv bias cancels)      y = fma(a, scale, shift)      x_{l+1} = relu(y)
 *     running_mean <- fma(m, mu + b, (1 - m) running_mean)      running_var <- fma(m, var M / (M - 1), (1 - m) running_var)
 * The variance is CENTRED: per column, group and 32-row tile of the group the count, the mean and sum (a - tile mean)^2 of the tile's rows
 * t < nsample (rows in the accumulator's order (i & 3) + 8 (i >> 2), i < 16, lane half 0 + half 1); they are merged with Chan's formula
 * (ampnet_fp_train_forward_f32) first into P = min(groups, 1024) partial rows (row r: the groups r, r + P, .. ascending, a group's tiles
 * ascending), then over the rows: lane t of a wave merges rows t, t + 64, .. ascending and the 64 lane results go through a halving tree
 * (lane t takes lane t + 32, 16, .. 1).  Pass l recomputes layers < l from the inputs; no activation is written to memory.  The last
 * launch is the eval forward's own kernel on the fold (scale, shift) so formed: `out` is the max of what the statistics were taken from.
 * Backward.  The arguments of ampnet_sa_backward_f32 with, per layer, save_mean_l and save_invstd_l (pointers into the forward's two
 * arrays) in slots 4 and 5 of params_host in place of running_mean and running_var; b (slot 1) is not read.  scale and shift are rebuilt
 * from them by the forward's two operations (the same bits).
 *   arg(g, c)  the lowest t in [0, nsample) whose float32 relu(y) attains the group's maximum, y = fma(a, scale, shift); written to arg_out
 *              (may be NULL).  dx_L[(g, t), c] = dout[g, c] at t = arg(g, c), 0 elsewhere.
 *     dy = dx_{l+1} [y > 0]      dbeta = sum_rows dy      G = sum_rows dy a      dgamma = invstd fma(-mu, dbeta, G)      dbias = 0 (exact zeros)
 *     dz = scale fma(-(a - mu), dgamma invstd / M, dy - dbeta / M)   for EVERY row t < nsample      dW_l = dz^T x_l      dx_l = dz W_l
 * dfeats is the ordered gather of dx_0[:, 3:] as in ampnet_sa_backward_f32; xyz gets no gradient.  dz_l needs the sums over all rows, so
 * the backward is L + 1 phases with a finalize between them; the last layer's dy is kept as arg plus dout, never as a dense array.
 * Summation orders: a, y, dx_l, dW_l and dfeats as in ampnet_sa_backward_f32;
 *   dbeta, G  the last layer: one term dout[g, c] (times a at arg) per group; the other layers: per 32-row tile (g, m) the rows in the
 *             accumulator's order, lane half 0 then + half 1.  A workgroup adds its groups (the last layer) or tiles (tile = 2 g + m at
 *             nsample > 32, else g) w, w + P, .. ascending, P = min(groups, 2048); lane t of a wave adds workgroups t, t + 64, ..
 *             ascending and the 64 lane sums go through a halving tree
 * Workspace of the backward: ampnet_sa_train_backward_workspace_bytes(...) device bytes -- the layout of ampnet_sa_backward_f32 (x_l and dz_l
 * of all M rows, dx_0's feature columns, the split-K partials, the channel sums), then 2 sum_l cout_l coefficients and the n_clouds s
 * cout_{L-1} int32 of arg.
 * Limits and refusals (all four entry points, AMPNET_E_ARG with a sentence): those of ampnet_sa_forward_f32 and of ampnet_sa_backward_f32,
 * its 64-row LDS limit included (a shape that trains has a backward), plus M < 2, M > AMPNET_SA_TRAIN_MAX_ROWS (the statistics carry row
 * counts as floats, exact up to there), the momentum range and a short workspace.  No float atomics: two calls return the same bits.  Exact
 * fp32 MFMA whatever the matrix precision is.  Caller's stream, no host synchronisation.                                              */
#define AMPNET_SA_TRAIN_MAX_ROWS (1 << 24)
size_t ampnet_sa_train_forward_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L);
int ampnet_sa_train_forward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                                int nsample, const float *feats, int D, float *const *params_host, const int *cout_host,
                                const float *eps_host, int L, float momentum, float *out, float *save_mean, float *save_invstd,
                                void *workspace, size_t workspace_bytes, void *stream);
size_t ampnet_sa_train_backward_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L);
int ampnet_sa_train_backward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                                 int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                                 const float *eps_host, int L, const float *dout, float *dfeats, float *const *grads_host, int32_t *arg_out,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ---- the four backwards above on clouds of UNEQUAL size packed back to back (new symbols within ABI 18: nothing else moved,
 * AMPNET_ABI_VERSION stays 18).  Training and fine-tuning on clouds of native size: the ragged searches (ampnet_fps_ragged_f32,
 * ampnet_ball_query_ragged_f32 and ampnet_three_nn_ragged_f32 with global_index = 1) give centres, groups and neighbours as rows of the
 * packed array, and the forwards -- ampnet_sa_forward_f32, ampnet_fp_forward_f32 and their _train_ namesakes -- take that array as ONE
 * cloud (n_clouds = 1, n = total, n_clouds * s centres or coarse points): no row of theirs mixes with another, and batch statistics over
 * all rows of the call are the right statistics.  These are their backwards.  Each takes the argument list of its uniform namesake with
 * (n_clouds, n) replaced by
 *   cloud_off             DEVICE int32 [n_clouds + 1], ascending, cloud_off[0] = 0, cloud_off[n_clouds] = total (the table of
 *                         ampnet_fps_ragged_f32): cloud b is the rows cloud_off[b] .. cloud_off[b + 1] - 1 of the packed arrays
 *   n_clouds, total       the clouds and the rows of all of them
 * and s PER CLOUD: points2 / dpoints2 are [n_clouds * s, D2] with the coarse points of cloud b at [b s, (b + 1) s); centres, group_idx,
 * dout and arg_out of the set abstraction are [n_clouds * s, ..] in the same order.  idx (feature propagation), centres and group_idx
 * (set abstraction) hold GLOBAL rows: of the n_clouds * s coarse points, of the `total` points.
 * Each runs exactly the phases of its namesake on the packed array as one cloud -- so dpoints1, dW, dbias, dgamma, dbeta and arg_out are
 * that call's, bit for bit -- and only the last gather is segmented by cloud_off:
 *   dpoints2   one wave per coarse point j of cloud b = j / s scans the entries (i, q) of the fine rows i of cloud b alone, ascending,
 *              idx clamped into [b s, (b + 1) s - 1], fmaf(w, dx_0, sum)
 *   dfeats     one wave per point j; its cloud b (a binary search over cloud_off) has the centres [b s, (b + 1) s), and the wave scans
 *              their s nsample entries alone, ascending, clamped into the cloud's rows, plain sums
 * instead of the entries of the whole array, whose number grows with n_clouds for every one of the n_clouds * s (or total) waves.
 * Cloud by cloud, dpoints2 and dfeats are the bits the uniform entry point writes for that cloud alone (n_clouds = 1, local indices).
 * PRECONDITION: every index refers to a point, centre or coarse point of ITS OWN cloud, as the indices of the ragged searches do.  The
 * phases before the gather clamp an index into the whole packed array, the gather into the cloud: the two disagree only for an index that
 * violates the precondition (nothing is read or written out of bounds either way; the table's rows are clamped into [0, total]).
 * Workspace: the existing *_workspace_bytes functions called with the packed shape -- ampnet_fp_backward_workspace_bytes(D1, D2, 1,
 * total, ..) / ampnet_fp_train_backward_workspace_bytes likewise; ampnet_sa_backward_workspace_bytes(D, 1, n_clouds * s, nsample, ..) /
 * ampnet_sa_train_backward_workspace_bytes likewise -- and the layout is theirs.  Limits: those of the namesakes on the packed shape, so
 * total <= AMPNET_FP_TRAIN_MAX_ROWS and n_clouds * s * nsample <= AMPNET_SA_TRAIN_MAX_ROWS for the train-mode pair, k <= s, and
 * n_clouds * s <= 2^31 - 1.  No float atomics, every order a function of the shape and the table alone: two calls return the same bits.
 * Caller's stream, no host synchronisation.                                                                                         */
int ampnet_fp_backward_ragged_f32(const float *points1, int D1, const float *points2, int D2, const int32_t *cloud_off, int n_clouds, int total,
                                  int s, const int32_t *idx, const float *dist2, int k, const float *const *params_host, const int *cout_host,
                                  const float *eps_host, int L, const float *dout, float *dpoints1, float *dpoints2, float *const *grads_host,
                                  void *workspace, size_t workspace_bytes, void *stream);
int ampnet_fp_train_backward_ragged_f32(const float *points1, int D1, const float *points2, int D2, const int32_t *cloud_off, int n_clouds,
                                        int total, int s, const int32_t *idx, const float *dist2, int k, const float *const *params_host,
                                        const int *cout_host, const float *eps_host, int L, const float *dout, float *dpoints1,
                                        float *dpoints2, float *const *grads_host, void *workspace, size_t workspace_bytes, void *stream);
int ampnet_sa_backward_ragged_f32(const float *xyz, const int32_t *cloud_off, int n_clouds, int total, int ld, const int32_t *centres, int s,
                                  const int32_t *group_idx, int nsample, const float *feats, int D, const float *const *params_host,
                                  const int *cout_host, const float *eps_host, int L, const float *dout, float *dfeats,
                                  float *const *grads_host, int32_t *arg_out, void *workspace, size_t workspace_bytes, void *stream);
int ampnet_sa_train_backward_ragged_f32(const float *xyz, const int32_t *cloud_off, int n_clouds, int total, int ld, const int32_t *centres,
                                        int s, const int32_t *group_idx, int nsample, const float *feats, int D,
                                        const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                                        const float *dout, float *dfeats, float *const *grads_host, int32_t *arg_out, void *workspace,
                                        size_t workspace_bytes, void *stream);

/* ---- the per-point classifier of the PointNet++ segmentation model, eval mode, fused, and its backward (added within ABI 17: new
 * symbols, nothing else moved).  Stands in for the lines the reference's pointnet_2 carries commented out (pointnetAtt.py:294-296,
 * :318-321): bn1, drop1 (the identity in eval mode), conv2, log_softmax, permute.
 *   x            [M][ld] float32 rows, the first cin columns used, ld >= cin.  The rows are a flat list: the head has no per-cloud structure
 *   params_host  HOST array of 8 DEVICE pointers: W1 [hidden][cin], b1, gamma, beta, running_mean, running_var (each [hidden]),
 *                W2 [n_classes][hidden], b2 [n_classes]
 *   eps          BatchNorm's
 *   logp         [M][n_classes] float32 out, dense
 *   preds        [M] int64 out (what ampnet_confusion_i64 takes), or NULL
 * Arithmetic, per row x:
 *     a      = W1 x                                       cin ascending in blocks of 8 (padded with zeros), k-step i < 4 of lane half h takes k = k0 + 4 h + i,
 *                                                         one fmaf chain per element (the order of ampnet_fp_forward_f32)
 *     h      = relu(fma(a, scale, shift))                 scale = gamma / sqrt(var + eps), shift = (b1 - mean) * scale + beta: the fold of
 *                                                         ampnet_sa_forward_f32
 *     z      = W2 h + b2                                  the same contraction order over hidden, then one addition; no BatchNorm, no ReLU
 *     logp_c = (z_c - m) - logf(S)                        m = max_c z_c,  S = sum over c ascending of expf(z_c - m)
 *     pred   = the LOWEST c with z_c == m
 * expf and logf are the accurate library functions (tests/head_probe.py measures them).  Neither h nor z is written to memory.  The
 * summation orders are functions of the shape alone: the same bits run to run.
 * Backward, running_mean and running_var frozen, the forward keeps nothing.  dlogp [M][n_classes] is ANY upstream gradient g:
 *     dz_c = fma(-expf(logp_c), sum over j ascending of g_j, g_c)        logp recomputed by the forward's own code: the forward's bits
 *     db2  = sum_rows dz          dW2 = dz^T h          dh = dz W2
 *     dy = dh [y > 0],  dbeta = sum_rows dy,  G = sum_rows dy a,  dgamma = (G + (b1 - mean) dbeta) / sqrt(var + eps),  db1 = scale dbeta,
 *     dz1 = dy scale,  dW1 = dz1^T x,  dx = dz1 W1          one layer of ampnet_fp_backward_f32, with its summation orders
 *   dx           [M][cin] float32 out, dense, or NULL: not wanted
 *   grads_host   HOST array of 6 DEVICE pointers, all out: dW1 [hidden][cin], db1, dgamma, dbeta (each [hidden]), dW2 [n_classes][hidden],
 *                db2 [n_classes]
 *   db2          per 32-row tile the rows ascending; a workgroup adds its tiles (tile = workgroup + t * min(tiles, 1024)) ascending; lane t
 *                of a wave adds workgroups t, t + 64, .. ascending and the 64 lane sums go through a halving tree
 *   dW2, dh      as dW_l and dx_l of ampnet_fp_backward_f32 with the class dimension padded to 32 by zeros
 * No float atomics anywhere: two calls on the same inputs return the same bits.
 * Workspaces (contents undefined before and after; the size functions answer on the host, 0 = the shape is refused and ampnet_last_error
 * says why).  Forward: the fold, scale [hidden] then shift [hidden].  Backward: the fold; the layout of ampnet_fp_backward_f32 for ONE layer
 * cin -> hidden (the workgroups' partial sums, the rows x padded to a multiple of 32 columns, dz1 [M][hidden], the split-K partials of
 * dW); then h [M][hidden], dz [M][32], the workgroups' partial sums of dz [min(tiles, 1024)][32] and dW2 as [32][hidden], of which the
 * first n_classes rows are copied to the caller's.
 * Limits (anything else is refused with AMPNET_E_ARG on the host before any launch, there is no other path): 1 <= cin <=
 * AMPNET_SEG_HEAD_MAX_CIN, hidden a multiple of 32 in [32, AMPNET_SEG_HEAD_MAX_HIDDEN], 2 <= n_classes <= AMPNET_SEG_HEAD_MAX_CLASSES (one
 * MFMA column tile), 1 <= M <= AMPNET_SEG_HEAD_MAX_ROWS (a wave's tile counter stays inside an int).  Exact fp32 MFMA
 * (v_mfma_f32_32x32x2_f32) whatever the matrix precision is.
 * NOT BUILT: bf16, a fused loss (nll_loss on [M][C] is a small operation of the caller's).  Train-mode bn1 and dropout are the
 * _train_ entry points below; these two stay eval mode (drop1 the identity).                                                        */
#define AMPNET_SEG_HEAD_MAX_CIN 256
#define AMPNET_SEG_HEAD_MAX_HIDDEN 256
#define AMPNET_SEG_HEAD_MAX_CLASSES 32
#define AMPNET_SEG_HEAD_MAX_ROWS (0x7fff0000LL * 32)
size_t ampnet_seg_head_forward_workspace_bytes(int cin, int hidden, int n_classes, long long M);
int ampnet_seg_head_forward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes, const float *const *params_host,
                                float eps, float *logp, long long *preds, void *workspace, size_t workspace_bytes, void *stream);
size_t ampnet_seg_head_backward_workspace_bytes(int cin, int hidden, int n_classes, long long M);
int ampnet_seg_head_backward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes, const float *const *params_host,
                                 float eps, const float *dlogp, float *dx, float *const *grads_host, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* ---- the segmentation head in TRAIN mode: bn1 on batch statistics, drop1 a real dropout (new within ABI 18) ---------------------------
 * Forward.  The arguments of ampnet_seg_head_forward_f32 without preds (predict is an eval operation), and:
 *   params_host           the 8 pointers as before; running_mean and running_var (slots 4, 5) are READ AND WRITTEN
 *   momentum              a float in [0, 1] (anything else, NaN included, is refused)
 *   drop_p, seed          dropout of conv1's activations: 0 <= drop_p < 1 (anything else, NaN included, is refused); seed selects the mask
 *   save_mean, save_invstd   [hidden] float32 out each: the batch mean of the raw accumulator (WITHOUT b1) and 1 / sqrt(var + eps).  The
 *                         backward takes them; it never recomputes statistics.
 *   workspace             ampnet_seg_head_train_forward_workspace_bytes(cin, hidden, n_classes, M) device bytes (0 = the shape is refused):
 *                         the fold, then min(tiles, 1024) partial rows of 3 hidden floats
 * Over the M rows, with a = W1 x the raw accumulator in the eval forward's contraction order, the formulas of ampnet_fp_train_forward_f32:
 *     mu = mean_rows a      var = mean_rows (a - mu)^2 (biased)      invstd = 1 / sqrt(var + eps)      scale = gamma invstd
 *     shift = fma(-mu, scale, beta)   (b1 cancels)      y = fma(a, scale, shift)      h = relu(y)
 *     running_mean <- fma(m, mu + b1, (1 - m) running_mean)      running_var <- fma(m, var M / (M - 1), (1 - m) running_var)
 *     hd[r, c] = keep(r hidden + c) ? h dscale : 0      keep(i) = mix32(i ^ drop_base(seed, 0)) >= drop_threshold(drop_p)
 *     dscale = 1.0f / (1.0f - drop_p)      (the package's counter hash, restated in oracle/ampnet_oracle.py::keep_mask; drop_p == 0 hashes
 *     nothing and is the identity)
 *     z = W2 hd + b2      logp = log_softmax(z)      as in ampnet_seg_head_forward_f32
 * The statistics are centred and merged exactly as ampnet_fp_train_forward_f32 states: per column and 32-row tile the count, mean and
 * sum (a - tile mean)^2 of the valid rows, Chan's merge first into P = min(tiles, 1024) partial rows (row r: the tiles r, r + P, ..
 * ascending), then over the rows (lane t of a wave the rows t, t + 64, .. ascending, then a halving tree).  The last launch is the eval
 * forward's own kernel on the fold so formed, with the dropout applied to h in LDS between conv1 and conv2.
 * Backward.  The arguments of ampnet_seg_head_backward_f32 with drop_p, seed, save_mean and save_invstd as the forward had them;
 * running_mean, running_var and b1 are not read.  From g = dlogp:
 *     dz, db2 = sum_rows dz, dW2 = dz^T hd, dh = dz W2      as in ampnet_seg_head_backward_f32 (logp and hd recomputed: the forward's bits)
 *     dh' = keep ? dh dscale : 0      dy = dh' [y > 0]      dbeta = sum_rows dy      G = sum_rows dy a
 *     dgamma = invstd fma(-mu, dbeta, G)      db1 = 0 (exact zeros, written)
 *     dz1 = scale fma(-(a - mu), dgamma invstd / M, dy - dbeta / M)      dW1 = dz1^T x      dx = dz1 W1
 * with the summation orders of ampnet_fp_train_backward_f32 and ampnet_seg_head_backward_f32.  Workspace:
 * ampnet_seg_head_train_backward_workspace_bytes(...) device bytes: the eval backward's layout, then the two coefficients per channel.
 * Limits and refusals (AMPNET_E_ARG on the host before any launch): those of the eval entry points, plus M < 2,
 * M > AMPNET_SEG_HEAD_TRAIN_MAX_ROWS (the statistics carry row counts as floats, exact up to there; M hidden then fits the 32-bit dropout
 * counter), drop_p outside [0, 1), momentum outside [0, 1], null pointers and a short workspace.  No float atomics: two calls return the
 * same bits.  Exact fp32 MFMA whatever the matrix precision is.  Caller's stream, no host synchronisation.
 * NOT BUILT: bf16, a fused loss, momentum = None (the cumulative average), dropout in eval mode.                                     */
#define AMPNET_SEG_HEAD_TRAIN_MAX_ROWS (1 << 24)
size_t ampnet_seg_head_train_forward_workspace_bytes(int cin, int hidden, int n_classes, long long M);
int ampnet_seg_head_train_forward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes, float *const *params_host,
                                      float eps, float momentum, float drop_p, uint32_t seed, float *logp, float *save_mean,
                                      float *save_invstd, void *workspace, size_t workspace_bytes, void *stream);
size_t ampnet_seg_head_train_backward_workspace_bytes(int cin, int hidden, int n_classes, long long M);
int ampnet_seg_head_train_backward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes,
                                       const float *const *params_host, float eps, float drop_p, uint32_t seed, const float *save_mean,
                                       const float *save_invstd, const float *dlogp, float *dx, float *const *grads_host, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* ---- the loss behind the segmentation head: masked, weighted NLL with predictions and confusion counts (new symbols within ABI 18:
 * nothing else moved, AMPNET_ABI_VERSION stays 18) ---------------------------------------------------------------------------------------
 * One pass over the log-probabilities the head wrote, where the composition nll_loss + argmax + ampnet_confusion_i64 takes about eight
 * launches over the same array.  The loss is NOT fused into the head's kernel: logp is read from memory.
 *   logp      [M][C] float32, dense                      target   [M] int64
 *   class_w   [C] float32 device, or NULL = ones
 *   sums      [2] float64 device out: sum over the live rows of w[t] * -logp[m][t], and of w[t]
 *   loss      [1] float32 device out: (float)(sums[0] / sums[1])
 *   preds     [M] int64 out, or NULL                      counts   [C * C + 1] int64 out, or NULL
 * Ignored rows.  A row whose target lies outside [0, C) is ignored; -1 is the padding label and the ONLY such value the package's drivers
 * produce.  An ignored row adds nothing to sums and gets a zero row of dlogp; it still gets a prediction and is counted in counts[C * C].
 * This is torch's nll_loss(weight, ignore_index=-1, reduction='mean') on the drivers' targets; with every row ignored the loss is 0 / 0 = NaN
 * and dlogp is all zeros, as in torch.
 *   preds[m]  the LOWEST class among the equal largest logp[m][:] (the head's own rule, what ampnet_confusion_i64 takes)
 *   counts    the layout of ampnet_confusion_i64: counts[t * C + p] over the live rows, counts[C * C] the ignored rows.  The entry point
 *             zero-fills it on the stream; a workgroup counts in an int32 LDS table and adds its non-zero cells with integer atomics.
 * Summation: float64 throughout.  256-thread workgroups, grid = min(cdiv(M, 256), 1024), thread `i` of workgroup `g` takes the rows
 * 256 g + i + 256 grid k, k ascending; a wave adds its 64 lanes by a butterfly of shuffles (xor 32, 16, .. 1), thread 0 adds the four waves
 * ascending, the workgroup writes one double[2] row of the workspace, and a one-workgroup kernel adds the rows ascending.  w[t] * -logp is
 * exact in float64 (two float32 factors).  Every order is a function of (M, C) alone: two calls return the same bits.  No float atomics.
 *   workspace ampnet_seg_nll_forward_workspace_bytes(M) device bytes (0 = M is refused), aligned to 8: the workgroups' partial rows
 * Backward, for the upstream gradient g = grad_loss[0] (DEVICE memory: no host synchronisation):
 *     dlogp[m][t] = (float)(-(w[t] * g) / sums[1])      the float64 quotient rounded once, within half a float32 ulp;      0 elsewhere
 * (the float32 statement -(w[t] * g) / (float)sums[1] rounds sums[1], the product and the quotient and can land 2.5 ulp away; the C
 * values a row can take are formed once per workgroup, so the float64 divisions cost nothing that shows).
 * One thread per row writes all C values of its row: dlogp may be uninitialised memory.
 * Limits (AMPNET_E_ARG on the host before any launch): 2 <= C <= AMPNET_SEG_HEAD_MAX_CLASSES, 1 <= M <= AMPNET_SEG_HEAD_MAX_ROWS, null
 * pointers, a short or misaligned workspace.  The pass moves 4 M C bytes and is bound by its launches.  Caller's stream.               */
size_t ampnet_seg_nll_forward_workspace_bytes(long long M);
int ampnet_seg_nll_forward_f32(const float *logp, long long M, int C, const long long *target, const float *class_w, double *sums, float *loss,
                               long long *preds, long long *counts, void *workspace, size_t workspace_bytes, void *stream);
int ampnet_seg_nll_backward_f32(const long long *target, const float *class_w, const double *sums, const float *grad_loss, long long M, int C,
                                float *dlogp, void *stream);

/* ---- size-constrained k-means: the window grouping step in front of the path --------------------------
 * replaces the calls of the third-party k_means_constrained.KMeansConstrained at data_proc/3_kmeans.py:78-82 (size_min = size_max =
 * n_points, n_init 5, max_iter 10, tol 1e-2, features x, y, NDVI) and utils/utils.py:500-505 (size_min only).  That package is not part
 * of the reference repository: parity is UNPINNED; the algorithm below is this build's spec (csrc/kmeans.hip, oracle/kmeans_oracle.py):
 * farthest-point seeding, greedy capacity-constrained assignment in ascending (distance, point, cluster) order (every cluster first gets
 * size_min points, the rest go where capacity size_max allows), means, stop at centre shift <= tol * mean feature variance, best of n_init.
 *   feat     [n, 3] float32 device     labels  [n] int32 out     centres [k, 3] float32 out     inertia: device double out (may be NULL)
 *   1 <= k <= 32, k <= n <= 65536, size_min * k <= n <= size_max * k                                                                   */
size_t ampnet_kmeans_workspace_bytes(int n, int k);
int ampnet_kmeans_balanced_f32(const float *feat, int n, int k, int size_min, int size_max, int n_init, int max_iter, float tol,
                               uint32_t seed, int32_t *labels, float *centres, double *inertia, void *workspace, size_t workspace_bytes,
                               void *stream);

/* ---- global-batch BatchNorm under data parallelism (process-wide; SURVEY section 8(e) option A) ---------------------------------
 * The reference is single-device: its BatchNorm layers see the whole batch.  With a collective registered and world_size > 1,
 * every TRAIN-mode BatchNorm inside ampnet_encoder_fwd_f32 / _bwd_f32, ampnet_head_* and ampnet_gru_head_* uses the statistics of the
 * global batch: the forward all-gathers the per-slot (rows, mean, M2) of every rank and merges them (Chan), the backward all-reduces
 * the per-slot (sum dy, sum dy zhat, rows).  Running statistics are then identical on every rank.  A slot that holds no row on any rank
 * gets mean 0, variance 0 in the forward and P2 = P3 = 0 (dz = P1 dy) in the backward, as without a collective.  The library calls `fn`
 * on the host, between two launches:
 *   op AMPNET_COLLECTIVE_ALLGATHER      recv[k * n_floats .. ] = rank k's send[0 .. n_floats)      (recv holds world_size * n_floats)
 *   op AMPNET_COLLECTIVE_ALLREDUCE_SUM  send == recv: element-wise float32 sum over the ranks, in place
 * send / recv point into `scratch` (device memory of ampnet_collective_scratch_bytes(world_size) bytes the caller owns and keeps
 * alive); the exchange must be ordered after the work already enqueued on `stream` and before what is enqueued after fn returns
 * (torch.distributed on the current stream does that).  fn returns 0 on success.  fn = NULL switches back to per-rank statistics.
 * 18 + 18 latency-bound collectives per AMP-Net step: off by default (per-rank BatchNorm is the documented deviation).
 *
 * The six PointNet++ train entry points -- ampnet_fp_train_forward_f32 / ampnet_fp_train_backward_f32, ampnet_sa_train_forward_f32 /
 * ampnet_sa_train_backward_f32, ampnet_seg_head_train_forward_f32 / ampnet_seg_head_train_backward_f32 -- and their ragged namesakes
 * (ampnet_fp_train_backward_ragged_f32, ampnet_sa_train_backward_ragged_f32) follow a registered collective too, whatever world_size
 * is.  Per BatchNorm layer:
 *   forward   the rank's rows give ONE row (n_r, mean_r, M2_r)[cout]; one AMPNET_COLLECTIVE_ALLGATHER of 3 cout floats; every rank merges the
 *             world_size rows in rank order (Chan) into (n, mean, M2) and uses var = M2 / n, running_var's M2 / (n - 1) with the MERGED
 *             row count n = sum_r n_r -- the ranks may hold different numbers of rows.  scale, shift, save_mean, save_invstd and the running
 *             statistics come out the same on every rank, bit for bit.
 *   backward  dbeta = sum dy, dgamma = invstd (sum dy a - mean sum dy) and dbias = 0 are written from the RANK's sums (the caller's gradient
 *             all-reduce adds them up like every other parameter gradient); one AMPNET_COLLECTIVE_ALLREDUCE_SUM of (sum dy, sum dy a)[cout]
 *             and the rank's row count, 2 cout + 1 floats; the input gradient then uses the coefficients sum dy / n and
 *             dgamma_global invstd / n with dgamma_global = invstd (G - mean sum dy) on the global sums.
 * One exchange per BatchNorm layer and direction whatever the data (17 + 17 per step of pointnet_2_seg): every rank must make the same
 * sequence of calls.  A callback that fails ends the call with AMPNET_E_LAUNCH; nothing waits or retries.  With world_size 1 every exchange
 * is the identity and the results are those without a collective, bit for bit.  Row counts are carried as floats: with a collective
 * registered these entry points also refuse M * world_size above their AMPNET_*_TRAIN_MAX_ROWS -- a host-side rule, conservative because the
 * ranks' row counts differ and no rank knows the others'.  No new symbol: AMPNET_ABI_VERSION stays 18.                               */
#define AMPNET_COLLECTIVE_ALLGATHER 0
#define AMPNET_COLLECTIVE_ALLREDUCE_SUM 1
#define AMPNET_SYNC_MAX_SLOTS 32
#define AMPNET_SYNC_MAX_CHANNELS 256
typedef int (*ampnet_collective_fn)(void *ctx, int op, void *send, void *recv, size_t n_floats, void *stream);
size_t ampnet_collective_scratch_bytes(int world_size);
int ampnet_set_collective(ampnet_collective_fn fn, void *ctx, int rank, int world_size, void *scratch, size_t scratch_bytes);

/* ---- matrix-core operand precision (process-wide default, per-thread scoped override) ------------------------
 * AMPNET_PRECISION_F32 (default): v_mfma_f32_32x32x2_f32, exact fp32 products -- the mode every parity figure is quoted in.
 * AMPNET_PRECISION_BF16: the per-point layers of ampnet_encoder_fwd_f32 / ampnet_head_fwd_f32 round their MFMA operands
 * (activations after BatchNorm+ReLU, weights) to bf16 and accumulate in fp32 (v_mfma_f32_32x32x16_bf16); tensors in HBM,
 * BatchNorm statistics, loss and the whole backward stay fp32.  BASELINE.json config 3 ("bf16 MFMA MLP/attention").   */
#define AMPNET_PRECISION_F32 0
#define AMPNET_PRECISION_BF16 1
/* AMPNET_PRECISION_BF16_TRAIN: the forward of AMPNET_PRECISION_BF16 AND the fused backward of the shared per-point layers
 * (weight gradient dW = g^T a and data gradient dy = g W of one pass, csrc/pw_bwd_bf16.hip) with bf16 operands: g = dy P1 + z P2 + P3,
 * the recomputed activation a and the weights are formed in fp32 and rounded once; accumulation, BatchNorm-backward sums, the
 * K <= 12 input layers, the T-Net FC layers, the attention and every tensor in HBM stay fp32.                                   */
#define AMPNET_PRECISION_BF16_TRAIN 2
/* AMPNET_PRECISION_BF16_STORE: AMPNET_PRECISION_BF16_TRAIN, and the activations a train step keeps for its backward (the nine
 * pre-BatchNorm tensors of the encoder, z2 / z3 of the head) are STORED as bf16 (rounded once from the fp32 accumulator; the
 * BatchNorm statistics are taken before the rounding): the step moves about a third fewer HBM bytes.  Inputs, outputs (local,
 * global, feat_T, logits), gradients and parameters stay fp32.
 * ENFORCED: every train-mode ampnet_encoder_fwd_f32 / ampnet_head_fwd_f32 / ampnet_gru_head_fwd_f32 records (on the host) the mode its
 * workspace was written in; the matching *_bwd_f32 returns AMPNET_E_ARG when the storage format differs (mode 3 on one side only), or on a
 * workspace that holds no train-mode forward of this process, instead of misreading the saved activations (tests/test_bf16_gpu.py).
 * Modes 0 .. 2 share the fp32 tape: a backward in one of them may follow a forward in another.                                   */
#define AMPNET_PRECISION_BF16_STORE 3
/* AMPNET_PRECISION_F32_SPLIT ("f32x3"): fp32 results from the bf16 matrix pipe.  Every operand of the MFMA-bound per-point products
 * (the 128 -> 256 pooled layers and the 128 -> 128 layer of the forward; the Gram-form and the dense 128 x 128 fused backward) is split
 * into three bf16 terms a = a1 + a2 + a3 (three successive round-to-nearest roundings: the sum is the fp32 value exactly) and the
 * product is formed from six v_mfma_f32_32x32x16_bf16 instructions (a1 b1, a1 b2, a2 b1, a1 b3, a2 b2, a3 b1: each partial product
 * of two bf16 numbers is exact in fp32, the three dropped terms are below 2^-23 |a b|), accumulated in fp32: 6 / 16 of the fp32 MFMA
 * time at fp32 accuracy.  Tensors in HBM, BatchNorm statistics, prologues, epilogues and every other kernel are those of
 * AMPNET_PRECISION_F32 (same tape: a backward in one of the two modes may follow a forward in the other).  The parity tests of the
 * fp32 path run in this mode with the same bars (tests/conftest.py: AMPNET_TEST_PRECISION).                                       */
#define AMPNET_PRECISION_F32_SPLIT 4
int ampnet_set_matrix_precision(int mode);
int ampnet_get_matrix_precision(void);
/* Scoped override: ampnet_precision_scope_begin(mode) pushes `mode` (validated as ampnet_set_matrix_precision validates it) on a stack
 * that belongs to the CALLING THREAD, ampnet_precision_scope_end() pops it.  While the stack is not empty, every entry point called on
 * that thread dispatches on its top instead of the process-wide default -- including the workspace tags and their check -- so two
 * models of one process can run in different modes, and a backward can be run in the mode its forward recorded whatever the default
 * has become.  Other threads are unaffected.  The stack holds AMPNET_PRECISION_SCOPE_DEPTH entries: one more begin, or an end with
 * nothing pushed, returns AMPNET_E_ARG and changes nothing.  ampnet_get_matrix_precision() keeps returning the process-wide default;
 * ampnet_effective_matrix_precision() returns what a dispatch on the calling thread would see.                                   */
#define AMPNET_PRECISION_SCOPE_DEPTH 8
int ampnet_precision_scope_begin(int mode);
int ampnet_precision_scope_end(void);
int ampnet_effective_matrix_precision(void);

/* ---- a12: baseline single-window PointNet segmentation, eval forward -----------------------------------------
 * replaces SegmentationPointNet.forward (module.eval()) of pointNet/model/pointnet.py:128-154 (variant 0: 1024-d,
 * convolutions with bias, T-Net on x[:, :, :3], :71) and of pointNet/model/light_pointnet_256.py:128-153 (variant 1:
 * 256-d, no conv / fc bias, T-Net on x[:, :, :2], :71).  BASELINE.json config 1 ([4, 512, 9]) is the reference's CPU
 * plumbing case: this entry exists for parity and is not tuned.
 *   layers_host  [AMPNET_POINTNET_LAYERS * 6] device pointers, per layer {weight, bias, bn.weight, bn.bias,
 *                bn.running_mean, bn.running_var}; bias and the four BatchNorm pointers may be NULL.  Layer order:
 *                0-5   base_pointnet.input_transform   conv_1 conv_2 conv_3 fc_1 fc_2 fc_3   (bn_1 .. bn_5, none)
 *                6-11  base_pointnet.feature_transform  (same)
 *                12-16 base_pointnet.conv_1 .. conv_5   (bn_1 .. bn_5)
 *                17-20 conv_1 .. conv_4                 (bn_1 .. bn_3, none)
 *   x [B, N, 9] -> logits [B, n_classes, N]; feat_T [B, 64, 64] (optional) = feature_transform            */
#define AMPNET_POINTNET_LAYERS 21
size_t ampnet_pointnet_seg_workspace_bytes(int variant, int B, int N, int n_classes);
int ampnet_pointnet_seg_fwd_f32(const float *const *layers_host, int variant, const float *x, int B, int N,
                                int n_classes, float *logits, float *feat_T, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---- a12: the same model in train mode (BASELINE.json config 1 end to end) --------------------------------------------------
 * replaces SegmentationPointNet.forward under module.train() + loss.backward() as pointNet/baseline/train_segmentation.py:274-328 drives
 * them: batch-statistics BatchNorm (running statistics updated in place through layers_host, momentum 0.1, unbiased variance), and
 * the gradients of every parameter from (dlogits [B, C, N], d_feat_T [B, 64, 64] or NULL).  The forward keeps its activations in
 * `workspace` (ampnet_pointnet_seg_train_workspace_bytes); the backward must get the same, untouched workspace.  B >= 2.
 *   grads_host   [AMPNET_POINTNET_LAYERS * 4] device pointers per layer {d weight, d bias, d bn.weight, d bn.bias}, NULL where the
 *                layer has no such parameter; every gradient is overwritten                                                    */
size_t ampnet_pointnet_seg_train_workspace_bytes(int variant, int B, int N, int n_classes);
int ampnet_pointnet_seg_train_fwd_f32(const float *const *layers_host, int variant, const float *x, int B, int N, int n_classes,
                                      float *logits, float *feat_T, void *workspace, size_t workspace_bytes, void *stream);
int ampnet_pointnet_seg_bwd_f32(const float *const *layers_host, float *const *grads_host, int variant, const float *x, int B, int N,
                                int n_classes, const float *dlogits, const float *d_feat_T, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---- f4: the baseline classification PointNet (train and eval) ---------------------------------------------------------------
 * replaces ClassificationPointNet.forward of pointNet/model/pointnet.py:100-125 (variant 0: fc 1024 -> 512 -> 256 -> n_classes with bias)
 * and of pointNet/model/light_pointnet_256.py:100-125 (variant 1: fc 256 -> 128 -> 64 without bias, -> n_classes with bias), and
 * loss.backward() through it: global feature of BasePointNet(return_local_features=False) -> relu(bn_1(fc_1)) -> relu(bn_2(fc_2)) ->
 * Dropout(p) -> log_softmax(fc_3).  Same tape as the segmentation model (csrc/baseline_train.hip); built for parity, not tuned.
 *   layers_host  [AMPNET_POINTNET_CLS_LAYERS * 6], per layer as above; layer order 0-16 = base_pointnet (as above), 17-19 = fc_1 (bn_1),
 *                fc_2 (bn_2), fc_3 (none)
 *   train != 0:  batch statistics (running statistics updated in place), dropout keep(i) = hash(seed, i) >= p * 2^32 scaled 1 / (1 - p)
 *                (the package's counter hash, restated by oracle/ampnet_oracle.py:keep_mask -- not torch's Philox stream); B >= 2
 *   train == 0:  running statistics, no dropout
 *   x [B, N, 9] -> log_probs [B, n_classes]; feat_T [B, 64, 64] = feature_transform.
 * The backward takes (d_log_probs [B, n_classes], d_feat_T [B, 64, 64] or NULL), the drop_p / seed of the forward and its untouched
 * workspace; grads_host [AMPNET_POINTNET_CLS_LAYERS * 4] as above, every gradient overwritten.                                      */
#define AMPNET_POINTNET_CLS_LAYERS 20
size_t ampnet_pointnet_cls_workspace_bytes(int variant, int B, int N, int n_classes);
int ampnet_pointnet_cls_fwd_f32(const float *const *layers_host, int variant, const float *x, int B, int N, int n_classes, int train,
                                float drop_p, uint32_t seed, float *log_probs, float *feat_T, void *workspace, size_t workspace_bytes,
                                void *stream);
int ampnet_pointnet_cls_bwd_f32(const float *const *layers_host, float *const *grads_host, int variant, const float *x, int B, int N,
                                int n_classes, float drop_p, uint32_t seed, const float *d_log_probs, const float *d_feat_T,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ---- a7: optimiser -----------------------------------------------------------------------------------------
 * replaces torch.optim.Adam.step as the reference configures it (train_pointnet-attention.py:140-141,469-470):
 * betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad; `step` counts from 1.  One launch updates a list of
 * tensors: four HOST arrays of DEVICE pointers (parameter, gradient, exp_avg, exp_avg_sq) and a host array of sizes.
 * grad_scale multiplies the gradient on the fly (1 / world_size after a SUM all-reduce).                     */
int ampnet_adam_step_f32(float *const *params_host, const float *const *grads_host, float *const *m_host,
                         float *const *v_host, const long *numel_host, int n_tensors, float lr, float beta1,
                         float beta2, float eps, int step, float grad_scale, void *stream);

/* ---- measurement hooks (bench.py roofline leg) --------------------------------------------------------
 * ampnet_profile_enable(1) clears the table and brackets every instrumented kernel launch with two HIP events on
 * the launch stream; ampnet_profile_read() synchronises the device and sums elapsed ms, launches, algorithmic
 * flops and bytes per kernel name (names: max_rows x 64 chars).  Off by default: no events, no overhead.      */
int ampnet_profile_enable(int on);
int ampnet_profile_read(int max_rows, char *names, double *ms, long long *calls, double *flops, double *bytes);

/* ---- test hooks: not used by any product path -----------------------------------------------------------
 * One launch of a per-point layer kernel on inputs the caller chooses (tests/test_pw_layers_gpu.py holds each one
 * to a float64 restatement of its contract).  The structs mirror the internal launch records of csrc/kernels.h
 * (PwGemm, PwBwd + GradSrc / ActSrc): see the comments there for what every field means.  Every pointer comes with
 * its extent in ELEMENTS (`*_n`); before anything is launched the probe checks on the host that each extent covers
 * what the kernel will touch (win_off is copied to the host and checked for monotonicity) and returns AMPNET_E_ARG
 * otherwise.  The current matrix precision picks the kernel family, as it does for the product paths.
 * AmpnetPwGemmProbe.a_bf16 / z_bf16 (the last two fields) declare A / Z to be bf16 tensors behind the float pointers, as
 * precision mode 3 stores them; A_n / Z_n count ELEMENTS of whichever type, so the same extent checks hold.  They are
 * read only where `tail` == 1: a caller built against the descriptor that ended at pfin_out_n left that word (its pad0)
 * at 0, and nothing past its shorter struct is touched.  The probe adds no check of its own on the flags: pw_gemm's argument checks (a bf16 precision mode, lda % 8 == 0 for a bf16 A) are
 * the gate, as in the product.                                                                                */
typedef struct AmpnetPwGemmProbe {
    const float *A; int64_t A_n; int32_t lda, cin;
    const float *W; int64_t W_n; int64_t w_win_stride; int32_t ldw, perwin_slot_major;
    const float *bias; int64_t bias_n; int64_t bias_win_stride;
    const float *pro_scale, *pro_shift; int64_t pro_n;        /* [n_slots, cin] each */
    int32_t n_slots; float drop_p; uint32_t drop_seed; int32_t cout;
    float *Z; int64_t Z_n; int32_t ldz, stat_lanes;
    float *part_sum, *part_sq; int64_t part_n;                 /* each */
    int32_t *part_rows; int64_t part_rows_n;
    float *part_max; int32_t *part_amax; int64_t pool_n;        /* each */
    const float *pool_gamma; int64_t pool_gamma_n;
    const int32_t *win_off; int64_t win_off_n;
    int32_t Q, chunk_rows, chunks, uniform_rows, identity_k; float fin_eps;
    const float *fin_gamma, *fin_beta; int64_t fin_in_n;       /* [cout] each */
    float *fin_scale, *fin_shift, *fin_mean, *fin_invstd, *fin_smean, *fin_suvar; int64_t fin_out_n;   /* [n_slots, cout] each */
    const float *pfin_sum, *pfin_sq; int64_t pfin_n;           /* [pfin_parts, cin] each */
    const int32_t *pfin_rows; int64_t pfin_rows_n; int32_t pfin_parts, tail;   /* tail (the former pad0, 0 there): 1 = a_bf16 / z_bf16 follow */
    const float *pfin_gamma, *pfin_beta; int64_t pfin_in_n;    /* [cin] each */
    float *pfin_scale, *pfin_shift, *pfin_mean, *pfin_invstd, *pfin_smean, *pfin_suvar; int64_t pfin_out_n;   /* [n_slots, cin] each */
    int32_t a_bf16, z_bf16;                                     /* A / Z are bf16 tensors (PwGemm.a_bf16 / z_bf16); A_n / Z_n stay in ELEMENTS */
} AmpnetPwGemmProbe;

/* kind 0 = pw_bwd_fused (which picks the split / bf16 kernels by itself, as in the product).  dbg_row_wrap is always 0.
 * kind 1 = pw_dgrad (PwDgrad): g = (dy, gz, P1..P3, act, CX), prev = (pz, ps, pt, drop, CY == cp), W / ldw / w_slot_stride /
 *          w_win_stride / perwin_slot_major, bias_slot, add, out, part_a / part_b [Q * part_chunks, cp], chunk_rows x chunks per window.
 * kind 2 = pw_wgrad (PwWgrad): x = (dy, gz, P1..P3, act, CX), y = (pz, ps, pt, drop, CY), dWpart [Q * chunks, CX, ldp],
 *          dbpart [Q * chunks, CX].
 * Kinds 1 and 2 read fp32 tensors only (no bf16 z) and take the dense / act gradient sources (not the sparse arg / dpool one). */
typedef struct AmpnetPwBwdProbe {
    int32_t kind, CX, CY, act;
    const float *dy, *gz; int64_t g_n;                         /* [rows, CX] each; gz may be a bf16 tensor (g_z_bf16) */
    const float *P1, *P2, *P3; int64_t P_n;                    /* [n_slots, CX] each */
    int32_t g_z_bf16, prev_z_bf16;
    const float *pz; int64_t pz_n;                             /* [rows, CY] */
    const float *ps, *pt, *prev_mean, *prev_invstd; int64_t ps_n;   /* [n_slots, CY] each */
    float drop_p; uint32_t drop_seed;
    const float *W; int64_t W_n; int64_t w_slot_stride, w_win_stride; int32_t ldw, perwin_slot_major;
    const float *bias_slot; int64_t bias_slot_n;
    const float *add; int64_t add_n;
    float *out; int64_t out_n;
    float *dWpart, *dbpart, *part_a, *part_b; int64_t dW_n, db_n, pab_n;
    const int32_t *win_off; int64_t win_off_n;
    int32_t Q, n_slots, max_rows, blocks_per_slot, items_per_block, fin_parts;
    const float *fin_part_a, *fin_part_b; int64_t fin_part_n;  /* [fin_parts, CX] each */
    int32_t fin_rows, pad0;
    const float *fin_gamma, *fin_mean, *fin_invstd; int64_t fin_in_n;   /* [n_slots, CX] each (gamma: [CX]) */
    float *fin_P1, *fin_P2, *fin_P3, *fin_slot_ab; int64_t fin_out_n;    /* each >= [n_slots, CX, 2] */
    int32_t cp, part_chunks, chunk_rows, chunks, ldp, pad1;     /* kinds 1 and 2 (ABI 6) */
} AmpnetPwBwdProbe;

/* One launch of a kernel of the max-pooled layers' backward (kernels.h, "backward of a max-pooled layer"), by `op`:
 *   0 pool_bwd        (d_pooled, arg, zext, scale .. invstd -> dpm, P1 .. P3, slot_ab)
 *   1 slot_mats       (W, P2, P3 -> G, c0)
 *   2 sparse_scatter  (arg, dpm, P1, W, z_prev (bf16 if z_bf16), *_prev -> out +=, part_a / part_b at q * part_chunks + slot_idx)
 *   3 sparse_rows     (arg, dpm, P1, W -> srows, srow_row, srow_cnt)
 *   4 sparse_fix      (srows, srow_row, srow_cnt, z_prev, *_prev -> out +=, part_a / part_b)
 *   5 pooled_wgrad    (W, P1 .. P3, gram, asum, arg, dpm, z_prev, s_prev, t_prev -> dW; wgram optional scratch)
 *   6 reduce_slots    (red_part0 [Q * chunks, red_n0] -> red_out0 [n_slots, red_n0])
 *   7 reduce_slots2   (the same for both pairs in one launch)
 * arg (and, for op 4, srow_cnt / srow_row) are copied to the host and every row they name must lie in its own window;
 * C <= 256, cp <= 128, Q % n_slots == 0 and pooled_wgrad's LDS bound are checked before the launch.                  */
typedef struct AmpnetPooledBwdProbe {
    int32_t op, Q, n_slots, C, cp, slot_major, z_bf16, chunks, part_chunks, slot_idx, red_n0, red_n1;
    const int32_t *win_off; int64_t win_off_n;
    const int32_t *arg; int64_t arg_n;                          /* [Q, C] */
    const float *zext, *d_pooled; float *dpm; int64_t qc_n;     /* [Q, C] each */
    const float *scale, *shift, *mean, *invstd; int64_t bn_n;   /* [n_slots, C] each */
    float *P1, *P2, *P3; int64_t P_n;                           /* [n_slots, C] each */
    float *slot_ab; int64_t slot_ab_n;                          /* [n_slots, C, 2] */
    const float *W; int64_t W_n;                                /* [C, cp] */
    float *G, *c0; int64_t G_n, c0_n;                           /* [n_slots, cp, cp], [n_slots, cp] */
    const float *z_prev; int64_t z_prev_n;                      /* [rows, cp] */
    const float *s_prev, *t_prev, *mean_prev, *invstd_prev; int64_t prev_n;   /* [n_slots, cp] each */
    float *out; int64_t out_n;                                  /* [rows, cp] */
    float *part_a, *part_b; int64_t part_n;                     /* [Q * part_chunks, cp] each */
    float *srows; int64_t srows_n;                              /* [Q * C, cp] */
    int32_t *srow_row; int64_t srow_row_n;                      /* [Q * C] */
    int32_t *srow_cnt; int64_t srow_cnt_n;                      /* [Q] */
    const float *gram, *asum; int64_t gram_n, asum_n;           /* [n_slots, cp, cp], [n_slots, cp] */
    float *wgram; int64_t wgram_n;                              /* [n_slots, C, cp] or NULL */
    float *dW; int64_t dW_n;                                    /* [C, cp] */
    const float *red_part0, *red_part1; int64_t red_part0_n, red_part1_n;
    float *red_out0, *red_out1; int64_t red_out0_n, red_out1_n;
} AmpnetPooledBwdProbe;

/* The input layers' weight gradient: op 0 = pw_input_wgrad (PwInputWgrad, bwd_misc.h; P1 .. P3 given, or formed in the kernel from
 * fin_part_a / fin_part_b), op 1 = input_param_grads (dWeff -> dW, and dT at the slot-major row in mode 1).  mode 0: W [64, 3];
 * mode 1: W [64, 12] and T [Q, 3, 3].                                                                                              */
typedef struct AmpnetInputWgradProbe {
    int32_t op, mode, perwin_slot_major, Q, n_slots, fin_parts, fin_rows, pad0;
    const float *x; int64_t x_n;                                /* [rows, 9] */
    const float *dy; int64_t dy_n;                              /* [rows, 64] */
    const float *W; int64_t W_n;
    const float *T; int64_t T_n;                                /* [Q, 9] */
    const float *P1, *P2, *P3; int64_t P_n;                     /* [n_slots, 64] each */
    const float *fin_part_a, *fin_part_b; int64_t fin_part_n;   /* [fin_parts, 64] each */
    const float *fin_gamma; int64_t fin_gamma_n;                /* [64] */
    const float *fin_mean, *fin_invstd; int64_t fin_in_n;       /* [n_slots, 64] each */
    float *fin_P1, *fin_P2, *fin_P3, *fin_slot_ab; int64_t fin_out_n;   /* each >= [n_slots, 64, 2] */
    float *dWeff; int64_t dWeff_n;                              /* [Q, 64, 9] */
    float *dW; int64_t dW_n;                                    /* [64, 3] or [64, 12] */
    float *dT; int64_t dT_n;                                    /* [Q, 9] (mode 1) */
    const int32_t *win_off; int64_t win_off_n;
} AmpnetInputWgradProbe;

/* the geometry the orchestration would choose for a layer of Q windows (max_rows rows at most) in n_slots slots */
typedef struct AmpnetPwPlan {
    int32_t stat_lanes, stat_parts, stat_direct, stat_lane_cap;   /* pw_gemm_stat_plan(Q, stat_chunks, n_slots, lane cap of cin x cout) */
    int32_t chunk_rows, chunks, x_chunk_rows, x_chunks;           /* enc_shape: point layers, point layers on the split kernels */
    int32_t fc_rows, fc_chunk_rows, fc_chunks;
    int32_t bwd_blocks, bwd_item_rows, bwd_x3;                    /* pw_bwd_blocks, pw_bwd_item_rows, pw_bwd_x3_supported(bwd) (-1: bwd NULL) */
} AmpnetPwPlan;

/* One launch of a kernel of the segmentation head, the loss tail or the small-GEMM token path (ABI 7), by `op`:
 *   0 posenc_tokens       (gl [Q, 256], cent [Q, 2], w1 [16, 2], b1 [16], w2 [256, 16], b2 [256] -> tok [Q, 256]; hid / slope [Q, 16] both or neither)
 *   1 attention_core      (qkv [B * W, 768], mask [B, W] or NULL -> probs [B, 8, W, W] or NULL, ctx [B * W, 256]; drop_p, drop_seed = the hash base)
 *   2 attention_core_bwd  (qkv, probs, dctx [B * W, 256] -> dqkv [B * W, 768])
 *   3 head_logits (+ loss_finalize when loss_out is given)
 *                         (z4 [R, ldz4] -> logits [R / P, C, P]; preds [R], targets [R], class_w [C], loss_part [cdiv(R, 256), 2], loss_out [2]
 *                          optional; as in the head's forward the kernel gets loss_part only together with targets)
 *   4 head_out_bwd        (dlogits [R / P, C, P], z3 [R, 64] fp32 or (z_bf16) bf16, scale / shift / mean / invstd [64], w4 [C, 64]
 *                          -> dy3 [R, 64], part_a / part_b [cdiv(R, 1024), 64], w4part [cdiv(R, 1024), C * 64 + C])
 *   5 sgemm_linear_bwd    (G [rows, n_out] ldg, X [rows, n_in] ldx, Wl [n_out, n_in] ldw -> dW [n_out, n_in] lddw, dX [rows, n_in] lddx;
 *                          db [n_out] and dx_mul [rows, n_in] (lddx) optional)
 *   6 sgemm_wgrad_bias    (G, X -> dW, db)
 *   7 exp / log sweep     (X [rows] -> dX [3, rows] = __expf(x), expf(x), logf(x): the device functions the softmax bars of the tests rest on)
 * 1 <= W <= 32, 1 <= C <= 8, R % P == 0 and every extent are checked on the host before the launch.  The launch is recorded under the
 * kernel's name for ampnet_profile_read ("head_out_bwd<f32>" / "head_out_bwd<bf16>" by z_bf16; the small GEMMs record their own).
 * z3_n counts elements of z3's own type.                                                                                        */
typedef struct AmpnetHeadProbe {
    int32_t op, B, W, Q, R, P, C, ldz4, z_bf16, rows, n_out, n_in, ldg, ldx, ldw, lddw, lddx, pad0;
    float drop_p; uint32_t drop_seed;
    const float *gl, *cent, *w1, *b1, *w2, *b2; int64_t gl_n, cent_n, w1_n, b1_n, w2_n, b2_n;
    float *tok, *hid, *slope; int64_t tok_n, hid_n;              /* hid_n: hid and slope each */
    const float *qkv; int64_t qkv_n;
    const uint8_t *mask; int64_t mask_n;
    float *probs; int64_t probs_n;                               /* written by op 1, read by op 2 */
    float *ctx; int64_t ctx_n;
    const float *dctx; int64_t dctx_n;
    float *dqkv; int64_t dqkv_n;
    const float *z4; int64_t z4_n;
    float *logits; int64_t logits_n;
    const long long *targets; int64_t targets_n;
    const float *class_w; int64_t class_w_n;
    long long *preds; int64_t preds_n;
    float *loss_part; int64_t loss_part_n;
    float *loss_out; int64_t loss_out_n;
    const float *dlogits; int64_t dlogits_n;
    const float *z3; int64_t z3_n;
    const float *scale, *shift, *mean, *invstd; int64_t bn_n;    /* [64] each */
    const float *w4; int64_t w4_n;
    float *dy3; int64_t dy3_n;
    float *part_a, *part_b; int64_t part_n;                      /* each */
    float *w4part; int64_t w4part_n;
    const float *G; int64_t G_n;
    const float *X; int64_t X_n;
    const float *Wl; int64_t Wl_n;
    float *dW; int64_t dW_n;
    float *dX; int64_t dX_n;
    float *db; int64_t db_n;
    const float *dx_mul; int64_t dx_mul_n;
} AmpnetHeadProbe;

/* One launch of a BatchNorm / pooling glue kernel (csrc/pw_misc.hip, bwd_misc.hip, pw_bwd.hip: reduce_windows) or of its host entry
 * point (ABI 15; csrc/layer_probe.hip, tests/test_bn_glue_gpu.py), by `op`.  Field names are those of the launch records in csrc/kernels.h.
 *   0  pw_input            (x [rows, 9], W [64, 3 | 12], T [Q, 9] in mode 1 -> Z [rows, 64] fp32 or (z_bf16) bf16; part_sum / part_sq
 *                           [Q * chunks, 64], or with part_rows [parts] the per-workgroup form [parts, 64], parts = stat_lanes rounded up to
 *                           a multiple of n_slots, stat_lanes from ampnet_probe_bn_plan)
 *   1  bn_finalize         (part_sum / part_sq [Q * chunks, C]; rows per partial from part_rows [Q * chunks], uniform_rows or win_off;
 *                           gamma / beta [C] -> scale / shift [n_slots, C]; mean / invstd and stat_mean / stat_uvar optional;
 *                           merge_ws [bn_finalize_merge_floats] optional: the two-stage form where the host entry point picks it)
 *   2  bn_finalize_gathered (part_sum = gather_ranks segments of gather_seg floats {mean [n_slots, C], M2 [n_slots, C], rows [n_slots] int})
 *   3  bn_fold             (n_items layers of it_C[i] channels, item i at offset sum_{j<i} it_C[j] of gamma / beta / rmean / rvar / scale /
 *                           shift; eps)
 *   4  bn_running_update   (item i at offset n_slots * sum_{j<i} it_C[j] of stat_mean / stat_uvar [n_slots, it_C[i]] and sum it_C[j] of
 *                           rmean / rvar; momentum)
 *   5  pool_finalize       (part_max [Q * chunks, C], part_amax or NULL, scale / shift [n_slots, C] -> pooled, arg, zext [Q, C]; mode 1:
 *                           the in-kernel BatchNorm form, C == 256, part_sum / part_sq [pfin_parts, 256] and part_rows [pfin_parts] are the
 *                           producer's partials, gamma / beta in, scale / shift / mean / invstd / stat_mean / stat_uvar out; win_off is
 *                           needed with part_amax: every entry must be -1 or a row of its window)
 *   6  bn_bwd_finalize     (part_a / part_b [(part_Q > 0 ? part_Q : Q) * chunks, C], win_off or uniform_rows, gamma, mean, invstd
 *                           -> P1 .. P3 [n_slots, C], slot_ab [n_slots, C, 2])
 *   7  bn_param_grads      (items as op 4: slot_ab [n_slots, it_C[i], 2] -> dgamma / dbeta [it_C[i]])
 *   8  fc_act              (z [rows, C], scale / shift [cdiv(rows, per), C] -> act)
 *   9  fc_act_pair         (op 8 for (z, scale, shift, act, C) and (z1, s1, t1, act1, C1) in one launch)
 *   10 fc_bn_bwd           (da, z [n_slots * per, C], scale .. invstd [n_slots, C] -> g, slot_ab)
 *   11 colsum              (src [rows, C] -> dst [C])
 *   12 reduce_windows      (src: Q partials `stride` apart of [rows, cols] on ld_part -> dst [rows, cols] on ld_dst, = or +=)
 *   13 reduce_windows_multi (n_items of op 12's overwrite form: it_* and the element offsets it_part_off / it_dst_off into src / dst)
 *   14 transpose64_slot_major (src [Q * chunks, 64, 64], add [Q, 64, 64] or NULL -> dst [Q, 64, 64])
 *   15 add_identity        (dst [Q, k, k] += I)
 *   16 fill_i32_ramp       (idst [rows] = i * step)
 * Every extent is checked on the host first (win_off, part_amax and, for op 5 mode 1, part_rows are copied to the host for that).
 * While a collective is installed the host entry points take their global-batch branches: ops 1, 6 and 10 run them (one exchange per
 * call, after the checks: every rank must make the same calls; shapes beyond the scratch segment come back as AMPNET_E_ARG before any
 * exchange), every other op refuses to run.                                                                                         */
#define AMPNET_BN_PROBE_ITEMS 25       /* one more than bn_fold / bn_running_update / bn_param_grads take: the refusal can be reached */
#define AMPNET_BN_PROBE_REDUCE 13      /* one more than reduce_windows_multi takes */
typedef struct AmpnetBnProbe {
    int32_t op, mode, Q, n_slots, C, C1, chunks, chunk_rows, uniform_rows, stat_lanes, perwin_slot_major, z_bf16, out_slot_major, part_Q,
            pfin_parts, gather_ranks, n_items, rows, cols, ld_part, ld_dst, accumulate, by_workgroup, per, k, step;
    float eps, momentum;
    int64_t stride, gather_seg;
    int32_t it_C[AMPNET_BN_PROBE_ITEMS], pad0;
    int32_t it_Q[AMPNET_BN_PROBE_REDUCE], it_rows[AMPNET_BN_PROBE_REDUCE], it_cols[AMPNET_BN_PROBE_REDUCE],
            it_ld_part[AMPNET_BN_PROBE_REDUCE], it_ld_dst[AMPNET_BN_PROBE_REDUCE], pad1;
    int64_t it_stride[AMPNET_BN_PROBE_REDUCE], it_part_off[AMPNET_BN_PROBE_REDUCE], it_dst_off[AMPNET_BN_PROBE_REDUCE];
    const float *x; int64_t x_n;
    const float *W; int64_t W_n;
    const float *T; int64_t T_n;
    float *Z; int64_t Z_n;                                      /* elements of Z's own type */
    float *part_sum; int64_t part_sum_n;
    float *part_sq; int64_t part_sq_n;
    int32_t *part_rows; int64_t part_rows_n;
    const int32_t *win_off; int64_t win_off_n;
    const float *gamma; int64_t gamma_n;
    const float *beta; int64_t beta_n;
    float *scale; int64_t scale_n;
    float *shift; int64_t shift_n;
    float *mean; int64_t mean_n;
    float *invstd; int64_t invstd_n;
    float *stat_mean; int64_t stat_mean_n;
    float *stat_uvar; int64_t stat_uvar_n;
    float *merge_ws; int64_t merge_ws_n;
    float *rmean; int64_t rmean_n;
    float *rvar; int64_t rvar_n;
    const float *part_max; int64_t part_max_n;
    const int32_t *part_amax; int64_t part_amax_n;
    float *pooled; int64_t pooled_n;
    int32_t *arg; int64_t arg_n;
    float *zext; int64_t zext_n;
    const float *part_a; int64_t part_a_n;
    const float *part_b; int64_t part_b_n;
    float *P1; int64_t P1_n;
    float *P2; int64_t P2_n;
    float *P3; int64_t P3_n;
    float *slot_ab; int64_t slot_ab_n;
    float *dgamma; int64_t dgamma_n;
    float *dbeta; int64_t dbeta_n;
    const float *z; int64_t z_n;
    const float *da; int64_t da_n;
    float *g; int64_t g_n;
    float *act; int64_t act_n;
    const float *z1; int64_t z1_n;
    const float *s1; int64_t s1_n;
    const float *t1; int64_t t1_n;
    float *act1; int64_t act1_n;
    const float *src; int64_t src_n;
    float *dst; int64_t dst_n;
    const float *add; int64_t add_n;
    int32_t *idst; int64_t idst_n;
} AmpnetBnProbe;

/* what the orchestration would size for the input layers' per-workgroup statistics and the two-stage bn_finalize */
typedef struct AmpnetBnPlan {
    int32_t input_stat_lanes;      /* pw_input_stat_lanes(Q, chunks, n_slots) */
    int32_t input_stat_parts;      /* the partial slots those lanes write: lanes rounded up to a multiple of n_slots */
    int64_t merge_floats;          /* bn_finalize_merge_floats(n_slots, C) */
} AmpnetBnPlan;

/* One launch of a kernel of the GRU recurrence (csrc/gru_head.hip) or of the classification head (csrc/cls_head.hip) through the launch
 * wrappers the product entry points call (csrc/head.h), by `op` (ABI 16; csrc/layer_probe.hip, tests/test_gru_cls_layers_gpu.py):
 *   0 gru_seq_kernel      (gi [B * W, 192] = W_ih x + b_ih, Whh [192, 64], bhh [192] -> h_out [B * W, 64]; gates [B * W, 256] =
 *                          (r, z, n, W_hn h + b_hn) per step, or NULL)
 *   1 gru_seq_bwd_kernel  (dH [B * W, 64], gates, h_all [B * W, 64], Whh -> dgi, dgh [B * W, 192], hprev_out [B * W, 64])
 *   2 cls_mix_kernel      (o [B * W, 256] (token (b, w) at row b W + w), cw [W], cb [1] -> x [B, 256])
 *   3 cls_weights_kernel  (probs [B, 8, W, W], drop_p, drop_seed = the hash base -> wout [B, W, W])
 *   4 cls_bn_act_kernel   (z [B, 128] in place, b2, gamma, beta [128], rmean, rvar [128] in place when train -> scale, shift, mean,
 *                          invstd [128], act [B, 128])
 *   5 cls_out_kernel      (act [B, 128], W3 [C, 128], b3 [C] -> out [B, C])
 *   6 cls_mix_bwd_kernel  (dx, x [B, 256], o, cw -> d_o [B * W, 256], cwpart [B, W + 1])
 *   7 tanhf / sigmoid sweep (X [rows] -> Y [2, rows] = tanhf(x), the recurrence's 1 / (1 + __expf(-x)))
 * 1 <= B <= 65535; 1 <= W <= 4096 for ops 0 and 1, 1 <= W <= 32 for ops 2, 3, 6; 1 <= C <= 16 for op 5; 0 <= drop_p < 1; every extent is
 * checked on the host before the launch, which is recorded under the kernel's name for ampnet_profile_read ("gru_act_sweep" for op 7). */
typedef struct AmpnetSeqProbe {
    int32_t op, B, W, C, train, rows; float drop_p; uint32_t drop_seed;
    const float *gi; int64_t gi_n;
    const float *Whh; int64_t Whh_n;
    const float *bhh; int64_t bhh_n;
    float *h_out; int64_t h_out_n;
    float *gates; int64_t gates_n;                               /* written by op 0, read by op 1 */
    const float *dH; int64_t dH_n;
    const float *h_all; int64_t h_all_n;
    float *dgi; int64_t dgi_n;
    float *dgh; int64_t dgh_n;
    float *hprev_out; int64_t hprev_out_n;
    const float *o; int64_t o_n;
    const float *cw; int64_t cw_n;
    const float *cb; int64_t cb_n;
    float *x; int64_t x_n;                                       /* written by op 2, read by op 6 */
    const float *probs; int64_t probs_n;
    float *wout; int64_t wout_n;
    float *z; int64_t z_n;
    const float *b2; int64_t b2_n;
    const float *gamma; int64_t gamma_n;
    const float *beta; int64_t beta_n;
    float *rmean; int64_t rmean_n;
    float *rvar; int64_t rvar_n;
    float *scale; int64_t scale_n;
    float *shift; int64_t shift_n;
    float *mean; int64_t mean_n;
    float *invstd; int64_t invstd_n;
    float *act; int64_t act_n;                                   /* written by op 4, read by op 5 */
    const float *W3; int64_t W3_n;
    const float *b3; int64_t b3_n;
    float *out; int64_t out_n;
    const float *dx; int64_t dx_n;
    float *d_o; int64_t d_o_n;
    float *cwpart; int64_t cwpart_n;
    const float *X; int64_t X_n;
    float *Y; int64_t Y_n;
} AmpnetSeqProbe;

/* One launch of a kernel of the baseline single-window PointNet (csrc/baseline.hip: bl_*, the eval forward; csrc/baseline_train.hip: bt_*,
 * the train forward and backward) through the launch wrappers the product entry points call (csrc/baseline.h), by `op` (ABI 18;
 * csrc/layer_probe.hip, tests/test_baseline_layers_gpu.py).  Rows are [M, C]; windowed tensors are [B, N, C]:
 *    0 bt_bias            (z [M, C] in place, bias [C] or NULL, add [ceil(M / per), C] or NULL, per)
 *    1 bt_stats           (z [M, C], eps, momentum -> mean, invstd [C]; rm, rv [C] in place)
 *    2 bt_running_stats   (rm, rv [C], eps -> mean, invstd [C])
 *    3 bt_bn_act          (z [M, C], mean, invstd, gamma, beta [C] -> a [M, C])
 *    4 bt_bn_bwd_sums     (da, a, z [M, C], mean, invstd [C] -> dg, dbe [C])
 *    5 bt_bn_bwd_apply    (da [M, C] in place, a, z, mean, invstd, gamma, dg, dbe)
 *    6 bt_rowmax          (a [B, N, C] -> out [B, C], arg [B, C])            7 bl_rowmax (a -> out)
 *    8 bt_pool_scatter    (x = d_pool [B, C], arg [B, C] (each in [0, N), checked) -> a = d_a [B, N, C], which the caller zeroed)
 *    9 bt_mix, 10 bl_mix  (x [M, 9], T [ceil(M / N), k, k] -> out [M, 9]; M rows in windows of N; k in {2, 3})
 *   11 bt_mix_bwd         (x, da = d_xin [B * N, 9] -> out = dT [B, k, k])
 *   12 bt_segsum          (da = dz [B, N, C] -> out [B, C])
 *   13 bt_logits          (z [B * N, C] -> out [B, C, N])      14 bt_logits_to_rows (out -> z)      15 bl_logits (as 13)
 *   16 bt_fill            (z [n] = value)                       17 bt_add (z [n] += x [n])
 *   18 bt_dropout         (a [n], drop_p, drop_seed -> out [n]; out == a allowed)
 *   19 bt_log_softmax     (z [B, C] -> out [B, C]; C <= 64)     20 bt_log_softmax_bwd (z, da = d_out [B, C] -> out = dz)
 *   21 bl_fold            (bias, gamma (with beta, rm, rv) [C], either NULL, eps -> scale, shift [C])
 *   22 bl_affine          (z [M, C] in place, scale, shift [C], add [ceil(M / per), C] or NULL, per, relu)
 *   23 fwd_layer          (A [M, lda], W [C, ldw] read at column w0, K; bias / gamma, beta, rm, rv / add, per as above; train = 0 takes
 *                          the running statistics -> z [M, C], a [M, C] (gamma given, else z alone is written), mean, invstd [C])
 *   24 bwd_layer          (da [M, C] in place, a, z, mean, invstd, gamma or NULL, W, A as above -> dW [C, ldw] at column w0, db or NULL,
 *                          dg, dbe (required with gamma), dA [M, ld_dA] or NULL, = or += by `accumulate`)
 * Every dimension an op reads is >= 1 and every product of them < 2^24; B <= 65535.  Every extent is checked on the host before the launch
 * (AMPNET_E_ARG, nothing written); single-kernel ops are recorded under the kernel's name for ampnet_profile_read.                        */
typedef struct AmpnetBaselineProbe {
    int32_t op, B, N, M, C, K, k, per, relu, train, accumulate, lda, ldw, w0, ld_dA, pad0;
    float eps, momentum, value, drop_p; uint32_t drop_seed, pad1;
    int64_t n;
    float *z; int64_t z_n;
    float *a; int64_t a_n;
    float *da; int64_t da_n;
    float *mean; int64_t mean_n;
    float *invstd; int64_t invstd_n;
    const float *gamma; int64_t gamma_n;
    const float *beta; int64_t beta_n;
    float *rm; int64_t rm_n;
    float *rv; int64_t rv_n;
    const float *bias; int64_t bias_n;
    const float *add; int64_t add_n;
    float *dg; int64_t dg_n;
    float *dbe; int64_t dbe_n;
    float *out; int64_t out_n;
    int32_t *arg; int64_t arg_n;
    const float *x; int64_t x_n;
    const float *T; int64_t T_n;
    const float *W; int64_t W_n;
    float *dW; int64_t dW_n;
    float *db; int64_t db_n;
    float *dA; int64_t dA_n;
    const float *A; int64_t A_n;
    float *scale; int64_t scale_n;
    float *shift; int64_t shift_n;
} AmpnetBaselineProbe;

int ampnet_probe_baseline_f32(const AmpnetBaselineProbe *d, void *stream);
int ampnet_probe_pw_gemm_f32(const AmpnetPwGemmProbe *d, void *stream);
int ampnet_probe_pw_bwd_f32(const AmpnetPwBwdProbe *d, void *stream);
int ampnet_probe_pooled_bwd_f32(const AmpnetPooledBwdProbe *d, void *stream);
int ampnet_probe_input_wgrad_f32(const AmpnetInputWgradProbe *d, void *stream);
int ampnet_probe_head_f32(const AmpnetHeadProbe *d, void *stream);
int ampnet_probe_bn_f32(const AmpnetBnProbe *d, void *stream);
int ampnet_probe_bn_plan(int Q, int chunks, int n_slots, int C, AmpnetBnPlan *out_host);
int ampnet_probe_seq_f32(const AmpnetSeqProbe *d, void *stream);
int ampnet_probe_pw_plan(int Q, int n_slots, int max_rows, int cin, int cout, int stat_chunks, const AmpnetPwBwdProbe *bwd, AmpnetPwPlan *out_host);

/* The tape of ampnet_sa_train_backward_f32 (csrc/set_abstraction_train.hip; tests/test_sa_train_gpu.py checks every layer alone on it).
 * For layer l < L of the shape (D, n_clouds, s, nsample, cout_host, L): the byte offsets inside the backward's workspace, and the row
 * strides in floats, of x_l (the layer's input rows, stride = cin_l rounded up to 32, the padded columns zero) and dz_l (stride cout_l).
 * Both hold the M = n_clouds s nsample rows (g, t), t < nsample, in that order, and are valid after ampnet_sa_train_backward_f32 has
 * returned (and its stream has run) until the workspace is written again.  Launches nothing; the shape's refusals are the backward's. */
int ampnet_sa_train_backward_tape(int D, int n_clouds, int s, int nsample, const int *cout_host, int L, int l, size_t *x_offset_bytes,
                                  int *x_stride, size_t *dz_offset_bytes, int *dz_stride);

#ifdef __cplusplus
}
#endif
#endif /* AMPNET_HIP_H */
