// seg_head_train_bwd.hip -- the backward of the segmentation head in TRAIN mode, through bn1's batch statistics and drop1's mask (C ABI:
// ampnet_seg_head_train_backward_f32 and its _workspace_bytes; the arithmetic: include/ampnet_hip.h).  The forward keeps save_mean and
// save_invstd only; everything else is recomputed with the forward's own code, so the ReLU mask, the keep mask and the log-probabilities are
// the forward's bits.  dz1 needs sum dy and sum dy a over ALL rows, so the work is two phases with a finalize between them.  Kernels on
// the caller's stream:
//
//   fpt_fold_kernel             (bn_train.hip) scale and shift from the saved statistics, by the forward's two operations.
//   segt_bwd_phase1_kernel      A workgroup is ONE wave and a wave owns 32 consecutive rows, walking the tiles blockIdx.x, + gridDim.x; the
//       LDS tiles X, H, D, G and the staged W2 of seg_head_backward_kernel.  It loads x and g, runs conv1 with the forward's code into H,
//       drops and rescales H in place (hd, stored for dW2), forms z, the log-probabilities and dz in D as the eval backward does (stored
//       padded to 32 columns, with the workgroup's db2 partials), dh = dz W2 over H (mlp_dgrad on the staged W2), the mask and scale of
//       dropout on dh in the tile, and bnt_form_dy (bn_train.h) on X: dy = dh' [y > 0] to the workspace and sum dy, sum dy a into the
//       workgroup's own partial row.
//   fpt_bwd_finalize_kernel     (bn_train.hip) dbeta, dgamma = invstd (G - mean dbeta), db1 = 0 and the coefficients dbeta / M and
//       dgamma invstd / M of phase 2.
//   segt_bwd_phase2_kernel      The same walk.  X comes back from the workspace copy phase 1 stored, bnt_form_dz recomputes a and writes
//       dz1 = scale (dy - dbeta / M - (a - mean) invstd dgamma / M) into the tile and over dy, and dx = dz1 W1 (mlp_dgrad) goes straight
//       to the caller when it is wanted.
//   seg_weight_grads_launch     (seg_head_bwd.hip) dW1, dW2 and db2, exactly the eval backward's.
//
// Every order is a function of the shape alone: no float atomics, two runs give the same bits.  Exact fp32 MFMA whatever the matrix
// precision is.  Neither phase kernel spills, so the column loops are not split further than four tiles at a time.
#include "bn_train.h"
#include "seg_head.h"

namespace ampnet {

template <bool DROP>
__global__ __launch_bounds__(64) void segt_bwd_phase1_kernel(MlpPlan p, SegPlan s, SegBwdPlan b, SegDrop drop, const float *__restrict__ x, int ld,
                                                            long long M, const float *__restrict__ fold, const float *__restrict__ dlogp,
                                                            int n_tiles)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x;
    const int C = s.n_classes, hidden = s.hidden, cin = p.cin[0], kp = p.kp[0];
    float *X = s_mem, *H = s_mem + b.off_h, *D = s_mem + b.off_d, *G = s_mem + b.off_g, *s_w2 = s_mem + b.off_w2;
    float *part_b = b.parts + (size_t)blockIdx.x * 2 * hidden, *part_g = part_b + hidden, *part_2 = b.parts2 + (size_t)blockIdx.x * 32;
    if (lane < 32) {
        for (int c = lane; c < hidden; c += 32) part_b[c] = part_g[c] = 0.0f;       // channel c belongs to lane c % 32, here and below
        part_2[lane] = 0.0f;
    }
    seg_stage_w2(s_w2, s.w2, C, hidden, lane, 64);
    const float *scale = fold, *shift = fold + hidden;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = (long long)tile * 32;
        const int rows = (int)min(32LL, M - row0);
        seg_load_rows(X, b.ld_x, kp, x + (size_t)row0 * ld, ld, cin, rows, lane);
        for (int e = lane; e < 32 * 32; e += 64) {
            const int t = e >> 5, c = e & 31;
            G[t * SEG_LD_D + c] = t < rows && c < C ? dlogp[(size_t)(row0 + t) * C + c] : 0.0f;
        }
        wave_lds_sync();                          // (the first tile: also the staged W2)
        fpb_store_rows(X, b.ld_x, kp, b.xs0 + (size_t)row0 * b.ldxs0, b.ldxs0, rows, lane);
        mlp_dispatch<K_QUADS>(p, 0, 32, s_mem, X, b.ld_x, fold, MlpToTile{H, b.ld_h}, nullptr, lane);
        wave_lds_sync();
        if (DROP) {
            seg_dropout(H, b.ld_h, hidden, row0, rows, drop, lane);
            wave_lds_sync();
        }
        fpb_store_rows(H, b.ld_h, hidden, b.hs + (size_t)row0 * hidden, hidden, rows, lane);
        seg_logits(H, b.ld_h, s_w2, hidden, s.b2, C, D, SEG_LD_D, lane);
        wave_lds_sync();
        if (lane < 32) {
            float *zr = D + lane * SEG_LD_D;
            const float *gr = G + lane * SEG_LD_D;
            seg_log_softmax_row(zr, C);
            float sg = 0.0f;
            for (int c = 0; c < C; ++c) sg += gr[c];
            for (int c = 0; c < C; ++c) zr[c] = lane < rows ? fmaf(-expf(zr[c]), sg, gr[c]) : 0.0f;
            for (int c = C; c < 32; ++c) zr[c] = 0.0f;
        }
        wave_lds_sync();
        fpb_store_rows(D, SEG_LD_D, 32, b.dz2 + (size_t)row0 * 32, 32, rows, lane);
        if (lane < 32) {
            float sb = 0.0f;
            for (int t = 0; t < 32; ++t) sb += D[t * SEG_LD_D + lane];
            part_2[lane] += sb;                   // (this lane alone ever touches this word)
        }
        // dh = dz W2 over the 32 padded classes -> H (hd has gone to the workspace), as in seg_head_backward_kernel
        int c0 = 0;
        for (; c0 + 128 <= hidden; c0 += 128) mlp_dgrad<4>(D, SEG_LD_D, s_w2, hidden + 1, 32, c0, H, b.ld_h, nullptr, 0, nullptr, 0, rows, lane);
        for (; c0 < hidden; c0 += 32) mlp_dgrad<1>(D, SEG_LD_D, s_w2, hidden + 1, 32, c0, H, b.ld_h, nullptr, 0, nullptr, 0, rows, lane);
        wave_lds_sync();
        if (DROP) {                               // dh' = keep ? dh dscale : 0: the forward's mask, hashed again
            seg_dropout(H, b.ld_h, hidden, row0, rows, drop, lane);
            wave_lds_sync();
        }
        float *dz_ws = b.dz1 + (size_t)row0 * hidden;
        int n0 = 0;
        if (p.w_vec[0]) {
            for (; n0 + 128 <= hidden; n0 += 128)
                bnt_form_dy<4, K_QUADS, true, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
            for (; n0 < hidden; n0 += 32)
                bnt_form_dy<1, K_QUADS, true, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
        } else {
            for (; n0 + 128 <= hidden; n0 += 128)
                bnt_form_dy<4, K_QUADS, false, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
            for (; n0 < hidden; n0 += 32)
                bnt_form_dy<1, K_QUADS, false, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
        }
        wave_lds_sync();                          // the next tile overwrites every tile
    }
}

__global__ __launch_bounds__(64) void segt_bwd_phase2_kernel(MlpPlan p, SegBwdPlan b, long long M, const float *__restrict__ fold,
                                                            const float *__restrict__ mean, const float *__restrict__ coef, int n_tiles,
                                                            float *__restrict__ dx)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x;
    const int hidden = p.cout[0], cin = p.cin[0], kp = p.kp[0];
    float *X = s_mem, *T = s_mem + b.off_h;
    const float *scale = fold, *shift = fold + hidden, *c1 = coef, *c2 = coef + hidden;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = (long long)tile * 32;
        const int rows = (int)min(32LL, M - row0);
        fpb_load_rows(X, b.ld_x, kp, b.xs0 + (size_t)row0 * b.ldxs0, b.ldxs0, rows, lane);
        wave_lds_sync();
        float *dz_ws = b.dz1 + (size_t)row0 * hidden;
        int n0 = 0;
        if (p.w_vec[0]) {
            for (; n0 + 128 <= hidden; n0 += 128)
                bnt_form_dz<4, K_QUADS, true>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, mean, c1, c2, T, b.ld_h, rows, 0, nullptr, nullptr, dz_ws, lane);
            for (; n0 < hidden; n0 += 32)
                bnt_form_dz<1, K_QUADS, true>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, mean, c1, c2, T, b.ld_h, rows, 0, nullptr, nullptr, dz_ws, lane);
        } else {
            for (; n0 + 128 <= hidden; n0 += 128)
                bnt_form_dz<4, K_QUADS, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, mean, c1, c2, T, b.ld_h, rows, 0, nullptr, nullptr, dz_ws, lane);
            for (; n0 < hidden; n0 += 32)
                bnt_form_dz<1, K_QUADS, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, mean, c1, c2, T, b.ld_h, rows, 0, nullptr, nullptr, dz_ws, lane);
        }
        wave_lds_sync();
        if (dx) {                                 // every column is the caller's, as in seg_head_backward_kernel
            float *dst = dx + (size_t)row0 * cin;
            int c0 = 0;
            for (; c0 + 128 <= cin; c0 += 128) mlp_dgrad<4>(T, b.ld_h, p.w[0], cin, hidden, c0, nullptr, 0, dst, cin, nullptr, 0, rows, lane);
            for (; c0 < cin; c0 += 32) mlp_dgrad<1>(T, b.ld_h, p.w[0], cin, hidden, c0, nullptr, 0, dst, cin, nullptr, 0, rows, lane);
        }
        wave_lds_sync();                          // the next tile overwrites both tiles
    }
}

}  // namespace ampnet

extern "C" size_t ampnet_seg_head_train_backward_workspace_bytes(int cin, int hidden, int n_classes, long long M)
{
    using namespace ampnet;
    SegShape sh;
    if (segt_shape("ampnet_seg_head_train_backward_workspace_bytes", cin, hidden, n_classes, M, sh) != AMPNET_OK) return 0;
    return sh.train_floats * sizeof(float);
}

extern "C" int ampnet_seg_head_train_backward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes,
                                                  const float *const *params_host, float eps, float drop_p, uint32_t seed, const float *save_mean,
                                                  const float *save_invstd, const float *dlogp, float *dx, float *const *grads_host,
                                                  void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_seg_head_train_backward_f32";
    hipStream_t st = (hipStream_t)stream;
    SegShape sh;
    AMPNET_TRY(seg_check_entry(what, x, ld, cin, hidden, n_classes, M, params_host, sh));
    AMPNET_TRY(bnt_rows_ok(what, M, AMPNET_SEG_HEAD_TRAIN_MAX_ROWS, "rows"));
    AMPNET_REQUIRE(dlogp && grads_host, "%s: null pointer", what);
    AMPNET_REQUIRE(save_mean && save_invstd, "%s: null save_mean or save_invstd", what);
    AMPNET_TRY(segt_check_drop(what, drop_p));
    AMPNET_TRY(sa_check_tables(what, nullptr, grads_host, 1));
    AMPNET_REQUIRE(grads_host[4] && grads_host[5], "%s: null gradient pointer (dW2, db2)", what);
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.train_floats * sizeof(float)));
    // the saved statistics where the fold looks for them; running_mean and running_var are not read
    const float *slots[6] = {params_host[0], params_host[1], params_host[2], params_host[3], save_mean, save_invstd};
    MlpPlan p;
    MlpFold f;
    if (!mlp_plan_build(what, cin, 32, slots, &hidden, &eps, 1, p, f)) return AMPNET_E_ARG;
    mlp_plan_unstaged(p);
    float *ws = static_cast<float *>(workspace), *coef = ws + sh.off_coef;
    SegBwdPlan b;
    const size_t lds = seg_bwd_plan(p, sh, ws, b);
    AMPNET_REQUIRE(lds <= (size_t)MLP_LDS_BYTES, "%s: a wave's tiles (%zu bytes) exceed the LDS", what, lds);
    const SegPlan s = {n_classes, hidden, 0, params_host[6], params_host[7]};
    const SegDrop drop = {drop_base(seed, 0), drop_threshold(drop_p), 1.0f / (1.0f - drop_p)};
    static bool attr_set[3] = {false, false, false};
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(segt_bwd_phase1_kernel<false>), attr_set[0]));
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(segt_bwd_phase1_kernel<true>), attr_set[1]));
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(segt_bwd_phase2_kernel), attr_set[2]));
    AMPNET_TRY(fpt_fold_launch(p, f, ws, st));
    if (drop_p > 0.0f)
        hipLaunchKernelGGL(segt_bwd_phase1_kernel<true>, dim3(sh.grid), dim3(64), lds, st, p, s, b, drop, x, ld, M, ws, dlogp, sh.n_tiles);
    else
        hipLaunchKernelGGL(segt_bwd_phase1_kernel<false>, dim3(sh.grid), dim3(64), lds, st, p, s, b, drop, x, ld, M, ws, dlogp, sh.n_tiles);
    AMPNET_TRY(check_launch("segt_bwd_phase1_kernel"));
    AMPNET_TRY(fpt_bwd_finalize_launch(hidden, b.parts, sh.grid, M, save_mean, save_invstd, grads_host[1], grads_host[2], grads_host[3], coef, st));
    const size_t lds2 = (size_t)(b.off_h + 32 * b.ld_h) * sizeof(float);
    hipLaunchKernelGGL(segt_bwd_phase2_kernel, dim3(sh.grid), dim3(64), lds2, st, p, b, M, ws, save_mean, coef, sh.n_tiles, dx);
    AMPNET_TRY(check_launch("segt_bwd_phase2_kernel"));
    return seg_weight_grads_launch(what, sh, ws, cin, hidden, n_classes, M, grads_host, st);
}
