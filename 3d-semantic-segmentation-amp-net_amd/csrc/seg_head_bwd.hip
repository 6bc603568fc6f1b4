// seg_head_bwd.hip -- the backward of the fused segmentation head with BatchNorm's running statistics frozen (C ABI:
// ampnet_seg_head_backward_f32, ampnet_seg_head_backward_workspace_bytes).  With g = dlogp, any upstream gradient:
//     dz_c = g_c - expf(logp_c) sum_j g_j,  db2 = sum_rows dz,  dW2 = dz^T h,  dh = dz W2,
// and from dh on conv1 is ONE layer of the frozen-statistics backward of feature_propagation_bwd.hip.  The forward keeps nothing.  Kernels on
// the caller's stream:
//
//   fold (sa_fold_kernel)        scale and shift, as in the forward.
//   seg_head_backward_kernel     A workgroup is ONE wave and a wave owns 32 consecutive rows, walking the tiles blockIdx.x, + gridDim.x.  Tiles in
//       LDS: X [32][kp + 1] the rows, H [32][hidden + 1], D and G [32][33], and W2 staged zero-padded to 32 rows (seg_head.h).  It loads x and
//       g (zeros past M and past n_classes), runs conv1 with the forward's own code into H, forms z in D and the log-probabilities with the
//       forward's own code (seg_logits, seg_log_softmax_row: the same bits), and lane t < 32 turns row t of D into dz in place, the
//       columns past n_classes and the rows past M zeros.  Lane c < 32 adds column c of D, rows ascending, into ITS word of the workgroup's
//       row of partials.  dh = dz W2 is mlp_dgrad on the staged W2 with the class dimension padded to 32 (zeros add nothing) and
//       overwrites H; fpb_recompute finds conv1's accumulators and ReLU mask again from X and leaves dz1 = dy scale in H, and dx = dz1 W1
//       (mlp_dgrad) goes straight to the caller's dx when it is wanted.  x, h, dz (32 columns) and dz1 of the wave's rows go to the
//       workspace for the two weight gradients.
//   fp_wgrad_kernel, fp_wgrad_reduce_kernel   twice (mlp_bwd.hip): dW1 = dz1^T x to the caller, dW2 = dz^T h as [32][hidden] to the workspace,
//       whose first n_classes rows a device-to-device copy hands to the caller's dW2.
//   seg_db2_kernel               db2: a wave per class adds the workgroups' partials, lane t the workgroups t, t + 64, .. ascending, then a halving
//       tree (the order of fp_bwd_finalize_kernel).
//   fp_bwd_finalize_kernel       dbeta, dgamma and db1 of conv1 (mlp_bwd.hip).
//
// Every order is a function of the shape alone: no float atomics, two runs give the same bits.  Exact fp32 MFMA whatever the matrix
// precision is.
#include "seg_head.h"

namespace ampnet {

__global__ __launch_bounds__(64) void seg_head_backward_kernel(MlpPlan p, SegPlan s, SegBwdPlan b, const float *__restrict__ x, int ld, long long M,
                                                              const float *__restrict__ fold, const float *__restrict__ dlogp, int n_tiles,
                                                              float *__restrict__ dx)
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
        // dh = dz W2 over the 32 padded classes -> H.  mlp_dgrad takes ONE number as the row stride of w and as the bound of the column:
        // the staged copy's stride is hidden + 1 and the columns walked here end at hidden - 1.
        int c0 = 0;
        for (; c0 + 128 <= hidden; c0 += 128) mlp_dgrad<4>(D, SEG_LD_D, s_w2, hidden + 1, 32, c0, H, b.ld_h, nullptr, 0, nullptr, 0, rows, lane);
        for (; c0 < hidden; c0 += 32) mlp_dgrad<1>(D, SEG_LD_D, s_w2, hidden + 1, 32, c0, H, b.ld_h, nullptr, 0, nullptr, 0, rows, lane);
        wave_lds_sync();
        float *dz_ws = b.dz1 + (size_t)row0 * hidden;
        int n0 = 0;
        if (p.w_vec[0]) {
            for (; n0 + 128 <= hidden; n0 += 128)
                fpb_recompute<4, true>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
            for (; n0 < hidden; n0 += 32)
                fpb_recompute<1, true>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
        } else {
            for (; n0 + 128 <= hidden; n0 += 128)
                fpb_recompute<4, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
            for (; n0 < hidden; n0 += 32)
                fpb_recompute<1, false>(X, b.ld_x, p.w[0], cin, kp, hidden, n0, scale, shift, H, b.ld_h, nullptr, rows, dz_ws, part_b, part_g, lane);
        }
        wave_lds_sync();
        if (dx) {                                 // every column is the caller's: D1 = cin, nothing goes to the dx_0 rows of a gather
            float *dst = dx + (size_t)row0 * cin;
            for (c0 = 0; c0 + 128 <= cin; c0 += 128) mlp_dgrad<4>(H, b.ld_h, p.w[0], cin, hidden, c0, nullptr, 0, dst, cin, nullptr, 0, rows, lane);
            for (; c0 < cin; c0 += 32) mlp_dgrad<1>(H, b.ld_h, p.w[0], cin, hidden, c0, nullptr, 0, dst, cin, nullptr, 0, rows, lane);
        }
        wave_lds_sync();
    }
}

__global__ __launch_bounds__(256) void seg_db2_kernel(const float *__restrict__ parts2, int n_parts, int n_classes, float *__restrict__ db2)
{
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_classes) return;                   // (the whole wave)
    float v = 0.0f;
    for (int q = lane; q < n_parts; q += 64) v += parts2[(size_t)q * 32 + c];
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    if (!lane) db2[c] = v;
}

int seg_weight_grads_launch(const char *what, const SegShape &sh, float *ws, int cin, int hidden, int n_classes, long long M,
                            float *const *grads_host, hipStream_t st)
{
    float *wpart = ws + sh.lay.off_wpart, *dw2 = ws + sh.off_dw2;
    AMPNET_TRY(fpb_wgrad_launch(ws + sh.lay.off_dz[0], hidden, ws + sh.lay.off_xs[0], cin, sh.ldxs0, M, sh.chunk_rows, sh.chunks, wpart,
                                grads_host[0], st));
    AMPNET_TRY(fpb_wgrad_launch(ws + sh.off_dz2, 32, ws + sh.off_hs, hidden, hidden, M, sh.chunk_rows, sh.chunks, wpart, dw2, st));
    hipError_t e = hipMemcpyAsync(grads_host[4], dw2, (size_t)n_classes * hidden * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "%s: hipMemcpyAsync(dW2): %s", what, hipGetErrorString(e));
    hipLaunchKernelGGL(seg_db2_kernel, dim3(cdiv(n_classes, 4)), dim3(256), 0, st, ws + sh.off_parts2, sh.grid, n_classes, grads_host[5]);
    return check_launch("seg_db2_kernel");
}

}  // namespace ampnet

extern "C" size_t ampnet_seg_head_backward_workspace_bytes(int cin, int hidden, int n_classes, long long M)
{
    using namespace ampnet;
    SegShape sh;
    if (seg_shape("ampnet_seg_head_backward_workspace_bytes", cin, hidden, n_classes, M, sh) != AMPNET_OK) return 0;
    return sh.floats * sizeof(float);
}

extern "C" int ampnet_seg_head_backward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes, const float *const *params_host,
                                            float eps, const float *dlogp, float *dx, float *const *grads_host, void *workspace,
                                            size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_seg_head_backward_f32";
    hipStream_t st = (hipStream_t)stream;
    SegShape sh;
    AMPNET_TRY(seg_check_entry(what, x, ld, cin, hidden, n_classes, M, params_host, sh));
    AMPNET_REQUIRE(dlogp && grads_host, "%s: null pointer", what);
    AMPNET_TRY(sa_check_tables(what, nullptr, grads_host, 1));
    AMPNET_REQUIRE(grads_host[4] && grads_host[5], "%s: null gradient pointer (dW2, db2)", what);
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.floats * sizeof(float)));
    MlpPlan p;
    MlpFold f;
    if (!mlp_plan_build(what, cin, 32, params_host, &hidden, &eps, 1, p, f)) return AMPNET_E_ARG;
    mlp_plan_unstaged(p);
    float *ws = static_cast<float *>(workspace);
    SegBwdPlan b;
    const size_t lds = seg_bwd_plan(p, sh, ws, b);
    AMPNET_REQUIRE(lds <= (size_t)MLP_LDS_BYTES, "%s: a wave's tiles (%zu bytes) exceed the LDS", what, lds);
    const SegPlan s = {n_classes, hidden, 0, params_host[6], params_host[7]};
    FpBwdFin g = {};
    g.dbias[0] = grads_host[1];
    g.dgamma[0] = grads_host[2];
    g.dbeta[0] = grads_host[3];
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(seg_head_backward_kernel), attr_set));
    AMPNET_TRY(mlp_fold_launch(p, f, ws, st));
    hipLaunchKernelGGL(seg_head_backward_kernel, dim3(sh.grid), dim3(64), lds, st, p, s, b, x, ld, M, ws, dlogp, sh.n_tiles, dx);
    AMPNET_TRY(check_launch("seg_head_backward_kernel"));
    AMPNET_TRY(seg_weight_grads_launch(what, sh, ws, cin, hidden, n_classes, M, grads_host, st));
    return fpb_finalize_launch(p, f, g, ws, b.parts, sh.grid, hidden, st);
}
