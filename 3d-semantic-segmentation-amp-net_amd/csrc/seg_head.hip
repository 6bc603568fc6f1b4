// seg_head.hip -- the per-point classifier of the PointNet++ semantic-segmentation model in eval mode, fused (C ABI:
// ampnet_seg_head_forward_f32; the arithmetic: include/ampnet_hip.h).  Per row x of [M][ld]:
//     h = relu(bn_eval(W1 x + b1)),  z = W2 h + b2,  logp = log_softmax(z),  pred = the lowest arg-max of z.
// The fold kernel (fused_mlp.hip) runs first, then ONE kernel: neither h nor z reaches HBM.
//
//   * The rows are a flat list: a wave owns 32 consecutive rows (a tile may span clouds, the head has no per-cloud structure) and walks the
//     tiles blockIdx.x * nw + wave, + gridDim.x * nw, as the feature-propagation forward does.
//   * Tile A [32][max(kp, 32) + 1] takes the rows (coalesced; zeros past cin and past M), conv1 is the shared core's one layer
//     (mlp_dispatch<K_QUADS>, MlpToTile) into tile B [32][hidden + 1], conv2 is mlp_accumulate<1, K_QUADS> on tile B against W2 staged in LDS
//     zero-padded to 32 rows (seg_head.h).  z then passes through tile A, which x has left free: lane t < 32 reads row t, takes the max,
//     the lowest arg-max and S over the classes ascending, and writes the row's log-probabilities back.
//   * logp [M][n_classes] is dense, so all 64 lanes store the tile's rows * n_classes floats flat: consecutive lanes, consecutive floats.
//     The rows past M are never stored.
//   * The plan is mlp_plan_build's with the tiles and the staging laid out here: the waves per workgroup are halved (4, 2, 1) until the
//     tiles fit beside W2, and W1 is staged behind W2 when it still fits (else read through L2 by dwordx4, as fp1 of pointnet_2 reads its).
//   * Train mode (seg_head_train.hip) launches the same kernel as its last step, on a fold formed from the batch statistics and with
//     DROP = true: eval and train share the hot kernel, as fp_forward_kernel serves both feature-propagation forwards.
#include "seg_head.h"

namespace ampnet {

// DROP = false is eval mode and does nothing with `drop`; DROP = true (train mode, seg_head_train.hip) drops and rescales conv1's
// activations in tile B before conv2 reads them.
template <bool DROP>
__global__ __launch_bounds__(256) void seg_head_forward_kernel(MlpPlan p, SegPlan s, SegDrop drop, const float *__restrict__ x, int ld,
                                                              long long M, const float *__restrict__ fold, int n_tiles,
                                                              float *__restrict__ logp, long long *__restrict__ preds)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = s.n_classes;
    const MlpLds m = mlp_lds(p, 32, s_mem, wave);
    float *s_w2 = m.s_w + s.w2_off;
    mlp_stage_weights(p, m.s_w, tid, 64 * p.nw);
    seg_stage_w2(s_w2, s.w2, C, s.hidden, tid, 64 * p.nw);
    __syncthreads();
    for (int tile = blockIdx.x * p.nw + wave; tile < n_tiles; tile += gridDim.x * p.nw) {
        const long long row0 = (long long)tile * 32;
        const int rows = (int)min(32LL, M - row0);
        seg_load_rows(m.tile_a, p.ld_a, p.kp[0], x + (size_t)row0 * ld, ld, p.cin[0], rows, lane);
        wave_lds_sync();
        mlp_dispatch<K_QUADS>(p, 0, 32, m.s_w, m.tile_a, p.ld_a, fold, MlpToTile{m.tile_b, p.ld_b}, nullptr, lane);
        wave_lds_sync();
        if (DROP) {
            seg_dropout(m.tile_b, p.ld_b, s.hidden, row0, rows, drop, lane);
            wave_lds_sync();
        }
        seg_logits(m.tile_b, p.ld_b, s_w2, s.hidden, s.b2, C, m.tile_a, p.ld_a, lane);       // (conv1's reads of tile A are done)
        wave_lds_sync();
        if (lane < 32) {
            const int arg = seg_log_softmax_row(m.tile_a + lane * p.ld_a, C);
            if (preds && lane < rows) preds[row0 + lane] = arg;
        }
        wave_lds_sync();
        float *dst = logp + (size_t)row0 * C;
        for (int e = lane; e < rows * C; e += 64) {
            const int t = e / C;
            dst[e] = m.tile_a[t * p.ld_a + (e - t * C)];
        }
        wave_lds_sync();                          // the next tile's rows overwrite tile A
    }
}

int seg_shape(const char *what, int cin, int hidden, int n_classes, long long M, SegShape &sh)
{
    AMPNET_REQUIRE(cin >= 1 && cin <= AMPNET_SEG_HEAD_MAX_CIN, "%s: cin=%d must be in [1, %d]", what, cin, AMPNET_SEG_HEAD_MAX_CIN);
    AMPNET_REQUIRE(hidden >= 32 && hidden <= AMPNET_SEG_HEAD_MAX_HIDDEN && hidden % 32 == 0, "%s: hidden=%d must be a multiple of 32 in [32, %d]",
                   what, hidden, AMPNET_SEG_HEAD_MAX_HIDDEN);
    AMPNET_REQUIRE(n_classes >= 2 && n_classes <= AMPNET_SEG_HEAD_MAX_CLASSES, "%s: n_classes=%d must be in [2, %d]", what, n_classes,
                   AMPNET_SEG_HEAD_MAX_CLASSES);
    // (the tile counter of a wave steps by at most 4096 past the last tile: keep that inside an int)
    AMPNET_REQUIRE(M >= 1 && M <= AMPNET_SEG_HEAD_MAX_ROWS, "%s: M=%lld rows must be in [1, %lld]", what, M, (long long)AMPNET_SEG_HEAD_MAX_ROWS);
    sh = {};
    sh.n_tiles = (int)((M + 31) / 32);
    sh.grid = sh.n_tiles < FPB_MAX_GRID ? sh.n_tiles : FPB_MAX_GRID;
    fpb_chunk_rule(M, sh.chunk_rows, sh.chunks);
    sh.fold_floats = align_up((size_t)2 * hidden, 64);
    AMPNET_TRY(mlp_bwd_layout(what, sh.fold_floats, cin, 0, M, sh.grid, sh.chunks, &hidden, 1, sh.lay));
    sh.ldxs0 = sh.lay.ldxs[0];
    // behind the shared layout: conv1's activations h [M][hidden], dz [M][32] (the class dimension padded with zeros), the workgroups'
    // partial sums of dz [grid][32], dW2 as the split-K GEMM writes it [32][hidden].  (The split-K partials of the shared layout hold
    // chunks * hidden * ldxs0 floats, ldxs0 >= 32: enough for dW2's.)
    size_t off = sh.lay.floats;
    sh.off_hs = off;
    off += align_up((size_t)M * hidden, 64);
    sh.off_dz2 = off;
    off += align_up((size_t)M * 32, 64);
    sh.off_parts2 = off;
    off += align_up((size_t)sh.grid * 32, 64);
    sh.off_dw2 = off;
    off += (size_t)32 * hidden;
    sh.floats = off;
    sh.off_coef = align_up(off, 64);
    sh.train_floats = sh.off_coef + align_up((size_t)2 * hidden, 64);
    sh.off_stats = sh.fold_floats;
    sh.train_fwd_floats = sh.off_stats + align_up((size_t)sh.grid * 3 * hidden, 64);
    return AMPNET_OK;
}

int seg_check_entry(const char *what, const float *x, int ld, int cin, int hidden, int n_classes, long long M, const float *const *params_host,
                    SegShape &sh)
{
    AMPNET_REQUIRE(x && params_host, "%s: null pointer", what);
    for (int q = 0; q < 8; ++q) AMPNET_REQUIRE(params_host[q], "%s: null parameter %d (W1, b1, gamma, beta, running_mean, running_var, W2, b2)", what, q);
    AMPNET_TRY(seg_shape(what, cin, hidden, n_classes, M, sh));
    AMPNET_REQUIRE(ld >= cin, "%s: ld=%d is less than cin=%d", what, ld, cin);
    return AMPNET_OK;
}

int seg_forward_plan(const char *what, int cin, int hidden, const float *const *params_host, float eps, MlpPlan &p, MlpFold &f, size_t &lds)
{
    if (!mlp_plan_build(what, cin, 32, params_host, &hidden, &eps, 1, p, f)) return AMPNET_E_ARG;
    // the tiles and the staging of this kernel: tile A also carries z (32 columns), tile B conv1's activations; W2, then W1 if it fits
    p.ld_a = (p.kp[0] > 32 ? p.kp[0] : 32) + 1;
    p.ld_b = hidden + 1;
    const size_t tile_bytes = (size_t)32 * (p.ld_a + p.ld_b) * sizeof(float), w2_floats = (size_t)32 * (hidden + 1),
                 w1_floats = (size_t)hidden * (p.kp[0] + 1);
    p.nw = 4;
    while (p.nw > 1 && p.nw * tile_bytes + w2_floats * sizeof(float) > (size_t)MLP_LDS_BYTES) p.nw /= 2;
    lds = p.nw * tile_bytes + w2_floats * sizeof(float);
    AMPNET_REQUIRE(lds <= (size_t)MLP_LDS_BYTES, "%s: a wave's tiles and W2 (%zu bytes) exceed the LDS", what, lds);
    p.w_off[0] = lds + w1_floats * sizeof(float) <= (size_t)MLP_LDS_BYTES ? (int)w2_floats : -1;
    if (p.w_off[0] >= 0) lds += w1_floats * sizeof(float);
    return AMPNET_OK;
}

int seg_forward_launch(const char *what, const MlpPlan &p, size_t lds, const SegPlan &s, const SegDrop *drop, const float *x, int ld, long long M,
                       const float *fold, int n_tiles, float *logp, long long *preds, hipStream_t st)
{
    static bool attr_set[2] = {false, false};
    const dim3 grid(mlp_grid(n_tiles, p.nw)), block(64 * p.nw);
    if (drop) {
        AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(seg_head_forward_kernel<true>), attr_set[1]));
        hipLaunchKernelGGL(seg_head_forward_kernel<true>, grid, block, lds, st, p, s, *drop, x, ld, M, fold, n_tiles, logp, preds);
    } else {
        AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(seg_head_forward_kernel<false>), attr_set[0]));
        hipLaunchKernelGGL(seg_head_forward_kernel<false>, grid, block, lds, st, p, s, SegDrop{}, x, ld, M, fold, n_tiles, logp, preds);
    }
    return check_launch("seg_head_forward_kernel");
}

}  // namespace ampnet

extern "C" size_t ampnet_seg_head_forward_workspace_bytes(int cin, int hidden, int n_classes, long long M)
{
    using namespace ampnet;
    SegShape sh;
    if (seg_shape("ampnet_seg_head_forward_workspace_bytes", cin, hidden, n_classes, M, sh) != AMPNET_OK) return 0;
    return sh.fold_floats * sizeof(float);
}

extern "C" int ampnet_seg_head_forward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes, const float *const *params_host,
                                           float eps, float *logp, long long *preds, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_seg_head_forward_f32";
    hipStream_t st = (hipStream_t)stream;
    SegShape sh;
    AMPNET_TRY(seg_check_entry(what, x, ld, cin, hidden, n_classes, M, params_host, sh));
    AMPNET_REQUIRE(logp, "%s: null pointer", what);
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.fold_floats * sizeof(float)));
    MlpPlan p;
    MlpFold f;
    size_t lds;
    AMPNET_TRY(seg_forward_plan(what, cin, hidden, params_host, eps, p, f, lds));
    const SegPlan s = {n_classes, hidden, 0, params_host[6], params_host[7]};
    float *fold = static_cast<float *>(workspace);
    AMPNET_TRY(mlp_fold_launch(p, f, fold, st));
    return seg_forward_launch(what, p, lds, s, nullptr, x, ld, M, fold, sh.n_tiles, logp, preds, st);
}
