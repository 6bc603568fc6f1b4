// seg_head_train.hip -- the per-point classifier of the PointNet++ segmentation model in TRAIN mode: bn1 on the statistics of the batch,
// its running statistics updated, drop1 a real dropout (C ABI: ampnet_seg_head_train_forward_f32 and its _workspace_bytes; the
// arithmetic: include/ampnet_hip.h).  Everything runs on the caller's stream, no float atomics, every summation order a function of the
// shape alone; exact fp32 MFMA whatever the matrix precision is.  The backward is seg_head_train_bwd.hip.
//
//   segt_stats_kernel           Four waves per workgroup, a wave owns a partial row at a time: row r takes the 32-row tiles r, r + P, ..
//       (P = min(tiles, 1024)) in ascending order, whatever the launch's shape is.  Per tile it loads the rows (seg_load_rows: zeros past
//       cin and past M), forms conv1's raw accumulators a = W1 x in the forward's contraction order and merges the tile's count, mean and
//       sum (a - mean)^2 over its VALID rows into the partial row (bn_train.h: bnt_tile_stats, Chan's merge).  W1 is read through L2, as
//       fpt_stats_kernel reads the layer it takes statistics of; no activation reaches memory.
//   fpt_stats_finalize_kernel   (bn_train.hip) a wave per channel merges the partial rows and writes save_mean, save_invstd, the
//       running-statistics update and scale = gamma invstd, shift = fma(-mean, scale, beta) into the fold -- the two operations
//       fpt_fold_kernel repeats from the saved statistics in the backward: the same bits.
//   seg_head_forward_kernel<DROP>   (seg_head.hip) the eval forward's kernel on that fold, so the accumulators the statistics were taken
//       from are the ones it normalises, bit for bit.  drop_p > 0 runs the DROP = true instantiation, which keeps and rescales conv1's
//       activations in LDS between conv1 and conv2; drop_p == 0 runs eval's own instantiation and hashes nothing.
#include "bn_train.h"
#include "seg_head.h"

namespace ampnet {

constexpr int SEGT_STATS_WAVES = 4;

// parts [n_parts][3 hidden]: per partial row the count, mean and sum of squared deviations of every channel
__global__ __launch_bounds__(64 * SEGT_STATS_WAVES) void segt_stats_kernel(MlpPlan p, const float *__restrict__ x, int ld, long long M, int n_tiles,
                                                                         int n_parts, float *__restrict__ parts)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cin = p.cin[0], hidden = p.cout[0], kp = p.kp[0];
    float *tile = s_mem + wave * 32 * p.ld_a;     // (private to the wave: no workgroup barrier anywhere)
    for (int row = blockIdx.x * SEGT_STATS_WAVES + wave; row < n_parts; row += gridDim.x * SEGT_STATS_WAVES) {
        float *part_n = parts + (size_t)row * 3 * hidden, *part_mean = part_n + hidden, *part_m2 = part_mean + hidden;
        if (lane < 32)
            for (int c = lane; c < hidden; c += 32) part_n[c] = part_mean[c] = part_m2[c] = 0.0f;     // channel c belongs to lane c % 32
        for (int t = row; t < n_tiles; t += n_parts) {
            const long long row0 = (long long)t * 32;
            const int rows = (int)min(32LL, M - row0);
            seg_load_rows(tile, p.ld_a, kp, x + (size_t)row0 * ld, ld, cin, rows, lane);
            wave_lds_sync();
            int n0 = 0;
            if (p.w_vec[0]) {
                for (; n0 + 128 <= hidden; n0 += 128) bnt_tile_stats<4, K_QUADS, true>(tile, p.ld_a, 0, p.w[0], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
                for (; n0 < hidden; n0 += 32) bnt_tile_stats<1, K_QUADS, true>(tile, p.ld_a, 0, p.w[0], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
            } else {
                for (; n0 + 128 <= hidden; n0 += 128) bnt_tile_stats<4, K_QUADS, false>(tile, p.ld_a, 0, p.w[0], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
                for (; n0 < hidden; n0 += 32) bnt_tile_stats<1, K_QUADS, false>(tile, p.ld_a, 0, p.w[0], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
            }
            wave_lds_sync();                      // the next tile's rows overwrite the tile
        }
    }
}

int segt_shape(const char *what, int cin, int hidden, int n_classes, long long M, SegShape &sh)
{
    AMPNET_TRY(seg_shape(what, cin, hidden, n_classes, M, sh));
    return bnt_rows_ok(what, M, AMPNET_SEG_HEAD_TRAIN_MAX_ROWS, "rows");
}

int segt_check_drop(const char *what, float drop_p)
{
    AMPNET_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, "%s: drop_p=%g must be in [0, 1)", what, (double)drop_p);      // (NaN fails both)
    return AMPNET_OK;
}

}  // namespace ampnet

extern "C" size_t ampnet_seg_head_train_forward_workspace_bytes(int cin, int hidden, int n_classes, long long M)
{
    using namespace ampnet;
    SegShape sh;
    if (segt_shape("ampnet_seg_head_train_forward_workspace_bytes", cin, hidden, n_classes, M, sh) != AMPNET_OK) return 0;
    return sh.train_fwd_floats * sizeof(float);
}

extern "C" int ampnet_seg_head_train_forward_f32(const float *x, int ld, long long M, int cin, int hidden, int n_classes, float *const *params_host,
                                                 float eps, float momentum, float drop_p, uint32_t seed, float *logp, float *save_mean,
                                                 float *save_invstd, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_seg_head_train_forward_f32";
    hipStream_t st = (hipStream_t)stream;
    SegShape sh;
    AMPNET_TRY(seg_check_entry(what, x, ld, cin, hidden, n_classes, M, params_host, sh));
    AMPNET_TRY(bnt_rows_ok(what, M, AMPNET_SEG_HEAD_TRAIN_MAX_ROWS, "rows"));
    AMPNET_REQUIRE(logp, "%s: null pointer", what);
    AMPNET_REQUIRE(save_mean && save_invstd, "%s: null save_mean or save_invstd", what);
    AMPNET_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "%s: momentum=%g must be in [0, 1]", what, (double)momentum);
    AMPNET_TRY(segt_check_drop(what, drop_p));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.train_fwd_floats * sizeof(float)));
    // the hot kernel's plan, with the saved statistics where the fold looks for them
    const float *slots[8] = {params_host[0], params_host[1], params_host[2], params_host[3], save_mean, save_invstd, params_host[6], params_host[7]};
    MlpPlan p;
    MlpFold f;
    size_t lds;
    AMPNET_TRY(seg_forward_plan(what, cin, hidden, slots, eps, p, f, lds));
    float *fold = static_cast<float *>(workspace), *parts = fold + sh.off_stats;
    const size_t stats_lds = (size_t)SEGT_STATS_WAVES * 32 * p.ld_a * sizeof(float);          // at most 4 * 32 * 257 floats: 129 KB
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(segt_stats_kernel), attr_set));
    hipLaunchKernelGGL(segt_stats_kernel, dim3(cdiv(sh.grid, SEGT_STATS_WAVES)), dim3(64 * SEGT_STATS_WAVES), stats_lds, st, p, x, ld, M, sh.n_tiles,
                       sh.grid, parts);
    AMPNET_TRY(check_launch("segt_stats_kernel"));
    const FptStats q = {f.bias[0], f.gamma[0], f.beta[0], params_host[4], params_host[5], save_mean, save_invstd, eps, momentum, hidden, p.fold_off[0]};
    AMPNET_TRY(fpt_stats_finalize_launch(q, parts, sh.grid, M, fold, st));
    const SegPlan s = {n_classes, hidden, 0, params_host[6], params_host[7]};
    const SegDrop drop = {drop_base(seed, 0), drop_threshold(drop_p), 1.0f / (1.0f - drop_p)};
    return seg_forward_launch(what, p, lds, s, drop_p > 0.0f ? &drop : nullptr, x, ld, M, fold, sh.n_tiles, logp, nullptr, st);
}
