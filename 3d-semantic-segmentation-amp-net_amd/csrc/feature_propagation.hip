// feature_propagation.hip -- one PointNet++ feature-propagation layer in eval mode, fused (C ABI: ampnet_fp_forward_f32).
//
// The input row of fine point i of cloud c is  [points1[i] (D1 values, or none), sum_k w_k points2[idx_k] (D2 values)],  the column order of
// the usual cat([points1, interpolated]); w_k = r_k / sum_k r_k, r_k = 1 / (dist2_k + 1e-8f), over the k <= 3 neighbours
// ampnet_three_nn_f32 found (k = 1: weight 1, the usual implementation's "repeat" branch).  Every layer computes relu(bn_eval(W row + b))
// and the last layer's activations are the output: there is no reduction over rows.  Nothing interpolated, concatenated or intermediate
// reaches HBM: a WAVE owns 32 consecutive fine points of one cloud, builds their rows straight into its own LDS tile and keeps them there
// through all layers (fused_mlp.h: the lane map, the LDS layout, the ping-pong, the weight staging and the BatchNorm fold).  What is this
// kernel's own:
//
//   * One row tile per wave.  A tile never spans two clouds; the rows past n of a cloud's last tile are zero-filled in LDS (nothing is
//     read for them) and never stored.  The row builder (fp_rows.h, shared with the backward) stores along the column, like the
//     epilogue: the odd stride serves both.
//   * The contraction order inside a block of 8 is K_QUADS (k = k0 + 4 h + i), so unstaged weights with cin a multiple of 8 (every shape of
//     pointnet_2) are one global_load_dwordx4 per lane and block.
//   * The last layer stores its relu'd accumulators straight to `out` (for a fixed register the 32 lanes of a half write 128 contiguous
//     bytes of one output row).
//   * A 384-wide input tile plus a 256-wide output tile (fp3 of pointnet_2) is 82 KB per wave and 320 + 256 (fp2) 74 KB: ONE wave per
//     workgroup for fp3 (B * 256 rows in all: the layer is small), two for fp2, four for fp1.  Layer 0's input is NOT built in K chunks.
//   * No reduction ties a wave to a group, so the waves of a workgroup (up to 128 rows) share the staged weights.
#include "fp_rows.h"

namespace ampnet {

__global__ __launch_bounds__(256) void fp_forward_kernel(MlpPlan p, const float *__restrict__ points1, int D1, const float *__restrict__ points2,
                                                        int D2, int n, int s, const int32_t *__restrict__ idx, const float *__restrict__ dist2,
                                                        int k, const float *__restrict__ fold, int tiles_per_cloud, int n_tiles,
                                                        float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MlpLds m = mlp_lds(p, 32, s_mem, wave);
    mlp_stage_weights(p, m.s_w, tid, 64 * p.nw);
    __syncthreads();
    const int kp0 = p.kp[0], cout_last = p.cout[p.L - 1];
    for (int tile = blockIdx.x * p.nw + wave; tile < n_tiles; tile += gridDim.x * p.nw) {
        const int cloud_i = tile / tiles_per_cloud, row0 = (tile - cloud_i * tiles_per_cloud) * 32;
        const int rows = min(32, n - row0);
        fp_build_rows(m.tile_a, p.ld_a, kp0, points1, D1, points2, D2, n, s, idx, dist2, k, cloud_i, row0, rows, lane);      // fp_rows.h
        wave_lds_sync();
        mlp_run<K_QUADS>(p, 32, m.s_w, m.tile_a, m.tile_b, fold, FpStore{cout_last, rows},
                         out + ((size_t)cloud_i * n + row0) * cout_last, lane);
        // the next tile's rows overwrite tile A: every read of this tile is done (the last layer's results went out from registers)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// fp_forward_kernel on `st` with the plan and LDS bytes of mlp_plan_build and a fold that is already (being) written on `st`: the eval entry
// point below folds the running statistics, the train-mode forward (feature_propagation_train.hip) the batch's.
int fp_forward_launch(const char *what, const MlpPlan &p, int lds, const float *points1, int D1, const float *points2, int D2, int n_clouds, int n,
                      int s, const int32_t *idx, const float *dist2, int k, const float *fold, float *out, hipStream_t st)
{
    static bool attr_set = false;
    int rc = mlp_allow_full_lds(what, reinterpret_cast<const void *>(fp_forward_kernel), attr_set);
    if (rc != AMPNET_OK) return rc;
    const int tiles_per_cloud = (int)(((long long)n + 31) / 32), n_tiles = n_clouds * tiles_per_cloud;
    hipLaunchKernelGGL(fp_forward_kernel, dim3(mlp_grid(n_tiles, p.nw)), dim3(64 * p.nw), lds, st, p, points1, D1, points2, D2, n, s, idx, dist2, k,
                       fold, tiles_per_cloud, n_tiles, out);
    return check_launch("fp_forward_kernel");
}

}  // namespace ampnet

extern "C" int ampnet_fp_forward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                                     const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host,
                                     int L, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(points2 && idx && dist2 && params_host && cout_host && eps_host && out, "ampnet_fp_forward_f32: null pointer");
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && s >= 1, "ampnet_fp_forward_f32: bad shape n_clouds=%d n=%d s=%d", n_clouds, n, s);
    AMPNET_REQUIRE(k >= 1 && k <= 3 && k <= s, "ampnet_fp_forward_f32: k=%d must be 1, 2 or 3 and <= s=%d", k, s);
    AMPNET_REQUIRE(L >= 1 && L <= AMPNET_FP_MAX_LAYERS, "ampnet_fp_forward_f32: L=%d layers, the kernel is built for 1 .. %d", L, AMPNET_FP_MAX_LAYERS);
    AMPNET_REQUIRE(D1 >= 0 && (D1 == 0) == (points1 == nullptr), "ampnet_fp_forward_f32: points1 must be NULL exactly when D1 = 0 (D1=%d)", D1);
    AMPNET_REQUIRE(D2 >= 1 && D1 <= AMPNET_FP_MAX_CIN && D2 <= AMPNET_FP_MAX_CIN && D1 + D2 <= AMPNET_FP_MAX_CIN,
                   "ampnet_fp_forward_f32: cin_0 = D1 + D2 = %d + %d must be in [1, %d] with D2 >= 1", D1, D2, AMPNET_FP_MAX_CIN);
    AMPNET_REQUIRE(workspace && workspace_bytes >= AMPNET_FP_WORKSPACE_BYTES, "ampnet_fp_forward_f32: workspace of %zu bytes, need %d",
                   workspace_bytes, AMPNET_FP_WORKSPACE_BYTES);
    const int tiles_per_cloud = (int)(((long long)n + 31) / 32);
    // (the tile counter of a wave steps by at most 4096 past the last tile: keep that inside an int)
    AMPNET_REQUIRE((long long)n_clouds * tiles_per_cloud <= 0x7fff0000LL, "ampnet_fp_forward_f32: n_clouds * ceil(n / 32) = %lld tiles exceed %lld",
                   (long long)n_clouds * tiles_per_cloud, 0x7fff0000LL);
    MlpPlan p;
    MlpFold f;
    const int lds = mlp_plan_build("ampnet_fp_forward_f32", D1 + D2, 32, params_host, cout_host, eps_host, L, p, f);
    if (!lds) return AMPNET_E_ARG;
    int rc = mlp_fold_launch(p, f, static_cast<float *>(workspace), (hipStream_t)stream);
    if (rc != AMPNET_OK) return rc;
    return fp_forward_launch("ampnet_fp_forward_f32", p, lds, points1, D1, points2, D2, n_clouds, n, s, idx, dist2, k, static_cast<float *>(workspace),
                             out, (hipStream_t)stream);
}
