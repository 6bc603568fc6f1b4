// feature_propagation_bf16.hip -- the eval feature-propagation forward with its matrix products in bf16 (C ABI: ampnet_fp_forward_bf16).
//
// feature_propagation.hip's kernel around the bf16 core (fused_mlp_bf16.h): the same neighbours and interpolation weights, the same rows
// (fp_build_rows forms a row in fp32 and the store rounds it to bf16; rows past n are zeros and never stored), one row tile of 32 fine
// points per wave, the same store epilogue (FpStore, on the last layer's fp32 values) and the same limits.  The rounding model is stated
// with ampnet_sa_forward_bf16 in include/ampnet_hip.h.  The workspace holds the BatchNorm fold (sa_fold_kernel, unchanged) and behind it
// every layer's weights as bf16 rows, converted once per call (mlp_bf16_weights_kernel): halved, two of fp1's three 128-wide layers are
// staged in LDS beside four waves' tiles (4 x 17 KB + 2 x 34 KB of 160 KB), where the fp32 kernel reads every layer through L2.
#include "fp_rows.h"
#include "fused_mlp_bf16.h"

namespace ampnet {

__global__ __launch_bounds__(256) void fp_forward_bf16_kernel(MlpPlanBf16 p, const float *__restrict__ points1, int D1,
                                                             const float *__restrict__ points2, int D2, int n, int s,
                                                             const int32_t *__restrict__ idx, const float *__restrict__ dist2, int k,
                                                             const float *__restrict__ fold, const __bf16 *__restrict__ wb, int tiles_per_cloud,
                                                             int n_tiles, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) __bf16 s_mem_bf16[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MlpLdsBf16 m = mlp_bf16_lds(p, 32, s_mem_bf16, wave);
    mlp_bf16_stage_weights(p, m.s_w, wb, tid, 64 * p.nw);
    __syncthreads();
    const int kp0 = p.kp[0], cout_last = p.cout[p.L - 1];
    for (int tile = blockIdx.x * p.nw + wave; tile < n_tiles; tile += gridDim.x * p.nw) {
        const int cloud_i = tile / tiles_per_cloud, row0 = (tile - cloud_i * tiles_per_cloud) * 32;
        const int rows = min(32, n - row0);
        fp_build_rows(m.tile_a, p.ld_a, kp0, points1, D1, points2, D2, n, s, idx, dist2, k, cloud_i, row0, rows, lane);
        wave_lds_sync();
        mlp_bf16_run(p, 32, m.s_w, wb, m.tile_a, m.tile_b, fold, FpStore{cout_last, rows}, out + ((size_t)cloud_i * n + row0) * cout_last, lane);
        // the next tile's rows overwrite tile A: every read of this tile is done (the last layer's results went out from registers)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// what both entry points check of the shape (the limits of ampnet_fp_forward_f32); the bytes of the weight region behind the fold, 0
// after a failure
static size_t fp_bf16_weight_bytes(const char *what, int D1, int D2, int n_clouds, int n, const int *cout_host, int L)
{
    MLP_BF16_REQUIRE(cout_host, "%s: null pointer", what);
    MLP_BF16_REQUIRE(n_clouds >= 1 && n >= 1, "%s: bad shape n_clouds=%d n=%d", what, n_clouds, n);
    MLP_BF16_REQUIRE(L >= 1 && L <= AMPNET_FP_MAX_LAYERS, "%s: L=%d layers, the kernel is built for 1 .. %d", what, L, AMPNET_FP_MAX_LAYERS);
    MLP_BF16_REQUIRE(D1 >= 0 && D2 >= 1 && D1 <= AMPNET_FP_MAX_CIN && D2 <= AMPNET_FP_MAX_CIN && D1 + D2 <= AMPNET_FP_MAX_CIN,
                     "%s: cin_0 = D1 + D2 = %d + %d must be in [1, %d] with D2 >= 1", what, D1, D2, AMPNET_FP_MAX_CIN);
    const long long tiles = (long long)n_clouds * (((long long)n + 31) / 32);
    // (the tile counter of a wave steps by at most 4096 past the last tile: keep that inside an int)
    MLP_BF16_REQUIRE(tiles <= 0x7fff0000LL, "%s: n_clouds * ceil(n / 32) = %lld tiles exceed %lld", what, tiles, 0x7fff0000LL);
    return mlp_bf16_weight_bytes(what, D1 + D2, cout_host, L);
}

}  // namespace ampnet

extern "C" size_t ampnet_fp_forward_bf16_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L)
{
    using namespace ampnet;
    const size_t wbytes = fp_bf16_weight_bytes("ampnet_fp_forward_bf16_workspace_bytes", D1, D2, n_clouds, n, cout_host, L);
    return wbytes ? MLP_BF16_FOLD_BYTES + wbytes : 0;
}

extern "C" int ampnet_fp_forward_bf16(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                                      const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host,
                                      int L, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_fp_forward_bf16";
    AMPNET_REQUIRE(points2 && idx && dist2 && params_host && cout_host && eps_host && out, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && s >= 1, "%s: bad shape n_clouds=%d n=%d s=%d", what, n_clouds, n, s);
    AMPNET_REQUIRE(k >= 1 && k <= 3 && k <= s, "%s: k=%d must be 1, 2 or 3 and <= s=%d", what, k, s);
    AMPNET_REQUIRE(D1 >= 0 && (D1 == 0) == (points1 == nullptr), "%s: points1 must be NULL exactly when D1 = 0 (D1=%d)", what, D1);
    const size_t wbytes = fp_bf16_weight_bytes(what, D1, D2, n_clouds, n, cout_host, L);
    if (!wbytes) return AMPNET_E_ARG;
    AMPNET_REQUIRE(workspace && workspace_bytes >= MLP_BF16_FOLD_BYTES + wbytes, "%s: workspace of %zu bytes, need %zu", what, workspace_bytes,
                   MLP_BF16_FOLD_BYTES + wbytes);
    AMPNET_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", what);
    MlpPlan p32;
    MlpFold f;
    MlpPlanBf16 p;
    const int lds = mlp_bf16_plan_build(what, D1 + D2, 32, params_host, cout_host, eps_host, L, p32, f, p);
    if (!lds) return AMPNET_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    float *fold = static_cast<float *>(workspace);
    __bf16 *wb = reinterpret_cast<__bf16 *>(static_cast<char *>(workspace) + MLP_BF16_FOLD_BYTES);
    AMPNET_TRY(mlp_fold_launch(p32, f, fold, st));
    AMPNET_TRY(mlp_bf16_weights_launch(p, wb, st));
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(fp_forward_bf16_kernel), attr_set));
    const int tiles_per_cloud = (int)(((long long)n + 31) / 32), n_tiles = n_clouds * tiles_per_cloud;
    hipLaunchKernelGGL(fp_forward_bf16_kernel, dim3(mlp_grid(n_tiles, p.nw)), dim3(64 * p.nw), lds, st, p, points1, D1, points2, D2, n, s, idx,
                       dist2, k, fold, wb, tiles_per_cloud, n_tiles, out);
    return check_launch("fp_forward_bf16_kernel");
}
