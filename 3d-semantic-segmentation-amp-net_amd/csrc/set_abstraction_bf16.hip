// set_abstraction_bf16.hip -- the eval set-abstraction forward with its matrix products in bf16 (C ABI: ampnet_sa_forward_bf16).
//
// set_abstraction.hip's kernel around the bf16 core (fused_mlp_bf16.h): the same groups, the same gather (sa_gather_group forms a row in
// fp32 and the store rounds it to bf16), the same padding of nsample to R = 32 or 64 rows by repeating row 0, the same max epilogue
// (SaMax, on the last layer's fp32 values) and the same limits (sa_check_limits).  The rounding model is stated with the entry point in
// include/ampnet_hip.h.  The workspace holds the BatchNorm fold (sa_fold_kernel, unchanged) and behind it every layer's weights as bf16
// rows, converted once per call (mlp_bf16_weights_kernel).
#include "fused_mlp_bf16.h"
#include "sa_tiles.h"

namespace ampnet {

__global__ __launch_bounds__(256) void sa_forward_bf16_kernel(MlpPlanBf16 p, const float *__restrict__ xyz, int n, int ld,
                                                             const int32_t *__restrict__ centres, int s, const int32_t *__restrict__ group_idx,
                                                             int nsample, const float *__restrict__ feats, int D, const float *__restrict__ fold,
                                                             const __bf16 *__restrict__ wb, int n_groups, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) __bf16 s_mem_bf16[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MlpLdsBf16 m = mlp_bf16_lds(p, p.R, s_mem_bf16, wave);
    mlp_bf16_stage_weights(p, m.s_w, wb, tid, 64 * p.nw);
    __syncthreads();
    const int cin0 = p.cin[0], kp0 = p.kp[0], cout_last = p.cout[p.L - 1];
    for (int g = blockIdx.x * p.nw + wave; g < n_groups; g += gridDim.x * p.nw) {
        sa_gather_group(m.tile_a, p.ld_a, p.R, kp0, cin0, xyz, n, ld, centres, s, group_idx, nsample, feats, D, g, lane);
        wave_lds_sync();
        mlp_bf16_run(p, p.R, m.s_w, wb, m.tile_a, m.tile_b, fold, SaMax{}, out + (size_t)g * cout_last, lane);
        // the next centre's gather overwrites tile A: every read of this centre is done (the last layer's results are in registers)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// what both entry points check of the shape; the bytes of the weight region behind the fold, 0 after a failure
static size_t sa_bf16_weight_bytes(const char *what, int D, int n_clouds, int s, int nsample, const int *cout_host, int L)
{
    MLP_BF16_REQUIRE(cout_host, "%s: null pointer", what);
    MLP_BF16_REQUIRE(n_clouds >= 1 && s >= 1, "%s: bad shape n_clouds=%d s=%d", what, n_clouds, s);
    if (sa_check_limits(what, D, n_clouds, s, nsample, L, false) != AMPNET_OK) return 0;
    return mlp_bf16_weight_bytes(what, 3 + D, cout_host, L);
}

}  // namespace ampnet

extern "C" size_t ampnet_sa_forward_bf16_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L)
{
    using namespace ampnet;
    const size_t wbytes = sa_bf16_weight_bytes("ampnet_sa_forward_bf16_workspace_bytes", D, n_clouds, s, nsample, cout_host, L);
    return wbytes ? MLP_BF16_FOLD_BYTES + wbytes : 0;
}

extern "C" int ampnet_sa_forward_bf16(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                                      int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                                      const float *eps_host, int L, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_sa_forward_bf16";
    AMPNET_REQUIRE(xyz && centres && group_idx && params_host && cout_host && eps_host && out, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld >= 3 && s >= 1, "%s: bad shape n_clouds=%d n=%d ld=%d s=%d", what, n_clouds, n, ld, s);
    AMPNET_TRY(sa_check_feats(what, feats, D, nullptr));
    const size_t wbytes = sa_bf16_weight_bytes(what, D, n_clouds, s, nsample, cout_host, L);
    if (!wbytes) return AMPNET_E_ARG;
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, MLP_BF16_FOLD_BYTES + wbytes));
    AMPNET_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", what);
    MlpPlan p32;
    MlpFold f;
    MlpPlanBf16 p;
    const int lds = mlp_bf16_plan_build(what, 3 + D, nsample <= 32 ? 32 : 64, params_host, cout_host, eps_host, L, p32, f, p);
    if (!lds) return AMPNET_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    float *fold = static_cast<float *>(workspace);
    __bf16 *wb = reinterpret_cast<__bf16 *>(static_cast<char *>(workspace) + MLP_BF16_FOLD_BYTES);
    AMPNET_TRY(mlp_fold_launch(p32, f, fold, st));
    AMPNET_TRY(mlp_bf16_weights_launch(p, wb, st));
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sa_forward_bf16_kernel), attr_set));
    const int n_groups = n_clouds * s;
    hipLaunchKernelGGL(sa_forward_bf16_kernel, dim3(mlp_grid(n_groups, p.nw)), dim3(64 * p.nw), lds, st, p, xyz, n, ld, centres, s, group_idx,
                       nsample, feats, D, fold, wb, n_groups, out);
    return check_launch("sa_forward_bf16_kernel");
}
