// set_abstraction_msg.hip -- K set-abstraction branches around the same centres (multi-scale grouping), eval mode, in ONE launch (C ABI:
// ampnet_sa_msg_forward_f32).
//
// Branch k is ampnet_sa_forward_f32 on its own group_idx and layers: the same plan (mlp_plan_build for R = 32 / 64), the same gather
// (sa_gather_group) and the same layer code (mlp_run<K_PAIRS> with SaMax), so its values are that entry point's bit for bit.  What is this
// kernel's own:
//
//   * The K plans travel by value in the kernel arguments (about 150 bytes each) and are read in place, through a reference into the
//     argument segment: a copy into a local would be indexed by the layer and land in scratch.
//   * A WORKGROUP belongs to one branch, found from blockIdx.x (wave-uniform): branch k has the workgroups [wg_begin, wg_begin + wg_count),
//     wg_count = mlp_grid(n_groups, nw_k).  It stages that branch's weights once and walks that branch's groups with that branch's nw.
//   * The block is 64 x the largest nw and the dynamic LDS the largest need.  All of a block's threads stage the weights; the waves
//     beyond the branch's own nw then leave (a branch has fewer waves only when its tiles are too large for more: there is no LDS for them).
//   * The destination row is out + g C + col_off: the branches write disjoint column slices of the concatenated output, no atomics.
#include "sa_tiles.h"

namespace ampnet {

struct SaMsgBranch {
    MlpPlan p;
    const int32_t *group_idx;
    int nsample, col_off, wg_begin, wg_count, fold_off;     // fold_off: floats from the workspace's start to this branch's fold region
};

struct SaMsgArgs {
    SaMsgBranch b[AMPNET_SA_MSG_MAX_SCALES];
    int K;
};

__global__ __launch_bounds__(256) void sa_msg_forward_kernel(SaMsgArgs a, const float *__restrict__ xyz, int n, int ld,
                                                            const int32_t *__restrict__ centres, int s, const float *__restrict__ feats, int D,
                                                            const float *__restrict__ fold_all, int n_groups, int C, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int k = 0;
    for (int j = 1; j < a.K; ++j)
        if ((int)blockIdx.x >= a.b[j].wg_begin) k = j;
    const SaMsgBranch &b = a.b[k];
    const MlpPlan &p = b.p;
    const MlpLds m = mlp_lds(p, p.R, s_mem, wave);
    mlp_stage_weights(p, m.s_w, tid, blockDim.x);
    __syncthreads();
    if (wave >= p.nw) return;
    const float *fold = fold_all + b.fold_off;
    const int32_t *__restrict__ group_idx = b.group_idx;
    const int cin0 = p.cin[0], kp0 = p.kp[0], nsample = b.nsample;
    float *dst0 = out + b.col_off;
    for (int g = ((int)blockIdx.x - b.wg_begin) * p.nw + wave; g < n_groups; g += b.wg_count * p.nw) {
        sa_gather_group(m.tile_a, p.ld_a, p.R, kp0, cin0, xyz, n, ld, centres, s, group_idx, nsample, feats, D, g, lane);
        wave_lds_sync();
        mlp_run<K_PAIRS>(p, p.R, m.s_w, m.tile_a, m.tile_b, fold, SaMax{}, dst0 + (size_t)g * C, lane);
        // the next centre's gather overwrites tile A: every read of this centre is done (the last layer's results are in registers)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace ampnet

extern "C" size_t ampnet_sa_msg_forward_workspace_bytes(int K)
{
    using namespace ampnet;
    if (K < 1 || K > AMPNET_SA_MSG_MAX_SCALES) {
        fail(AMPNET_E_ARG, "ampnet_sa_msg_forward_workspace_bytes: K=%d branches, the kernel is built for 1 .. %d", K, AMPNET_SA_MSG_MAX_SCALES);
        return 0;
    }
    return (size_t)K * AMPNET_SA_WORKSPACE_BYTES;
}

extern "C" int ampnet_sa_msg_forward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                                         const int32_t *const *group_idx_host, const int *nsample_host, const float *feats, int D,
                                         const float *const *params_host, const int *cout_host, const float *eps_host, const int *L_host, int K,
                                         float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_sa_msg_forward_f32";
    AMPNET_REQUIRE(xyz && centres && group_idx_host && nsample_host && params_host && cout_host && eps_host && L_host && out, "%s: null pointer", what);
    AMPNET_REQUIRE(K >= 1 && K <= AMPNET_SA_MSG_MAX_SCALES, "%s: K=%d branches, the kernel is built for 1 .. %d", what, K, AMPNET_SA_MSG_MAX_SCALES);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld >= 3 && s >= 1, "%s: bad shape n_clouds=%d n=%d ld=%d s=%d", what, n_clouds, n, ld, s);
    AMPNET_TRY(sa_check_feats(what, feats, D, nullptr));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, (size_t)K * AMPNET_SA_WORKSPACE_BYTES));
    const int n_groups = n_clouds * s;
    SaMsgArgs a = {};
    MlpFold f[AMPNET_SA_MSG_MAX_SCALES];
    a.K = K;
    int layer0 = 0, C = 0, grid = 0, lds = 0, nw_max = 1;
    for (int k = 0; k < K; ++k) {
        char who[64];
        snprintf(who, sizeof who, "%s: branch %d", what, k);
        const int nsample = nsample_host[k], L = L_host[k];
        AMPNET_REQUIRE(group_idx_host[k], "%s: null group_idx", who);
        AMPNET_TRY(sa_check_limits(what, D, n_clouds, s, nsample, L, false, who));
        SaMsgBranch &b = a.b[k];
        const int need = mlp_plan_build(who, 3 + D, nsample <= 32 ? 32 : 64, params_host + 6 * layer0, cout_host + layer0, eps_host + layer0, L,
                                        b.p, f[k]);
        if (!need) return AMPNET_E_ARG;
        b.group_idx = group_idx_host[k];
        b.nsample = nsample;
        b.col_off = C;
        b.wg_begin = grid;
        b.wg_count = mlp_grid(n_groups, b.p.nw);
        b.fold_off = k * (AMPNET_SA_WORKSPACE_BYTES / (int)sizeof(float));
        C += cout_host[layer0 + L - 1];
        grid += b.wg_count;
        lds = need > lds ? need : lds;
        nw_max = b.p.nw > nw_max ? b.p.nw : nw_max;
        layer0 += L;
    }
    float *fold_all = static_cast<float *>(workspace);
    for (int k = 0; k < K; ++k) {
        AMPNET_TRY(mlp_fold_launch(a.b[k].p, f[k], fold_all + a.b[k].fold_off, (hipStream_t)stream));
    }
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sa_msg_forward_kernel), attr_set));
    hipLaunchKernelGGL(sa_msg_forward_kernel, dim3(grid), dim3(64 * nw_max), lds, (hipStream_t)stream, a, xyz, n, ld, centres, s, feats, D,
                       fold_all, n_groups, C, out);
    return check_launch("sa_msg_forward_kernel");
}
