// set_abstraction.hip -- one PointNet++ set-abstraction layer in eval mode, fused (C ABI: ampnet_sa_forward_f32).
//
// For centre i of cloud c the group is the nsample rows  [xyz[idx_t] - xyz[centre_i] (3), feats[idx_t] (D)]  of group_idx[c][i][:];
// every layer computes relu(bn_eval(W row + b)) and the output is the per-channel max over the rows.  Nothing grouped reaches HBM:
// a WAVE owns a centre, gathers its rows straight into its own LDS tile and keeps them there through all layers (fused_mlp.h: the lane
// map, the LDS layout, the ping-pong, the weight staging and the BatchNorm fold).  What is this kernel's own:
//
//   * nsample is padded to R = 32 or 64 rows by repeating row 0, which cannot change the max; the one or two row tiles share a layer's
//     scale, shift and running maxima.
//   * The contraction order inside a block of 8 is K_PAIRS (k = k0 + 2 i + h); weights that are not staged are read dword by dword.
//   * The last layer writes nothing to LDS: its relu'd accumulators are reduced over their 16 registers and the two lane halves (the
//     row dimension) and lanes h = 0 store the maxima.
#include "sa_tiles.h"

namespace ampnet {

__global__ __launch_bounds__(256) void sa_forward_kernel(MlpPlan p, const float *__restrict__ xyz, int n, int ld, const int32_t *__restrict__ centres,
                                                        int s, const int32_t *__restrict__ group_idx, int nsample,
                                                        const float *__restrict__ feats, int D, const float *__restrict__ fold,
                                                        int n_groups, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MlpLds m = mlp_lds(p, p.R, s_mem, wave);
    mlp_stage_weights(p, m.s_w, tid, 64 * p.nw);
    __syncthreads();
    const int cin0 = p.cin[0], kp0 = p.kp[0], cout_last = p.cout[p.L - 1];
    for (int g = blockIdx.x * p.nw + wave; g < n_groups; g += gridDim.x * p.nw) {
        sa_gather_group(m.tile_a, p.ld_a, p.R, kp0, cin0, xyz, n, ld, centres, s, group_idx, nsample, feats, D, g, lane);
        wave_lds_sync();
        mlp_run<K_PAIRS>(p, p.R, m.s_w, m.tile_a, m.tile_b, fold, SaMax{}, out + (size_t)g * cout_last, lane);
        // the next centre's gather overwrites tile A: every read of this centre is done (the last layer's results are in registers)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

int sa_forward_launch(const char *what, const MlpPlan &p, int lds, const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                      const int32_t *group_idx, int nsample, const float *feats, int D, const float *fold, float *out, hipStream_t st)
{
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sa_forward_kernel), attr_set));
    const int n_groups = n_clouds * s;
    hipLaunchKernelGGL(sa_forward_kernel, dim3(mlp_grid(n_groups, p.nw)), dim3(64 * p.nw), lds, st, p, xyz, n, ld, centres, s, group_idx, nsample,
                       feats, D, fold, n_groups, out);
    return check_launch("sa_forward_kernel");
}

// ---- the host rules of the set-abstraction entry points, each stated once (sa_tiles.h says who calls what) ----------------------------

int sa_check_limits(const char *what, int D, int n_clouds, int count, int nsample, int L, bool group_all, const char *who)
{
    if (!who) who = what;
    const long long total = (long long)n_clouds * count;
    AMPNET_REQUIRE(total <= 0x7fffffffLL, "%s: n_clouds * %s = %lld %s exceed 2^31 - 1", what, group_all ? "n" : "s", total, group_all ? "rows" : "groups");
    if (!group_all)
        AMPNET_REQUIRE(nsample >= 1 && nsample <= AMPNET_SA_MAX_NSAMPLE, "%s: nsample=%d must be in [1, %d]", who, nsample, AMPNET_SA_MAX_NSAMPLE);
    AMPNET_REQUIRE(L >= 1 && L <= AMPNET_SA_MAX_LAYERS, "%s: L=%d layers, the kernel is built for 1 .. %d", who, L, AMPNET_SA_MAX_LAYERS);
    AMPNET_REQUIRE(D >= 0 && 3 + D <= AMPNET_SA_MAX_CIN, "%s: cin_0 = 3 + D = %d exceeds %d", what, 3 + D, AMPNET_SA_MAX_CIN);
    return AMPNET_OK;
}

int sa_check_feats(const char *what, const float *feats, int D, const float *dfeats)
{
    AMPNET_REQUIRE(D >= 0 && (D == 0) == (feats == nullptr), "%s: feats must be NULL exactly when D = 0 (D=%d)", what, D);
    AMPNET_REQUIRE(D > 0 || dfeats == nullptr, "%s: dfeats must be NULL when D = 0", what);
    return AMPNET_OK;
}

int sa_check_cloud(const char *what, int n, int ld, const float *feats, int D, const float *dfeats)
{
    AMPNET_REQUIRE(n >= 1 && ld >= 3, "%s: bad shape n=%d ld=%d", what, n, ld);
    return sa_check_feats(what, feats, D, dfeats);
}

int sa_check_tables(const char *what, const float *const *params_host, float *const *grads_host, int L)
{
    if (params_host)
        for (int q = 0; q < 6 * L; ++q) AMPNET_REQUIRE(params_host[q], "%s: null parameter %d of layer %d", what, q % 6, q / 6);
    for (int q = 0; q < 4 * L; ++q) AMPNET_REQUIRE(grads_host[q], "%s: null gradient pointer %d of layer %d", what, q % 4, q / 4);
    return AMPNET_OK;
}

int sa_check_workspace(const char *what, const void *workspace, size_t workspace_bytes, size_t need)
{
    AMPNET_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu", what, workspace_bytes, need);
    return AMPNET_OK;
}

}  // namespace ampnet

extern "C" int ampnet_sa_forward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                                     int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                                     const float *eps_host, int L, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_sa_forward_f32";
    AMPNET_REQUIRE(xyz && centres && group_idx && params_host && cout_host && eps_host && out, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld >= 3 && s >= 1, "%s: bad shape n_clouds=%d n=%d ld=%d s=%d", what, n_clouds, n, ld, s);
    AMPNET_TRY(sa_check_feats(what, feats, D, nullptr));
    AMPNET_TRY(sa_check_limits(what, D, n_clouds, s, nsample, L, false));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, AMPNET_SA_WORKSPACE_BYTES));
    MlpPlan p;
    MlpFold f;
    const int lds = mlp_plan_build(what, 3 + D, nsample <= 32 ? 32 : 64, params_host, cout_host, eps_host, L, p, f);
    if (!lds) return AMPNET_E_ARG;
    float *fold = static_cast<float *>(workspace);
    AMPNET_TRY(mlp_fold_launch(p, f, fold, (hipStream_t)stream));
    return sa_forward_launch(what, p, lds, xyz, n_clouds, n, ld, centres, s, group_idx, nsample, feats, D, fold, out, (hipStream_t)stream);
}
