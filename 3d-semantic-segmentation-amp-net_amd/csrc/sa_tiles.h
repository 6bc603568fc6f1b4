// sa_tiles.h -- what the set-abstraction kernels share (set_abstraction.hip: the eval forward; set_abstraction_bwd.hip: the backward with the
// running statistics frozen; set_abstraction_train.hip: batch statistics): the gather of a group's rows into a wave's LDS tile, the
// backwards' launch sizes and workspace layout, and the launchers of the forward's kernel and of the dfeats gather.  The device code of a
// tile (the raw accumulator, dx = dz W, the row stores and loads) is fused_mlp.h's and mlp_bwd.h's.
#pragma once
#include "mlp_bwd.h"

namespace ampnet {

constexpr int SAB_MAX_GRID = 2048;        // workgroups (= rows of the partials array) of the one-wave-per-group kernels

// The forward's gather of a WHOLE group g: the R rows [xyz[idx_t] - xyz[centre] (3), feats[idx_t] (D)] of group_idx[g][:] into `tile`
// [R][ldt], kp0 columns each (zeros past cin0).  Lane t holds the point of row t; the rows past nsample REPEAT row 0, which changes no max.
// Element e = (row, column) with the columns fastest, so a row's features load contiguously.
__device__ __forceinline__ void sa_gather_group(float *tile, int ldt, int R, int kp0, int cin0, const float *__restrict__ xyz, int n, int ld,
                                                const int32_t *__restrict__ centres, int s, const int32_t *__restrict__ group_idx, int nsample,
                                                const float *__restrict__ feats, int D, int g, int lane)
{
    const int cloud_i = g / s;
    const float *cloud = xyz + (size_t)cloud_i * n * ld;
    const float *fcloud = feats ? feats + (size_t)cloud_i * n * D : nullptr;
    const int cidx = min(max(centres[g], 0), n - 1);
    const float cx = cloud[(size_t)cidx * ld], cy = cloud[(size_t)cidx * ld + 1], cz = cloud[(size_t)cidx * ld + 2];
    const int my_idx = min(max(group_idx[(size_t)g * nsample + (lane < nsample ? lane : 0)], 0), n - 1);
    for (int e = lane; e < R * kp0; e += 64) {
        const int t = e / kp0, c = e - t * kp0;
        const int j = __shfl(my_idx, t);
        float v = 0.0f;
        if (c < 3) v = cloud[(size_t)j * ld + c] - (c == 0 ? cx : c == 1 ? cy : cz);
        else if (c < cin0) v = fcloud[(size_t)j * D + (c - 3)];
        tile[t * ldt + c] = v;
    }
}

// the eval forwards' last-layer epilogue (set_abstraction.hip, set_abstraction_msg.hip): the per-column max over the group's rows, stored to
// this centre's output row
struct SaMax {
    __device__ static float init() { return -INFINITY; }
    __device__ static void put(float &mx, float *, int, int, float v) { mx = fmaxf(mx, v); }
    __device__ static void done(float mx, float *dst, int col, int h)
    {
        const float o = fmaxf(mx, __shfl_xor(mx, 32));
        if (h == 0) dst[col] = o;
    }
};

// The 32-row-tile variant: rows m0 .. m0 + 31 of a group (group_g: its nsample indices; cx, cy, cz: its centre) into `tile` [32][ld].
// Unlike sa_gather_group it ZEROES the rows past `rows` instead of repeating row 0: its callers sum over the rows they store.
__device__ __forceinline__ void sat_gather_rows(float *tile, int ld, int kp0, int cin0, const float *__restrict__ cloud, int ldc,
                                                const float *__restrict__ fcloud, int D, int n, const int32_t *__restrict__ group_g, float cx,
                                                float cy, float cz, int m0, int rows, int lane)
{
    const int my_idx = min(max(group_g[(lane & 31) < rows ? m0 + (lane & 31) : 0], 0), n - 1);
    for (int e = lane; e < 32 * kp0; e += 64) {                // (32 kp0 is a multiple of 64: every lane makes the same trips)
        const int t = e / kp0, c = e - t * kp0;
        const int j = __shfl(my_idx, t);
        float v = 0.0f;
        if (t < rows) {
            if (c < 3) v = cloud[(size_t)j * ldc + c] - (c == 0 ? cx : c == 1 ? cy : cz);
            else if (c < cin0) v = fcloud[(size_t)j * D + (c - 3)];
        }
        tile[t * ld + c] = v;
    }
}

// what both entry points derive from the shape: the launch sizes, the LDS tiles and the workspace layout
struct SaBwdShape : MlpBwdLayout {
    long long M;
    int R, n_groups, grid, chunk_rows, chunks, lds_floats;
    int off_x[MLP_MAX_LAYERS + 1], ld_x[MLP_MAX_LAYERS + 1];
};

// checks the shape against the forward's limits and the LDS limit of sa_backward_kernel (`what` opens every message) and fills sh
int sab_shape(const char *what, int D, int n_clouds, int s, int nsample, const int *cout_host, int L, SaBwdShape &sh);
// sa_forward_kernel (set_abstraction.hip) on `st`, reading scale and shift of every layer from `fold` (plan.fold_off)
int sa_forward_launch(const char *what, const MlpPlan &p, int lds, const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                      const int32_t *group_idx, int nsample, const float *feats, int D, const float *fold, float *out, hipStream_t st);
// sa_dfeats_kernel (set_abstraction_bwd.hip) on `st`: dfeats [n_clouds, n, D] from the dx_0 rows [n_clouds s nsample][D] as an ordered gather
int sa_dfeats_launch(const float *dx0, int D, int n_clouds, int n, int s, int nsample, const int32_t *group_idx, float *dfeats, hipStream_t st);

}  // namespace ampnet
