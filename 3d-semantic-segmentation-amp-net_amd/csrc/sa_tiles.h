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
// Element e = (row, column) with the columns fastest, so a row's features load contiguously.  T: the tile's element type, float or (the
// bf16 forward, set_abstraction_bf16.hip) __bf16: the value is formed in fp32 either way and rounded once by the store.
template <class T>
__device__ __forceinline__ void sa_gather_group(T *tile, int ldt, int R, int kp0, int cin0, const float *__restrict__ xyz, int n, int ld,
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
        tile[t * ldt + c] = (T)v;
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

// The last layer's max WITH ITS ROW, one column of one lane: what the backwards and the whole-cloud forward keep where SaMax keeps a float.
// THE TIE RULE, stated here and nowhere else: of the rows that attain the largest y = relu(fma(a, scale, shift)) the LOWEST wins.  A lane
// offers its rows in ascending order (row tiles ascending, mlp_acc_row(i, h) ascending in i) and put() takes a row only on a strict >, so
// an equal later row never replaces an earlier one; merge_halves() joins the two lane halves of a column with one __shfl_xor(., 32) per
// member and hands a tie to the lower row, after which both halves hold the same winner.  Rows that are bit-identical copies of an earlier
// row (tile padding, the slots ball query filled by repeating its first member) therefore never win.  The forward's `arg`, the backward's
// routing of dout and the Python references' check_argmax all rest on this rule.  `a` is the winner's raw accumulator; a caller that never
// reads it (the whole-cloud forward) pays nothing for it.
struct SaArgMax {
    float best;
    int row;                              // (between the floats: the order in which hipcc emits sa_backward_kernel's selects, as before)
    float a;
    __device__ __forceinline__ void init() { best = -INFINITY; row = 0; a = 0.0f; }
    __device__ __forceinline__ void put(float a_, float y, int row_)
    {
        if (y > best) {
            best = y;
            row = row_;
            a = a_;
        }
    }
    __device__ __forceinline__ void merge_halves()
    {
        const float ob = __shfl_xor(best, 32), oa = __shfl_xor(a, 32);
        const int orow = __shfl_xor(row, 32);
        if (ob > best || (ob == best && orow < row)) {
            best = ob;
            row = orow;
            a = oa;
        }
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

// The host rules that several entry points state, each ONCE (set_abstraction.hip).  `what`, the entry point's name, opens the message; the
// result is AMPNET_OK or the failure's code with ampnet_last_error set.
// The limits: n_clouds * count below 2^31 (count = s, the groups; group_all: n, the rows), nsample (not with group_all), L, 3 + D.
// `who` names the branch whose nsample and L these are where that is not the entry point (multi-scale grouping).
int sa_check_limits(const char *what, int D, int n_clouds, int count, int nsample, int L, bool group_all, const char *who = nullptr);
// the features: feats NULL exactly when D = 0, dfeats (a forward passes nullptr) NULL when D = 0
int sa_check_feats(const char *what, const float *feats, int D, const float *dfeats);
// the cloud of the grouped backwards and the train forward, n >= 1 and ld >= 3, then sa_check_feats.  (The eval forwards refuse n and ld
// in one message with n_clouds and s, group_all words its own: those lines stay where they are, ahead of sa_check_feats.)
int sa_check_cloud(const char *what, int n, int ld, const float *feats, int D, const float *dfeats);
// the host tables of a backward: no null among the 6 L parameters (params_host = nullptr: mlp_plan_build will say so under the same
// name) nor among the 4 L gradient pointers
int sa_check_tables(const char *what, const float *const *params_host, float *const *grads_host, int L);
int sa_check_workspace(const char *what, const void *workspace, size_t workspace_bytes, size_t need);

// checks the shape against the forward's limits and the LDS limit of sa_backward_kernel (`what` opens every message) and fills sh
int sab_shape(const char *what, int D, int n_clouds, int s, int nsample, const int *cout_host, int L, SaBwdShape &sh);
// sa_forward_kernel (set_abstraction.hip) on `st`, reading scale and shift of every layer from `fold` (plan.fold_off)
int sa_forward_launch(const char *what, const MlpPlan &p, int lds, const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                      const int32_t *group_idx, int nsample, const float *feats, int D, const float *fold, float *out, hipStream_t st);
// sa_dfeats_kernel (set_abstraction_bwd.hip) on `st`: dfeats [n_clouds, n, D] from the dx_0 rows [n_clouds s nsample][D] as an ordered gather
int sa_dfeats_launch(const float *dx0, int D, int n_clouds, int n, int s, int nsample, const int32_t *group_idx, float *dfeats, hipStream_t st);

// the dfeats gather of c (mlp_bwd.h; s: centres) on `st`: sa_dfeats_launch, or sa_dfeats_ragged_kernel, which scans the groups of a point's
// own cloud alone
int sa_gather_launch(const float *dx0, int D, const BwdClouds &c, int nsample, const int32_t *group_idx, float *dfeats, hipStream_t st);

}  // namespace ampnet
