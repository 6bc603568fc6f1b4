// sa_tiles.h -- what the two set-abstraction backwards share (set_abstraction_bwd.hip: running statistics frozen;
// set_abstraction_train.hip: batch statistics): the raw accumulators of a layer in the forward's contraction order, dx = dz W in its lane
// map, the workspace layout, and the launchers of the forward's kernel and of the dfeats gather.
#pragma once
#include "mlp_bwd.h"

namespace ampnet {

constexpr int SAB_MAX_GRID = 2048;        // workgroups (= rows of the partials array) of the one-wave-per-group kernels

// the accumulators of NT column tiles from n0 on the 32 rows whose operand pointer is xr = x + (m0 + r) ldx + h: the forward's
// mlp_tiles<NT, K_PAIRS, false> on weights read from global memory
template <int NT>
__device__ __forceinline__ void sab_accumulate(f32x16 (&acc)[NT], const float *xr, const float *__restrict__ w, int cin, int kp, int n0, int r,
                                               int h)
{
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    for (int k0 = 0; k0 < kp; k0 += 8) {
        float av[4], bv[NT][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = xr[k0 + 2 * i];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float *wr = w + (size_t)(n0 + 32 * t + r) * cin + k0 + h;
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[t][i] = k0 + h + 2 * i < cin ? wr[2 * i] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
}

// dx = dz W for NT column tiles of the layer's INPUT from c0 on the 32 rows of d [32][ldd] (fpb_dgrad's lane map and order: o ascending
// in blocks of 8, k-step i of lane half h takes o = o0 + 2 i + h).  Results go to tile `xo` (l >= 1) or, xo == nullptr, columns
// [3, cin) of the rows < rows to dx0 [.][D] (layer 0).
template <int NT>
__device__ __forceinline__ void sab_dgrad(const float *d, int ldd, const float *__restrict__ w, int cin, int cout, int c0, float *xo, int ldxo,
                                          float *__restrict__ dx0, int D, int rows, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    const float *dr = d + r * ldd + h;
    for (int o0 = 0; o0 < cout; o0 += 8) {
        float av[4], bv[NT][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = dr[o0 + 2 * i];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = c0 + 32 * t + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[t][i] = c < cin ? w[(size_t)(o0 + 2 * i + h) * cin + c] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = c0 + 32 * t + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
            if (xo) {
                if (c < cin) xo[row * ldxo + c] = acc[t][i];
            } else if (row < rows && c >= 3 && c < cin) {
                dx0[(size_t)row * D + c - 3] = acc[t][i];
            }
        }
    }
}

// what both entry points derive from the shape: the launch sizes, the LDS tiles and the workspace layout (float offsets, multiples of 64)
struct SaBwdShape {
    long long M;
    int R, n_groups, grid, chunk_rows, chunks, sum_c, lds_floats;
    int cin[MLP_MAX_LAYERS], ldxs[MLP_MAX_LAYERS], off_x[MLP_MAX_LAYERS + 1], ld_x[MLP_MAX_LAYERS + 1];
    size_t off_parts, off_xs[MLP_MAX_LAYERS], off_dz[MLP_MAX_LAYERS], off_dx0, off_wpart, floats;
};

// checks the shape against the forward's limits and the LDS limit of sa_backward_kernel (`what` opens every message) and fills sh
int sab_shape(const char *what, int D, int n_clouds, int s, int nsample, const int *cout_host, int L, SaBwdShape &sh);
// sa_forward_kernel (set_abstraction.hip) on `st`, reading scale and shift of every layer from `fold` (plan.fold_off)
int sa_forward_launch(const char *what, const MlpPlan &p, int lds, const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                      const int32_t *group_idx, int nsample, const float *feats, int D, const float *fold, float *out, hipStream_t st);
// sa_dfeats_kernel (set_abstraction_bwd.hip) on `st`: dfeats [n_clouds, n, D] from the dx_0 rows [n_clouds s nsample][D] as an ordered gather
int sa_dfeats_launch(const float *dx0, int D, int n_clouds, int n, int s, int nsample, const int32_t *group_idx, float *dfeats, hipStream_t st);

}  // namespace ampnet
