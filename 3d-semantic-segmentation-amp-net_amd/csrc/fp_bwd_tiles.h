// fp_bwd_tiles.h -- what the two feature-propagation backwards share (feature_propagation_bwd.hip: running statistics frozen;
// feature_propagation_train.hip: batch statistics): the raw accumulators of a layer in the forward's contraction order, dx = dz W in its
// lane map, the workspace layout and the launcher of the dpoints2 gather.
#pragma once
#include "fp_rows.h"
#include "mlp_bwd.h"

namespace ampnet {

constexpr int FPB_MAX_GRID = 1024;        // workgroups (= rows of the partials array) of the one-wave-per-tile kernels

// The raw accumulators a = W x of NT column tiles from n0 on the wave's tile x [32][ldx], in the forward's order (mlp_tiles<NT, K_QUADS,
// VEC>: k ascending in blocks of 8, k-step i < 4 of lane half h takes k = k0 + 4 h + i).  w [cout][cin] global; VEC: 16-byte aligned rows,
// cin == kp.  Lane (r, h) ends with column n0 + 32 t + r of rows (i & 3) + 8 (i >> 2) + 4 h in acc[t][i].
template <int NT, bool VEC>
__device__ __forceinline__ void fpb_accumulate(const float *x, int ldx, const float *__restrict__ w, int cin, int kp, int n0, f32x16 (&acc)[NT],
                                               int lane)
{
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    const float *xr = x + r * ldx + 4 * h;
    for (int k0 = 0; k0 < kp; k0 += 8) {
        float av[4], bv[NT][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = xr[k0 + i];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float *wr = w + (size_t)(n0 + 32 * t + r) * cin + k0 + 4 * h;
            if (VEC) {
                const float4 q = *reinterpret_cast<const float4 *>(wr);
                bv[t][0] = q.x;
                bv[t][1] = q.y;
                bv[t][2] = q.z;
                bv[t][3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) bv[t][i] = k0 + 4 * h + i < cin ? wr[i] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
}

// dx = dz W for NT column tiles of the layer's INPUT from c0: dz [32][ldd] in LDS, w [cout][cin] global.  Results go to tile `xo` (l >= 1)
// or, xo == nullptr, to dpoints1 / the dx_0 rows of the workspace (layer 0; D1 + D2 = cin).
template <int NT>
__device__ __forceinline__ void fpb_dgrad(const float *d, int ldd, const float *__restrict__ w, int cin, int cout, int c0, float *xo, int ldxo,
                                          float *__restrict__ dp1, int D1, float *__restrict__ dx0, int D2, int rows, int lane)
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
            } else if (row < rows) {
                if (c < D1) dp1[(size_t)row * D1 + c] = acc[t][i];
                else if (c < cin) dx0[(size_t)row * D2 + c - D1] = acc[t][i];
            }
        }
    }
}

// what the backward entry points derive from the shape: the launch sizes and the workspace layout (float offsets, each a multiple of 64)
struct FpBwdShape {
    long long M;
    int tiles_per_cloud, n_tiles, grid, chunk_rows, chunks, sum_c;
    int cin[MLP_MAX_LAYERS], ldxs[MLP_MAX_LAYERS];
    size_t off_parts, off_xs[MLP_MAX_LAYERS], off_dz[MLP_MAX_LAYERS], off_dx0, off_wpart, floats;
};

// checks the shape against the forward's limits (`what` opens every message) and fills sh
int fpb_shape(const char *what, int D1, int D2, int n_clouds, int n, const int *cout_host, int L, FpBwdShape &sh);
// fp_scatter_kernel on `st`: dpoints2 [n_clouds, s, D2] from the dx_0 rows [n_clouds n][D2] as an ordered gather
int fp_scatter_launch(const float *dx0, int D2, int n_clouds, int n, int s, const int32_t *idx, const float *dist2, int k, float *dpoints2,
                      hipStream_t st);

}  // namespace ampnet
