// fp_rows.h -- the input rows of a feature-propagation layer, built into a wave's LDS tile: ONE copy of the interpolation arithmetic for the
// forward (feature_propagation.hip), the eval backward (feature_propagation_bwd.hip) and the train-mode passes
// (feature_propagation_train.hip), which rebuild the rows instead of reading stored ones and have to get the forward's bits to find the
// forward's ReLU masks.  Also the launcher of the forward's kernel, which the eval and the train-mode forward share.
#pragma once
#include "fused_mlp.h"

namespace ampnet {

// the inverse-distance weights of one fine point from its k squared distances: r_q = 1 / (d_q + 1e-8f), w_q = r_q / ((r_0 + r_1) + r_2)
__device__ __forceinline__ void fp_interp_weights(const float *__restrict__ d, int k, float (&wk)[3])
{
    float rk[3] = {0.0f, 0.0f, 0.0f};
    for (int q = 0; q < k; ++q) rk[q] = 1.0f / (d[q] + 1e-8f);
    float sum = rk[0];
    if (k > 1) sum += rk[1];
    if (k > 2) sum += rk[2];
    wk[0] = wk[1] = wk[2] = 0.0f;
    for (int q = 0; q < k; ++q) wk[q] = rk[q] / sum;
}

// Rows row0 .. row0 + 31 of cloud `cloud_i` into `tile` [32][ld], kp0 columns each (zeros past cin0 = D1 + D2): the rows past `rows` are
// zero-filled and nothing is read for them.  Lane t (and t + 32) holds the neighbours and weights of row t; indices are clamped into the
// coarse cloud.  The caller orders the stores before its reads (wave_lds_sync).  T: the tile's element type, float or (the bf16 forward,
// feature_propagation_bf16.hip) __bf16: the value is formed in fp32 either way and rounded once by the store.
template <class T>
__device__ __forceinline__ void fp_build_rows(T *tile, int ld, int kp0, const float *__restrict__ points1, int D1,
                                              const float *__restrict__ points2, int D2, int n, int s, const int32_t *__restrict__ idx,
                                              const float *__restrict__ dist2, int k, int cloud_i, int row0, int rows, int lane)
{
    const int cin0 = D1 + D2;
    const float *p1 = points1 ? points1 + ((size_t)cloud_i * n + row0) * D1 : nullptr;
    const float *p2 = points2 + (size_t)cloud_i * s * D2;
    int nb[3] = {0, 0, 0};
    float wk[3] = {0.0f, 0.0f, 0.0f};
    if ((lane & 31) < rows) {
        const size_t o = ((size_t)cloud_i * n + row0 + (lane & 31)) * k;
        for (int q = 0; q < k; ++q) nb[q] = min(max(idx[o + q], 0), s - 1);
        fp_interp_weights(dist2 + o, k, wk);
    }
    // the columns fastest across the lanes: a row's features load contiguously
#pragma unroll 2
    for (int t = 0; t < 32; ++t) {
        const int j0 = __shfl(nb[0], t), j1 = __shfl(nb[1], t), j2 = __shfl(nb[2], t);
        const float w0 = __shfl(wk[0], t), w1 = __shfl(wk[1], t), w2 = __shfl(wk[2], t);
        const float *f0 = p2 + (size_t)j0 * D2, *f1 = p2 + (size_t)j1 * D2, *f2 = p2 + (size_t)j2 * D2;
        for (int c = lane; c < kp0; c += 64) {
            float v = 0.0f;
            if (t < rows) {
                if (c < D1) {
                    v = p1[(size_t)t * D1 + c];
                } else if (c < cin0) {
                    v = w0 * f0[c - D1];
                    if (k > 1) v = fmaf(w1, f1[c - D1], v);
                    if (k > 2) v = fmaf(w2, f2[c - D1], v);
                }
            }
            tile[t * ld + c] = (T)v;
        }
    }
}

// the forwards' last-layer epilogue (feature_propagation.hip, feature_propagation_bf16.hip): rows < rows of the tile go to `dst` (global,
// row stride ldo)
struct FpStore {
    int ldo, rows;
    __device__ static float init() { return 0.0f; }
    __device__ void put(float &, float *dst, int row, int col, float v) const
    {
        if (row < rows) dst[(size_t)row * ldo + col] = v;
    }
    __device__ static void done(float, float *, int, int) {}
};

// fp_forward_kernel (feature_propagation.hip) on `st`, reading scale and shift of every layer from `fold` (plan.fold_off)
int fp_forward_launch(const char *what, const MlpPlan &p, int lds, const float *points1, int D1, const float *points2, int D2, int n_clouds, int n,
                      int s, const int32_t *idx, const float *dist2, int k, const float *fold, float *out, hipStream_t st);

}  // namespace ampnet
