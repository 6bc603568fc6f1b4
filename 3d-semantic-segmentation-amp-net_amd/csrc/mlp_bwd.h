// mlp_bwd.h -- what the backwards of the two fused PointNet++ layers share (feature_propagation_bwd.hip, set_abstraction_bwd.hip; the
// kernels and their launchers: mlp_bwd.hip): the split-K GEMM dW_l = dz_l^T x_l over rows kept in the workspace, its ordered reduce,
// the finalize kernel that turns the workgroups' per-channel partial sums into dbeta, dgamma and dbias, the chunk rule, the common part of
// the workspace layout, and the device code all four backwards (eval and train-mode) run on a wave's 32-row tile: the row stores and loads
// between LDS and the workspace and dx = dz W (mlp_dgrad); and the recompute-and-mask step of the frozen-statistics backwards that have no
// max to undo (fpb_recompute: feature propagation, and conv1 of the segmentation head, seg_head_bwd.hip).  The raw accumulator they recompute is the forward's, fused_mlp.h's
// mlp_accumulate, where the lane map and the two contraction orders are defined.
#pragma once
#include "fused_mlp.h"

namespace ampnet {

constexpr int FPB_MAX_CHUNKS = 256;       // split-K chunks of fp_wgrad_kernel
constexpr int FPB_MIN_CHUNK_ROWS = 64;

struct FpBwdFin {
    float *dbias[MLP_MAX_LAYERS], *dgamma[MLP_MAX_LAYERS], *dbeta[MLP_MAX_LAYERS];
};

// the rows of dW's contraction in chunks of max(64, ceil(M / 256) rounded up to 8)
inline void fpb_chunk_rule(long long M, int &chunk_rows, int &chunks)
{
    const long long per = (M + FPB_MAX_CHUNKS - 1) / FPB_MAX_CHUNKS;
    chunk_rows = (int)((per + 7) / 8 * 8);
    if (chunk_rows < FPB_MIN_CHUNK_ROWS) chunk_rows = FPB_MIN_CHUNK_ROWS;
    chunks = (int)((M + chunk_rows - 1) / chunk_rows);
}

// dW [cout][cin] = dz [M][cout]^T xs [M][ldxs] (ldxs = cin rounded up to 32, the padding zeros): fp_wgrad_kernel into
// wpart [chunks][cout][ldxs], then fp_wgrad_reduce_kernel, both on `st`
int fpb_wgrad_launch(const float *dz, int cout, const float *xs, int cin, int ldxs, long long M, int chunk_rows, int chunks, float *wpart,
                     float *dW, hipStream_t st);
// fp_bwd_finalize_kernel on `st`: parts [n_parts][2 sum_c] (a row per workgroup: sum dy, then sum dy a, layer l's channels from
// fold_off[l] / 2) -> g
int fpb_finalize_launch(const MlpPlan &p, const MlpFold &f, const FpBwdFin &g, const float *fold, const float *parts, int n_parts, int sum_c,
                        hipStream_t st);

// The clouds of a backward.  Uniform: n_clouds clouds of n points and s centres (set abstraction) or coarse points (feature propagation),
// cloud_off null.  Ragged (bwd_clouds_ragged): q clouds of unequal size packed back to back, cloud b being the rows cloud_off[b] ..
// cloud_off[b + 1] (a device table), each with s_cloud centres or coarse points; every phase but the last gather takes the packed array as
// ONE cloud: n_clouds = 1, n = total, s = q s_cloud.
struct BwdClouds {
    int n_clouds, n, s;
    const int32_t *cloud_off;
    int q, s_cloud;
};
// checks the ragged shape (`what` opens every message) and fills c
int bwd_clouds_ragged(const char *what, const int32_t *cloud_off, int n_clouds, int total, int s, BwdClouds &c);

// The part of the workspace every backward lays out the same way (float offsets, each a multiple of 64): the workgroups' partial rows, per
// layer its input rows x_l [M][ldxs_l] and dz_l [M][cout_l], the dx_0 rows the gather reads, and the split-K partials of dW.
struct MlpBwdLayout {
    int sum_c;                                                 // sum of cout_l
    int cin[MLP_MAX_LAYERS], ldxs[MLP_MAX_LAYERS];             // ldxs: cin_l rounded up to 32 (zeros)
    size_t off_parts, off_xs[MLP_MAX_LAYERS], off_dz[MLP_MAX_LAYERS], off_dx0, off_wpart, floats;
};

// Checks every cout (`what` opens the message) and fills lay from float offset `off` on: grid partial rows of 2 sum_c floats, M rows per
// layer, dx0_cols columns of dx_0, `chunks` partials of the largest dW.
int mlp_bwd_layout(const char *what, size_t off, int cin0, int dx0_cols, long long M, int grid, int chunks, const int *cout_host, int L,
                   MlpBwdLayout &lay);

// the wave's tile [.][ld] -> rows < rows of a global array with row stride ldg (columns past `valid` as zeros)
__device__ __forceinline__ void fpb_store_rows(const float *tile, int ld, int valid, float *__restrict__ g, int ldg, int rows, int lane)
{
    for (int t = 0; t < rows; ++t)
        for (int c = lane; c < ldg; c += 64) g[(size_t)t * ldg + c] = c < valid ? tile[t * ld + c] : 0.0f;
}

// rows < rows of a global array with row stride ldg -> the wave's tile, `width` columns (a multiple of 8, <= ldg); the rows past `rows` zero.
// A lane reads the words fpb_store_rows made it write (column c belongs to lane c % 64 in both), so a wave may load what it stored itself
// without a fence.
__device__ __forceinline__ void fpb_load_rows(float *tile, int ld, int width, const float *g, int ldg, int rows, int lane)
{
    for (int t = 0; t < 32; ++t)
        for (int c = lane; c < width; c += 64) tile[t * ld + c] = t < rows ? g[(size_t)t * ldg + c] : 0.0f;
}

// fpb_load_rows for rows another KERNEL stored: the elements spread over all 64 lanes (32 width is a multiple of 64)
__device__ __forceinline__ void fpb_load_rows_flat(float *tile, int ld, int width, const float *__restrict__ g, int ldg, int rows, int lane)
{
    for (int e = lane; e < 32 * width; e += 64) {
        const int t = e / width, c = e - t * width;
        tile[t * ld + c] = t < rows ? g[(size_t)t * ldg + c] : 0.0f;
    }
}

// The accumulators of layer l on the wave's tile x, NT column tiles from n0, in the forward's order (mlp_accumulate<NT, K_QUADS, VEC>), and the
// frozen-statistics backward's epilogue (feature_propagation_bwd.hip, seg_head_bwd.hip): d [32][ldd] holds dx_l on entry (dout != nullptr: the
// rows come from global memory, row stride cout) and dz on exit.
template <int NT, bool VEC>
__device__ __forceinline__ void fpb_recompute(const float *x, int ldx, const float *__restrict__ w, int cin, int kp, int cout, int n0,
                                              const float *__restrict__ scale, const float *__restrict__ shift, float *d, int ldd,
                                              const float *__restrict__ dout, int rows, float *__restrict__ dz_ws, float *part_b,
                                              float *part_g, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    mlp_accumulate<NT, K_QUADS, VEC>(acc, mlp_operand<K_QUADS>(x, ldx, r, h), w, cin, cin, kp, n0, r, h);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        const float sc = scale[col], sh = shift[col];
        float sb = 0.0f, sg = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mlp_acc_row(i, h);
            const float a = acc[t][i];
            float din;
            if (dout) din = row < rows ? dout[(size_t)row * cout + col] : 0.0f;
            else din = d[row * ldd + col];
            const float dy = fmaf(a, sc, sh) > 0.0f ? din : 0.0f;
            sb += dy;
            sg = fmaf(dy, a, sg);
            const float dzv = dy * sc;
            d[row * ldd + col] = dzv;
            if (row < rows) dz_ws[(size_t)row * cout + col] = dzv;
        }
        const float ob = __shfl_down(sb, 32), og = __shfl_down(sg, 32);
        if (h == 0) {                             // (this lane alone ever touches these two words of the workgroup's partials)
            part_b[col] += sb + ob;
            part_g[col] += sg + og;
        }
    }
}

// dx = dz W for NT column tiles of the layer's INPUT from c0: dz [32][ldd] in LDS, w [cout][cin] global.  The forward's lane map with cin
// and cout exchanged: lane (r, h) supplies row r of dz and column c0 + 32 t + r of W; o ascending in blocks of 8, k-step i < 4 of lane half
// h takes o = o0 + 2 i + h.  Results go to tile `xo` (l >= 1) or, xo == nullptr (layer 0), the rows < rows leave the kernel: columns < D1
// to dp1 [.][D1], columns [D1, cin) to dx0 [.][D2].  DROP_D1: nobody wants the first D1 columns and dp1 is null (set abstraction's three
// coordinates); a flag and not a test of dp1, so that each caller keeps one condition per element, as its kernel was tuned.
template <int NT, bool DROP_D1 = false>
__device__ __forceinline__ void mlp_dgrad(const float *d, int ldd, const float *__restrict__ w, int cin, int cout, int c0, float *xo, int ldxo,
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
            const int row = mlp_acc_row(i, h);
            if (xo) {
                if (c < cin) xo[row * ldxo + c] = acc[t][i];
            } else if (DROP_D1) {
                if (row < rows && c >= D1 && c < cin) dx0[(size_t)row * D2 + c - D1] = acc[t][i];
            } else if (row < rows) {
                if (c < D1) dp1[(size_t)row * D1 + c] = acc[t][i];
                else if (c < cin) dx0[(size_t)row * D2 + c - D1] = acc[t][i];
            }
        }
    }
}

}  // namespace ampnet
