// mlp_bwd.h -- what the backwards of the two fused PointNet++ layers share (feature_propagation_bwd.hip, set_abstraction_bwd.hip; the
// kernels and their launchers: mlp_bwd.hip): the split-K GEMM dW_l = dz_l^T x_l over rows kept in the workspace, its ordered reduce,
// the finalize kernel that turns the workgroups' per-channel partial sums into dbeta, dgamma and dbias, and the chunk rule.
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

// the wave's tile [.][ld] -> rows < rows of a global array with row stride ldg (columns past `valid` as zeros)
__device__ __forceinline__ void fpb_store_rows(const float *tile, int ld, int valid, float *__restrict__ g, int ldg, int rows, int lane)
{
    for (int t = 0; t < rows; ++t)
        for (int c = lane; c < ldg; c += 64) g[(size_t)t * ldg + c] = c < valid ? tile[t * ld + c] : 0.0f;
}

}  // namespace ampnet
