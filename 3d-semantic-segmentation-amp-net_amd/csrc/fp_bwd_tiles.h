// fp_bwd_tiles.h -- what the two feature-propagation backwards share (feature_propagation_bwd.hip: running statistics frozen;
// feature_propagation_train.hip: batch statistics): the launch sizes, the workspace layout and the launcher of the dpoints2 gather.  The
// device code of a tile (the raw accumulator, dx = dz W, the row stores and loads) is fused_mlp.h's and mlp_bwd.h's.
#pragma once
#include "fp_rows.h"
#include "mlp_bwd.h"

namespace ampnet {

constexpr int FPB_MAX_GRID = 1024;        // workgroups (= rows of the partials array) of the one-wave-per-tile kernels

// what the backward entry points derive from the shape: the launch sizes and the workspace layout (float offsets, each a multiple of 64)
struct FpBwdShape : MlpBwdLayout {
    long long M;
    int tiles_per_cloud, n_tiles, grid, chunk_rows, chunks;
};

// checks the shape against the forward's limits (`what` opens every message) and fills sh
int fpb_shape(const char *what, int D1, int D2, int n_clouds, int n, const int *cout_host, int L, FpBwdShape &sh);
// fp_scatter_kernel on `st`: dpoints2 [n_clouds, s, D2] from the dx_0 rows [n_clouds n][D2] as an ordered gather
int fp_scatter_launch(const float *dx0, int D2, int n_clouds, int n, int s, const int32_t *idx, const float *dist2, int k, float *dpoints2,
                      hipStream_t st);

// the dpoints2 gather of c (mlp_bwd.h; s: coarse points) on `st`: fp_scatter_launch, or fp_scatter_ragged_kernel, which scans a coarse
// point's own cloud alone
int fp_gather_launch(const float *dx0, int D2, const BwdClouds &c, const int32_t *idx, const float *dist2, int k, float *dpoints2, hipStream_t st);

}  // namespace ampnet
