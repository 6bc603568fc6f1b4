// three_nn.hip -- the neighbour search of a PointNet++ feature-propagation layer (C ABI: ampnet_three_nn_f32; from fine clouds of UNEQUAL
// size in one launch: ampnet_three_nn_ragged_f32).
//
// BUILD-DEFINED like knn.hip and ball_query.hip: the reference imports PointNetFeaturePropagation from a package it does not ship
// (pointnetAtt.py:4), so the spec is fixed in include/ampnet_hip.h and pinned by the build's own CPU restatement
// (tests/fp_ref.py: three_nn):
//     d(i, j) = float32 ((dx*dx + dy*dy) + dz*dz), one rounding per operation (cloud_search.h: staged_dist2, the distance of knn.hip and
//     ball_query.hip); with k = min(3, s) fine point i gets the k coarse points j with the smallest (d, j), ascending;
//     idx[c][i][0..k) are those j, dist2[c][i][0..k) their d.
// Difference from the usual implementation: that one forms  -2 x.y + |x|^2 + |y|^2  as a matrix product and sorts it, so the neighbours it
// picks among NEARLY equal distances (and the order of exactly equal ones) depend on the library's GEMM and sort.  Here the distance is
// the difference form above and ties go to the lower index, on every machine.
//
// Mapping to CDNA4: the coarse cloud's coordinates sit in LDS as three planes (the plan of knn.hip, s * 12 bytes <= 144 KB), one LANE
// owns one fine point.  Every lane walks the coarse points in index order -- all lanes read the same LDS address, a broadcast -- and
// keeps its three smallest (d, j) sorted in registers; insertion on strict `<` leaves an equal distance behind the earlier index, which is
// the tie rule.  No atomics, no sort, no cross-lane traffic.  ONE walk (three_nn_point) serves both kernels.
//
// Ragged: the fine clouds lie back to back in one [total, ld1] array, cloud b being the rows cloud_off[b] .. cloud_off[b + 1] (a device
// table, the layout of ampnet_fps_ragged_f32); every cloud has s coarse points, coarse [n_clouds, s, ld2].  With global_index = 1 the
// stored index is b * s + j, so idx addresses coarse as ONE cloud of n_clouds * s points (what ampnet_fp_forward_f32 takes with
// n_clouds = 1).  The grid is (ceil(max_n / 256), n_clouds): a workgroup that lies wholly past its cloud's end returns before it stages
// anything -- all of it together, so no barrier is split.
#include "cloud_search.h"

namespace ampnet {

constexpr int NN_THREADS = 256;

// The k nearest of the s staged coarse points to the fine point at row `p` -> idx[o .. o + k) (plus `add`) and dist2[o .. o + k)
__device__ __forceinline__ void three_nn_point(const float *s_cloud, int s, const float *__restrict__ p, int k, size_t o, int add,
                                               int32_t *__restrict__ idx, float *__restrict__ dist2)
{
    const float px = p[0], py = p[1], pz = p[2];
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
#pragma unroll 4
    for (int j = 0; j < s; ++j) {
        const float d = staged_dist2(s_cloud, s, j, px, py, pz);
        if (d < d2) {
            if (d < d1) {
                d2 = d1;
                i2 = i1;
                if (d < d0) {
                    d1 = d0;
                    i1 = i0;
                    d0 = d;
                    i0 = j;
                } else {
                    d1 = d;
                    i1 = j;
                }
            } else {
                d2 = d;
                i2 = j;
            }
        }
    }
    idx[o] = i0 + add;
    dist2[o] = d0;
    if (k > 1) {
        idx[o + 1] = i1 + add;
        dist2[o + 1] = d1;
    }
    if (k > 2) {
        idx[o + 2] = i2 + add;
        dist2[o + 2] = d2;
    }
}

__global__ __launch_bounds__(NN_THREADS) void three_nn_kernel(const float *__restrict__ fine, int n, int ld1, const float *__restrict__ coarse,
                                                             int s, int ld2, int k, int blocks_per_cloud, int32_t *__restrict__ idx,
                                                             float *__restrict__ dist2)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[s], y[s], z[s]
    const int cloud_i = blockIdx.x / blocks_per_cloud, blk = blockIdx.x - cloud_i * blocks_per_cloud;
    stage_cloud<NN_THREADS>(s_cloud, coarse + (size_t)cloud_i * s * ld2, s, ld2);
    const long long i = (long long)blk * NN_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)cloud_i * n + (size_t)i;
    three_nn_point(s_cloud, s, fine + row * ld1, k, row * k, 0, idx, dist2);
}

__global__ __launch_bounds__(NN_THREADS) void three_nn_ragged_kernel(const float *__restrict__ fine, int ld1, const int32_t *__restrict__ cloud_off,
                                                                     int total, int max_n, const float *__restrict__ coarse, int s, int ld2, int k, int global_index,
                                                                     int32_t *__restrict__ idx, float *__restrict__ dist2)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[s], y[s], z[s]
    const int cloud_i = blockIdx.y;
    const int row0 = cloud_off[cloud_i], n = min(cloud_off[cloud_i + 1] - row0, max_n);
    if (row0 < 0 || row0 > total - n) return;                            // (a table that leaves the array: nothing is read through it)
    if (blockIdx.x * NN_THREADS >= n) return;                            // workgroup-uniform, like the line above
    stage_cloud<NN_THREADS>(s_cloud, coarse + (size_t)cloud_i * s * ld2, s, ld2);
    const int i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)row0 + (size_t)i;
    three_nn_point(s_cloud, s, fine + row * ld1, k, row * k, global_index ? cloud_i * s : 0, idx, dist2);
}

// The coarse side's rule of both entry points -> k
static int three_nn_k(const char *who, int s, int *k)
{
    AMPNET_REQUIRE(s >= 1 && s <= AMPNET_THREE_NN_MAX_S, "%s: s=%d must be in [1, %d] (the coarse coordinates must fit LDS)", who, s,
                   AMPNET_THREE_NN_MAX_S);
    *k = s < 3 ? s : 3;
    return AMPNET_OK;
}

}  // namespace ampnet

extern "C" int ampnet_three_nn_f32(const float *fine, int n_clouds, int n, int ld1, const float *coarse, int s, int ld2, int32_t *idx,
                                   float *dist2, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_three_nn_f32";
    AMPNET_REQUIRE(fine && coarse && idx && dist2, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld1 >= 3 && ld2 >= 3, "%s: bad shape n_clouds=%d n=%d ld1=%d ld2=%d", what, n_clouds, n, ld1, ld2);
    int k;
    AMPNET_TRY(three_nn_k(what, s, &k));
    const int blocks_per_cloud = (int)(((long long)n + NN_THREADS - 1) / NN_THREADS);
    AMPNET_REQUIRE((long long)n_clouds * blocks_per_cloud <= 0x7fffffffLL, "%s: n_clouds * ceil(n / %d) = %lld exceeds 2^31 - 1", what, NN_THREADS,
                   (long long)n_clouds * blocks_per_cloud);
    AMPNET_TRY(allow_dynamic_lds<three_nn_kernel>(CLOUD_LDS_MAX, what));
    hipLaunchKernelGGL(three_nn_kernel, dim3(n_clouds * blocks_per_cloud), dim3(NN_THREADS), (size_t)s * 12, (hipStream_t)stream, fine, n, ld1, coarse,
                       s, ld2, k, blocks_per_cloud, idx, dist2);
    return check_launch("three_nn_kernel");
}

extern "C" int ampnet_three_nn_ragged_f32(const float *fine, int ld1, const int32_t *cloud_off, int n_clouds, int total, int max_n,
                                          const float *coarse, int s, int ld2, int global_index, int32_t *idx, float *dist2, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_three_nn_ragged_f32";
    AMPNET_REQUIRE(fine && cloud_off && coarse && idx && dist2, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n_clouds <= 65535 && ld1 >= 3 && ld2 >= 3 && max_n >= 1 && total >= max_n,
                   "%s: bad shape n_clouds=%d (1 .. 65535) ld1=%d ld2=%d max_n=%d total=%d", what, n_clouds, ld1, ld2, max_n, total);
    int k;
    AMPNET_TRY(three_nn_k(what, s, &k));
    AMPNET_TRY(allow_dynamic_lds<three_nn_ragged_kernel>(CLOUD_LDS_MAX, what));
    hipLaunchKernelGGL(three_nn_ragged_kernel, dim3(cdiv(max_n, NN_THREADS), n_clouds), dim3(NN_THREADS), (size_t)s * 12, (hipStream_t)stream, fine,
                       ld1, cloud_off, total, max_n, coarse, s, ld2, k, global_index ? 1 : 0, idx, dist2);
    return check_launch("three_nn_ragged_kernel");
}
