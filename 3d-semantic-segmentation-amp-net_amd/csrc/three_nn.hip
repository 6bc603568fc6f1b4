// three_nn.hip -- the neighbour search of a PointNet++ feature-propagation layer (C ABI: ampnet_three_nn_f32).
//
// BUILD-DEFINED like knn.hip and ball_query.hip: the reference imports PointNetFeaturePropagation from a package it does not ship
// (pointnetAtt.py:4), so the spec is fixed in include/ampnet_hip.h and pinned by the build's own CPU restatement
// (tests/fp_ref.py: three_nn):
//     d(i, j) = float32 ((dx*dx + dy*dy) + dz*dz), one rounding per operation (compiled with -ffp-contract=off, the distance of knn.hip
//     and ball_query.hip); with k = min(3, s) fine point i gets the k coarse points j with the smallest (d, j), ascending;
//     idx[c][i][0..k) are those j, dist2[c][i][0..k) their d.
// Difference from the usual implementation: that one forms  -2 x.y + |x|^2 + |y|^2  as a matrix product and sorts it, so the neighbours it
// picks among NEARLY equal distances (and the order of exactly equal ones) depend on the library's GEMM and sort.  Here the distance is
// the difference form above and ties go to the lower index, on every machine.
//
// Mapping to CDNA4: the coarse cloud's coordinates sit in LDS as three planes (the plan of knn.hip, s * 12 bytes <= 144 KB), one LANE
// owns one fine point.  Every lane walks the coarse points in index order -- all lanes read the same LDS address, a broadcast -- and
// keeps its three smallest (d, j) sorted in registers; insertion on strict `<` leaves an equal distance behind the earlier index, which is
// the tie rule.  No atomics, no sort, no cross-lane traffic.
#include "common.h"

#pragma clang fp contract(off)

namespace ampnet {

constexpr int NN_THREADS = 256;

__global__ __launch_bounds__(NN_THREADS) void three_nn_kernel(const float *__restrict__ fine, int n, int ld1, const float *__restrict__ coarse,
                                                             int s, int ld2, int k, int blocks_per_cloud, int32_t *__restrict__ idx,
                                                             float *__restrict__ dist2)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[s], y[s], z[s]
    const int tid = threadIdx.x;
    const int cloud_i = blockIdx.x / blocks_per_cloud, blk = blockIdx.x - cloud_i * blocks_per_cloud;
    const float *cc = coarse + (size_t)cloud_i * s * ld2;
    for (int j = tid; j < s; j += NN_THREADS) {
        s_cloud[j] = cc[(size_t)j * ld2 + 0];
        s_cloud[s + j] = cc[(size_t)j * ld2 + 1];
        s_cloud[2 * s + j] = cc[(size_t)j * ld2 + 2];
    }
    __syncthreads();
    const long long i = (long long)blk * NN_THREADS + tid;
    if (i >= n) return;
    const float *p = fine + ((size_t)cloud_i * n + (size_t)i) * ld1;
    const float px = p[0], py = p[1], pz = p[2];
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
#pragma unroll 4
    for (int j = 0; j < s; ++j) {
        const float dx = px - s_cloud[j], dy = py - s_cloud[s + j], dz = pz - s_cloud[2 * s + j];
        const float d = (dx * dx + dy * dy) + dz * dz;
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
    const size_t o = ((size_t)cloud_i * n + (size_t)i) * k;
    idx[o] = i0;
    dist2[o] = d0;
    if (k > 1) {
        idx[o + 1] = i1;
        dist2[o + 1] = d1;
    }
    if (k > 2) {
        idx[o + 2] = i2;
        dist2[o + 2] = d2;
    }
}

}  // namespace ampnet

extern "C" int ampnet_three_nn_f32(const float *fine, int n_clouds, int n, int ld1, const float *coarse, int s, int ld2, int32_t *idx,
                                   float *dist2, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(fine && coarse && idx && dist2, "ampnet_three_nn_f32: null pointer");
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld1 >= 3 && ld2 >= 3, "ampnet_three_nn_f32: bad shape n_clouds=%d n=%d ld1=%d ld2=%d", n_clouds, n,
                   ld1, ld2);
    AMPNET_REQUIRE(s >= 1 && s <= AMPNET_THREE_NN_MAX_S, "ampnet_three_nn_f32: s=%d must be in [1, %d] (the coarse coordinates must fit LDS)", s,
                   AMPNET_THREE_NN_MAX_S);
    const int blocks_per_cloud = (int)(((long long)n + NN_THREADS - 1) / NN_THREADS);
    AMPNET_REQUIRE((long long)n_clouds * blocks_per_cloud <= 0x7fffffffLL, "ampnet_three_nn_f32: n_clouds * ceil(n / %d) = %lld exceeds 2^31 - 1",
                   NN_THREADS, (long long)n_clouds * blocks_per_cloud);
    const size_t lds = (size_t)s * 3 * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(three_nn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "ampnet_three_nn_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    const int k = s < 3 ? s : 3;
    hipLaunchKernelGGL(three_nn_kernel, dim3(n_clouds * blocks_per_cloud), dim3(NN_THREADS), lds, (hipStream_t)stream, fine, n, ld1, coarse, s, ld2,
                       k, blocks_per_cloud, idx, dist2);
    return check_launch("three_nn_kernel");
}
