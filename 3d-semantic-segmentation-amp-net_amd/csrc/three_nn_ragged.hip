// three_nn_ragged.hip -- three_nn.hip's neighbour search from fine clouds of UNEQUAL size to coarse clouds of equal size, in one launch
// (C ABI: ampnet_three_nn_ragged_f32): the search of the LAST feature-propagation layer of a PointNet++ whose input clouds differ in size.
//
// The fine clouds lie back to back in one [total, ld1] array, cloud b being the rows cloud_off[b] .. cloud_off[b + 1] (a device table, the
// layout of ampnet_fps_ragged_f32); every cloud has s coarse points, coarse [n_clouds, s, ld2].  Spec, distance and tie rule are
// three_nn.hip's (tests/fp_ref.py: three_nn on the cloud alone): with global_index = 0 idx and dist2 are bit for bit what
// ampnet_three_nn_f32 writes for that cloud; with 1 the stored index is b * s + j, so idx addresses coarse as ONE cloud of n_clouds * s
// points (what ampnet_fp_forward_f32 takes with n_clouds = 1).
//
// Mapping to CDNA4: three_nn_kernel's -- the cloud's coarse coordinates in LDS as three planes, one LANE per fine point, strict `<`
// insertion into three sorted registers.  The grid is (ceil(max_n / 256), n_clouds): a workgroup that lies wholly past its cloud's end
// returns before it stages anything -- all of it together, so no barrier is split.
#include "common.h"

#pragma clang fp contract(off)

namespace ampnet {

constexpr int NNR_THREADS = 256;                         // three_nn.hip: NN_THREADS

__global__ __launch_bounds__(NNR_THREADS) void three_nn_ragged_kernel(const float *__restrict__ fine, int ld1, const int32_t *__restrict__ cloud_off,
                                                                      int total, int max_n, const float *__restrict__ coarse, int s, int ld2, int k, int global_index,
                                                                      int32_t *__restrict__ idx, float *__restrict__ dist2)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[s], y[s], z[s]
    const int tid = threadIdx.x;
    const int cloud_i = blockIdx.y;
    const int row0 = cloud_off[cloud_i], n = min(cloud_off[cloud_i + 1] - row0, max_n);
    if (row0 < 0 || row0 > total - n) return;                            // (a table that leaves the array: nothing is read through it)
    if (blockIdx.x * NNR_THREADS >= n) return;                           // workgroup-uniform, like the line above
    const float *cc = coarse + (size_t)cloud_i * s * ld2;
    for (int j = tid; j < s; j += NNR_THREADS) {
        s_cloud[j] = cc[(size_t)j * ld2 + 0];
        s_cloud[s + j] = cc[(size_t)j * ld2 + 1];
        s_cloud[2 * s + j] = cc[(size_t)j * ld2 + 2];
    }
    __syncthreads();
    const int i = blockIdx.x * NNR_THREADS + tid;
    if (i >= n) return;
    const float *p = fine + ((size_t)row0 + (size_t)i) * ld1;
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
    const int add = global_index ? cloud_i * s : 0;
    const size_t o = ((size_t)row0 + (size_t)i) * k;
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

}  // namespace ampnet

extern "C" int ampnet_three_nn_ragged_f32(const float *fine, int ld1, const int32_t *cloud_off, int n_clouds, int total, int max_n,
                                          const float *coarse, int s, int ld2, int global_index, int32_t *idx, float *dist2, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_three_nn_ragged_f32";
    AMPNET_REQUIRE(fine && cloud_off && coarse && idx && dist2, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n_clouds <= 65535 && ld1 >= 3 && ld2 >= 3 && max_n >= 1 && total >= max_n,
                   "%s: bad shape n_clouds=%d (1 .. 65535) ld1=%d ld2=%d max_n=%d total=%d", what, n_clouds, ld1, ld2, max_n, total);
    AMPNET_REQUIRE(s >= 1 && s <= AMPNET_THREE_NN_MAX_S, "%s: s=%d must be in [1, %d] (the coarse coordinates must fit LDS)", what, s,
                   AMPNET_THREE_NN_MAX_S);
    const size_t lds = (size_t)s * 3 * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(three_nn_ragged_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
        attr_set = true;
    }
    const int k = s < 3 ? s : 3;
    hipLaunchKernelGGL(three_nn_ragged_kernel, dim3(cdiv(max_n, NNR_THREADS), n_clouds), dim3(NNR_THREADS), lds, (hipStream_t)stream, fine, ld1,
                       cloud_off, total, max_n, coarse, s, ld2, k, global_index ? 1 : 0, idx, dist2);
    return check_launch("three_nn_ragged_kernel");
}
