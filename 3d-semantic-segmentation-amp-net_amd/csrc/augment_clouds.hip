// augment_clouds.hip -- the input pipeline of pn2_step.train_loop_clouds in one kernel: what augment.hip is for the window batch, for
// clouds of UNEQUAL size taken as the cluster files hold them.  The clusters go up once as they were concatenated ([total_in, 10]: nine
// features + the ASPRS class code) and ONE launch writes what the set-abstraction blocks and the loss consume:
//     the padding of short clouds      (utils.pad_cloud_sizes: padded row j of a cloud of n points is its row j % n)
//     one point shuffle per cloud      (shuffle_data, utils.py:607-617 -- here a keyed bijection that is never stored: kernels.h cloud_perm)
//     the z-rotation of x, y, z        (rotate_point_cloud_z, utils.py:582-604, as augment_kernel does it: float64 product, rounded once)
//     the label look-up                (amp_test._label_lut: 15 -> 1, 14 -> 2, 3 / 4 -> 3, 5 -> 4, else 0; padding rows -1)
// It replaces a [:, :9] copy, a long / clamp / index chain and, with a short cloud, two gathers, a where and three small uploads.
//
// Memory-bound gather: 40 B read and 44 .. 48 B written per row.  A workgroup owns 256 consecutive OUTPUT rows.  Every thread gathers
// one source row (five 8-byte loads: a row of `raw` starts at a multiple of 40 B), the nine features pass through LDS (row stride 9
// dwords: odd, so the 32 banks of a write are distinct) and leave as one contiguous run of 256 * 9 floats written 16 B per lane -- the
// run starts at a multiple of 256 * 36 B.  targets and src are one element per thread, contiguous across the wave.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ampnet {

constexpr int CI_ROWS = 256;      // output rows (= threads) per workgroup

__device__ inline long long cloud_label(float code)
{
    long long c = (long long)code;                 // Tensor.long(): truncation towards zero
    c = c < 0 ? 0 : (c > 255 ? 255 : c);
    return c == 15 ? 1 : c == 14 ? 2 : (c == 3 || c == 4) ? 3 : c == 5 ? 4 : 0;
}

__global__ __launch_bounds__(CI_ROWS) void cloud_input_kernel(const float *__restrict__ raw, const int *__restrict__ in_off,
                                                              const int *__restrict__ out_off, int Q, int total_out, uint32_t seed,
                                                              uint32_t step, int permute, int rotate, double c, double s,
                                                              float *__restrict__ rows, long long *__restrict__ targets,
                                                              int *__restrict__ src_out)
{
    __shared__ __attribute__((aligned(16))) float tile[CI_ROWS * 9];
    const int i0 = blockIdx.x * CI_ROWS;            // first output row of the workgroup (total_out < 2^31)
    const long long i = (long long)i0 + threadIdx.x;
    // the cloud of row i0: the last b with out_off[b] <= i0 (wave-uniform); a thread then walks forward to its own cloud
    int lo = 0, hi = Q - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (out_off[mid] <= i0) lo = mid; else hi = mid - 1;
    }
    if (i < total_out) {
        int b = lo;
        while (b + 1 < Q && i >= out_off[b + 1]) ++b;
        const int j = (int)(i - out_off[b]);
        const int r0 = in_off[b], n = in_off[b + 1] - r0;
        const int own = j < n ? j : j % n;
        const int row = r0 + (permute ? (int)cloud_perm(cloud_perm_key(seed, step, (uint32_t)b), (uint32_t)n, (uint32_t)own) : own);
        const float2 *p = reinterpret_cast<const float2 *>(raw + (size_t)row * 10);
        float v[10];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float2 t = p[k];
            v[2 * k] = t.x;
            v[2 * k + 1] = t.y;
        }
        if (rotate) {
            const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
            v[0] = (float)((x * c + y * (-s)) + z * 0.0);                 // np.dot(xyz, rot), column by column, in float64
            v[1] = (float)((x * s + y * c) + z * 0.0);
            v[2] = (float)((x * 0.0 + y * 0.0) + z * 1.0);
        }
        float *t = tile + threadIdx.x * 9;
#pragma unroll
        for (int f = 0; f < 9; ++f) t[f] = v[f];
        targets[i] = j < n ? cloud_label(v[9]) : -1LL;
        if (src_out) src_out[i] = row;
    }
    __syncthreads();
    const int live = min(CI_ROWS, total_out - i0) * 9;                   // floats of the workgroup's run
    float *dst = rows + (size_t)i0 * 9;                                   // 16-byte aligned: i0 * 36 B, i0 a multiple of 256
    const int n4 = live >> 2;
    for (int k = threadIdx.x; k < n4; k += CI_ROWS)
        reinterpret_cast<float4 *>(dst)[k] = reinterpret_cast<const float4 *>(tile)[k];
    for (int k = (n4 << 2) + threadIdx.x; k < live; k += CI_ROWS) dst[k] = tile[k];
}

}  // namespace ampnet

extern "C" int ampnet_cloud_input_f32(const float *raw, const int32_t *in_off, const int32_t *out_off, int Q, long long total_in,
                                      long long total_out, uint32_t seed, uint32_t step, int permute, int rotate, double cos_a,
                                      double sin_a, float *rows, long long *targets, int32_t *src, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(raw && in_off && out_off && rows && targets, "ampnet_cloud_input_f32: null pointer");
    AMPNET_REQUIRE(Q >= 1, "ampnet_cloud_input_f32: Q=%d clouds, at least one is needed", Q);
    AMPNET_REQUIRE(total_in >= Q && total_out >= total_in && total_out < (1LL << 31),
                   "ampnet_cloud_input_f32: bad totals: %lld input rows, %lld output rows for %d clouds (every cloud holds a point, padding "
                   "only adds rows, below 2^31)", total_in, total_out, Q);
    AMPNET_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                   "ampnet_cloud_input_f32: raw must be 8-byte and rows 16-byte aligned");
    hipLaunchKernelGGL(cloud_input_kernel, dim3((unsigned)((total_out + CI_ROWS - 1) / CI_ROWS)), dim3(CI_ROWS), 0, (hipStream_t)stream, raw,
                       in_off, out_off, Q, (int)total_out, seed, step, permute, rotate, cos_a, sin_a, rows, targets, src);
    return check_launch("cloud_input_kernel");
}
