// ball_query_ragged.hip -- ball_query.hip's grouping for clouds of UNEQUAL size in one launch (C ABI: ampnet_ball_query_ragged_f32).
//
// The clouds lie back to back in one [total, ld] array; cloud b is the rows cloud_off[b] .. cloud_off[b + 1] (a device table, the layout of
// ampnet_fps_ragged_f32) and has the same s centres as every other cloud, given relative to its own first row.  Spec, distance, membership
// rule, order and padding are ball_query.hip's (tests/sa_ref.py: ball_query on the cloud alone): with global_index = 0 the lists are bit for
// bit what ampnet_ball_query_f32 writes for that cloud; with 1 every stored index has cloud_off[b] added, so the lists address the packed
// array as ONE cloud (what ampnet_sa_forward_f32 takes with n_clouds = 1).
//
// Mapping to CDNA4: ball_query_kernel's -- the cloud's three coordinate planes in LDS, one WAVE per centre, ballot + mbcnt slots, no sort,
// no atomic.  The cloud is blockIdx.y and its length comes from the table.  The dynamic LDS of the launch is sized by the LARGEST cloud
// (max_n * 12 bytes), so the workgroups per CU -- the occupancy -- are those of the largest cloud for every cloud of the call; a cloud
// stages and walks only its own n points.  (1100 .. 4000 points, the clusters of a file: 13 .. 47 KB of the CU's 160 KB, and the 16 waves
// of a workgroup bound the residency before LDS does.  Callers whose sizes differ by an order of magnitude can bucket them as
// fps_indices_ragged does; tools/prof_pn2_ragged.py measures the unbucketed call.)
#include "common.h"

#pragma clang fp contract(off)

namespace ampnet {

constexpr int BQR_WAVES = 16;                            // ball_query.hip: BQ_WAVES

__global__ __launch_bounds__(64 * BQR_WAVES) void ball_query_ragged_kernel(const float *__restrict__ rows, int ld, const int32_t *__restrict__ cloud_off,
                                                                           int total, int max_n, const int32_t *__restrict__ centres, int s, float r2, int nsample,
                                                                           int centres_per_block, int global_index, int32_t *__restrict__ out,
                                                                           int32_t *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[n], y[n], z[n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cloud_i = blockIdx.y;
    const int row0 = cloud_off[cloud_i];
    const int n = min(cloud_off[cloud_i + 1] - row0, max_n);            // (a table that disagrees with max_n must not run past the LDS)
    if (n < 1 || row0 < 0 || row0 > total - n) return;                   // the whole workgroup: no barrier is split
    const float *cloud = rows + (size_t)row0 * ld;
    for (int j = tid; j < n; j += 64 * BQR_WAVES) {
        s_cloud[j] = cloud[(size_t)j * ld + 0];
        s_cloud[n + j] = cloud[(size_t)j * ld + 1];
        s_cloud[2 * n + j] = cloud[(size_t)j * ld + 2];
    }
    __syncthreads();
    const int add = global_index ? row0 : 0;
    const int c_begin = blockIdx.x * centres_per_block, c_end = min(c_begin + centres_per_block, s);
    for (int ci = c_begin + wave; ci < c_end; ci += BQR_WAVES) {
        const int cidx = min(max(centres[(size_t)cloud_i * s + ci], 0), n - 1);     // (in range for every checked caller: the clamp is for the rest)
        const float cx = s_cloud[cidx], cy = s_cloud[n + cidx], cz = s_cloud[2 * n + cidx];
        int32_t *dst = out + ((size_t)cloud_i * s + ci) * nsample;
        int filled = 0, first = cidx;                     // wave-uniform
        for (int base = 0; base < n && filled < nsample; base += 64) {
            const int j = base + lane, jc = min(j, n - 1);
            const float dx = cx - s_cloud[jc], dy = cy - s_cloud[n + jc], dz = cz - s_cloud[2 * n + jc];
            const float d = (dx * dx + dy * dy) + dz * dz;
            const bool in = j < n && d <= r2;
            const unsigned long long m = __ballot(in);
            if (m == 0) continue;
            if (filled == 0) first = base + __builtin_ctzll(m);
            const int slot = filled + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (in && slot < nsample) dst[slot] = j + add;
            filled += __popcll(m);
        }
        const int cnt = min(filled, nsample);
        for (int t = cnt + lane; t < nsample; t += 64) dst[t] = first + add;
        if (count && lane == 0) count[(size_t)cloud_i * s + ci] = cnt;
    }
}

}  // namespace ampnet

extern "C" int ampnet_ball_query_ragged_f32(const float *rows, int ld, const int32_t *cloud_off, int n_clouds, int total, int max_n,
                                            const int32_t *centres, int s, float radius, int nsample, int global_index, int32_t *out,
                                            int32_t *count, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_ball_query_ragged_f32";
    AMPNET_REQUIRE(rows && cloud_off && centres && out, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n_clouds <= 65535 && ld >= 3 && s >= 1 && max_n >= 1 && total >= max_n,
                   "%s: bad shape n_clouds=%d (1 .. 65535) ld=%d s=%d max_n=%d total=%d", what, n_clouds, ld, s, max_n, total);
    AMPNET_REQUIRE((long long)n_clouds * s * AMPNET_SA_MAX_NSAMPLE <= 0x7fffffffLL, "%s: n_clouds * s = %lld centres exceed %d", what,
                   (long long)n_clouds * s, 0x7fffffff / AMPNET_SA_MAX_NSAMPLE);
    AMPNET_REQUIRE(nsample >= 1 && nsample <= AMPNET_SA_MAX_NSAMPLE, "%s: nsample=%d must be in [1, %d]", what, nsample, AMPNET_SA_MAX_NSAMPLE);
    AMPNET_REQUIRE(radius >= 0.0f, "%s: radius=%g must be >= 0", what, (double)radius);
    const size_t lds = (size_t)max_n * 3 * sizeof(float);
    AMPNET_REQUIRE(lds <= 144 * 1024, "%s: max_n=%d exceeds %d points per cloud (coordinates must fit LDS)", what, max_n, 144 * 1024 / 12);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ball_query_ragged_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           144 * 1024);
        if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
        attr_set = true;
    }
    const float r2 = radius * radius;
    // the grid of ampnet_ball_query_f32
    int per_block = cdiv(s * n_clouds, 1024);
    if (per_block < 32) per_block = 32;
    if (per_block > s) per_block = s;
    hipLaunchKernelGGL(ball_query_ragged_kernel, dim3(cdiv(s, per_block), n_clouds), dim3(64 * BQR_WAVES), lds, (hipStream_t)stream, rows, ld, cloud_off,
                       total, max_n, centres, s, r2, nsample, per_block, global_index ? 1 : 0, out, count);
    return check_launch("ball_query_ragged_kernel");
}
