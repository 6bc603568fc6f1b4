// ball_query.hip -- radius (ball) grouping of FPS centres (C ABI: ampnet_ball_query_f32; at K radii in one pass: ampnet_ball_query_msg_f32).
//
// BUILD-DEFINED like knn.hip: the reference has no ball query, so the spec is fixed in include/ampnet_hip.h and pinned
// by the build's own CPU restatement (tests/sa_ref.py: ball_query):
//     d(j) = float32 ((dx*dx + dy*dy) + dz*dz), one rounding per operation (compiled with -ffp-contract=off, the distance of knn.hip);
//     j is a member of centre i's ball when d(j) <= r2, r2 = float32 (radius * radius) computed once on the host;
//     out[c][i][0..nsample) = the first nsample members in ascending index order, the rest repeats the first member;
//     count[c][i] = min(members, nsample).
//
// Mapping to CDNA4: the cloud's coordinates sit in LDS as three planes (the plan of knn.hip), one WAVE per centre.  The wave walks
// the candidates in index order, 64 per step: a ballot of the in-radius lanes and the count of set bits below the lane give every
// member its output slot, so the order needs no sort and no atomic.  The walk ends with the step that fills slot nsample - 1.
#include "common.h"

#pragma clang fp contract(off)

namespace ampnet {

constexpr int BQ_WAVES = 16;

__global__ __launch_bounds__(64 * BQ_WAVES) void ball_query_kernel(const float *__restrict__ xyz, int n, int ld, const int32_t *__restrict__ centres,
                                                                  int s, float r2, int nsample, int centres_per_block,
                                                                  int32_t *__restrict__ out, int32_t *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[n], y[n], z[n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cloud_i = blockIdx.y;
    const float *cloud = xyz + (size_t)cloud_i * n * ld;
    for (int j = tid; j < n; j += 64 * BQ_WAVES) {
        s_cloud[j] = cloud[(size_t)j * ld + 0];
        s_cloud[n + j] = cloud[(size_t)j * ld + 1];
        s_cloud[2 * n + j] = cloud[(size_t)j * ld + 2];
    }
    __syncthreads();
    const int c_begin = blockIdx.x * centres_per_block, c_end = min(c_begin + centres_per_block, s);
    for (int ci = c_begin + wave; ci < c_end; ci += BQ_WAVES) {
        const int cidx = centres[(size_t)cloud_i * s + ci];
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
            if (in && slot < nsample) dst[slot] = j;
            filled += __popcll(m);
        }
        const int cnt = min(filled, nsample);
        for (int t = cnt + lane; t < nsample; t += 64) dst[t] = first;
        if (count && lane == 0) count[(size_t)cloud_i * s + ci] = cnt;
    }
}

// K radii around the same centres (ampnet_ball_query_msg_f32): ball_query_kernel's staging, mapping and walk, with the distance of a
// candidate formed once and one ballot / prefix count per scale.  Every filled[k] and first[k] is wave-uniform; K is a template
// parameter so that they stay in registers.  A scale whose list is full takes no further part, and the walk ends with the step after
// which every list is full: per scale the stores are those of ball_query_kernel, in its order.
struct BqMsgArgs {
    float r2[AMPNET_SA_MSG_MAX_SCALES];
    int nsample[AMPNET_SA_MSG_MAX_SCALES];
    int32_t *out[AMPNET_SA_MSG_MAX_SCALES], *count[AMPNET_SA_MSG_MAX_SCALES];
};

template <int K>
__global__ __launch_bounds__(64 * BQ_WAVES) void ball_query_msg_kernel(const float *__restrict__ xyz, int n, int ld, const int32_t *__restrict__ centres,
                                                                      int s, BqMsgArgs a, int centres_per_block)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[n], y[n], z[n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cloud_i = blockIdx.y;
    const float *cloud = xyz + (size_t)cloud_i * n * ld;
    for (int j = tid; j < n; j += 64 * BQ_WAVES) {
        s_cloud[j] = cloud[(size_t)j * ld + 0];
        s_cloud[n + j] = cloud[(size_t)j * ld + 1];
        s_cloud[2 * n + j] = cloud[(size_t)j * ld + 2];
    }
    __syncthreads();
    const int c_begin = blockIdx.x * centres_per_block, c_end = min(c_begin + centres_per_block, s);
    for (int ci = c_begin + wave; ci < c_end; ci += BQ_WAVES) {
        const size_t row = (size_t)cloud_i * s + ci;
        const int cidx = centres[row];
        const float cx = s_cloud[cidx], cy = s_cloud[n + cidx], cz = s_cloud[2 * n + cidx];
        int filled[K], first[K];                          // wave-uniform
#pragma unroll
        for (int k = 0; k < K; ++k) {
            filled[k] = 0;
            first[k] = cidx;
        }
        bool open = true;                                 // some list is not full yet
        for (int base = 0; base < n && open; base += 64) {
            const int j = base + lane, jc = min(j, n - 1);
            const float dx = cx - s_cloud[jc], dy = cy - s_cloud[n + jc], dz = cz - s_cloud[2 * n + jc];
            const float d = (dx * dx + dy * dy) + dz * dz;
            open = false;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (filled[k] >= a.nsample[k]) continue;
                const bool in = j < n && d <= a.r2[k];
                const unsigned long long m = __ballot(in);
                if (m != 0) {
                    if (filled[k] == 0) first[k] = base + __builtin_ctzll(m);
                    const int slot = filled[k] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (in && slot < a.nsample[k]) a.out[k][row * a.nsample[k] + slot] = j;
                    filled[k] += __popcll(m);
                }
                open = open || filled[k] < a.nsample[k];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int nsample = a.nsample[k], cnt = min(filled[k], nsample);
            int32_t *dst = a.out[k] + row * nsample;
            for (int t = cnt + lane; t < nsample; t += 64) dst[t] = first[k];
            if (a.count[k] && lane == 0) a.count[k][row] = cnt;
        }
    }
}

template <int K>
static int ball_query_msg_launch(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const BqMsgArgs &a, size_t lds,
                                 int per_block, hipStream_t st)
{
    int rc = allow_dynamic_lds<ball_query_msg_kernel<K>>(144 * 1024, "ampnet_ball_query_msg_f32");
    if (rc != AMPNET_OK) return rc;
    hipLaunchKernelGGL(ball_query_msg_kernel<K>, dim3(cdiv(s, per_block), n_clouds), dim3(64 * BQ_WAVES), lds, st, xyz, n, ld, centres, s, a,
                       per_block);
    return check_launch("ball_query_msg_kernel");
}

}  // namespace ampnet

extern "C" int ampnet_ball_query_msg_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const float *radii_host,
                                         const int *nsample_host, int K, int32_t *const *out_host, int32_t *const *count_host, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_ball_query_msg_f32";
    AMPNET_REQUIRE(xyz && centres && radii_host && nsample_host && out_host, "%s: null pointer", what);
    AMPNET_REQUIRE(K >= 1 && K <= AMPNET_SA_MSG_MAX_SCALES, "%s: K=%d scales, the kernel is built for 1 .. %d", what, K, AMPNET_SA_MSG_MAX_SCALES);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld >= 3 && s >= 1, "%s: bad shape n_clouds=%d n=%d ld=%d s=%d", what, n_clouds, n, ld, s);
    const size_t lds = (size_t)n * 3 * sizeof(float);
    AMPNET_REQUIRE(lds <= 144 * 1024, "%s: n=%d exceeds %d points per cloud (coordinates must fit LDS)", what, n, 144 * 1024 / 12);
    BqMsgArgs a = {};
    for (int k = 0; k < K; ++k) {
        AMPNET_REQUIRE(out_host[k], "%s: scale %d: null output", what, k);
        AMPNET_REQUIRE(nsample_host[k] >= 1 && nsample_host[k] <= AMPNET_SA_MAX_NSAMPLE, "%s: scale %d: nsample=%d must be in [1, %d]", what, k,
                       nsample_host[k], AMPNET_SA_MAX_NSAMPLE);
        AMPNET_REQUIRE(radii_host[k] >= 0.0f, "%s: scale %d: radius=%g must be >= 0", what, k, (double)radii_host[k]);
        a.r2[k] = radii_host[k] * radii_host[k];
        a.nsample[k] = nsample_host[k];
        a.out[k] = out_host[k];
        a.count[k] = count_host ? count_host[k] : nullptr;
    }
    // the grid of ampnet_ball_query_f32
    int per_block = cdiv(s * n_clouds, 1024);
    if (per_block < 32) per_block = 32;
    if (per_block > s) per_block = s;
    hipStream_t st = (hipStream_t)stream;
    switch (K) {
    case 1: return ball_query_msg_launch<1>(xyz, n_clouds, n, ld, centres, s, a, lds, per_block, st);
    case 2: return ball_query_msg_launch<2>(xyz, n_clouds, n, ld, centres, s, a, lds, per_block, st);
    case 3: return ball_query_msg_launch<3>(xyz, n_clouds, n, ld, centres, s, a, lds, per_block, st);
    default: return ball_query_msg_launch<4>(xyz, n_clouds, n, ld, centres, s, a, lds, per_block, st);
    }
}

extern "C" int ampnet_ball_query_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, float radius, int nsample,
                                     int32_t *out, int32_t *count, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(xyz && centres && out, "ampnet_ball_query_f32: null pointer");
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld >= 3 && s >= 1, "ampnet_ball_query_f32: bad shape n_clouds=%d n=%d ld=%d s=%d", n_clouds, n, ld, s);
    AMPNET_REQUIRE(nsample >= 1 && nsample <= AMPNET_SA_MAX_NSAMPLE, "ampnet_ball_query_f32: nsample=%d must be in [1, %d]", nsample, AMPNET_SA_MAX_NSAMPLE);
    AMPNET_REQUIRE(radius >= 0.0f, "ampnet_ball_query_f32: radius=%g must be >= 0", (double)radius);
    const size_t lds = (size_t)n * 3 * sizeof(float);
    AMPNET_REQUIRE(lds <= 144 * 1024, "ampnet_ball_query_f32: n=%d exceeds %d points per cloud (coordinates must fit LDS)", n, 144 * 1024 / 12);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ball_query_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "ampnet_ball_query_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    const float r2 = radius * radius;
    // the grid of knn.hip: enough workgroups to fill 256 CUs, each amortising its copy of the cloud over >= 32 centres
    int per_block = cdiv(s * n_clouds, 1024);
    if (per_block < 32) per_block = 32;
    if (per_block > s) per_block = s;
    hipLaunchKernelGGL(ball_query_kernel, dim3(cdiv(s, per_block), n_clouds), dim3(64 * BQ_WAVES), lds, (hipStream_t)stream, xyz, n, ld, centres, s,
                       r2, nsample, per_block, out, count);
    return check_launch("ball_query_kernel");
}
