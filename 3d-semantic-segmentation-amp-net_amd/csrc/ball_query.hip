// ball_query.hip -- radius (ball) grouping of FPS centres (C ABI: ampnet_ball_query_f32; at K radii in one pass: ampnet_ball_query_msg_f32;
// for clouds of UNEQUAL size in one launch: ampnet_ball_query_ragged_f32).
//
// BUILD-DEFINED like knn.hip: the reference has no ball query, so the spec is fixed in include/ampnet_hip.h and pinned
// by the build's own CPU restatement (tests/sa_ref.py: ball_query):
//     d(j) = float32 ((dx*dx + dy*dy) + dz*dz), one rounding per operation (cloud_search.h: staged_dist2, the distance of knn.hip);
//     j is a member of centre i's ball when d(j) <= r2, r2 = float32 (radius * radius) computed once on the host;
//     out[c][i][0..nsample) = the first nsample members in ascending index order, the rest repeats the first member;
//     count[c][i] = min(members, nsample).
//
// Mapping to CDNA4: the cloud's coordinates sit in LDS as three planes (the plan of knn.hip), one WAVE per centre.  The wave walks
// the candidates in index order, 64 per step: a ballot of the in-radius lanes and the count of set bits below the lane give every
// member its output slot, so the order needs no sort and no atomic.  ONE walk (ball_walk) serves the three entry points; the two kernels
// differ in where a cloud's rows and length come from.
//
// Ragged: the clouds lie back to back in one [total, ld] array; cloud b is the rows cloud_off[b] .. cloud_off[b + 1] (a device table, the
// layout of ampnet_fps_ragged_f32) and has the same s centres as every other cloud, given relative to its own first row.  With
// global_index = 1 every stored index has cloud_off[b] added, so the lists address the packed array as ONE cloud (what
// ampnet_sa_forward_f32 takes with n_clouds = 1).  The dynamic LDS of the launch is sized by the LARGEST cloud (max_n * 12 bytes), so the
// workgroups per CU -- the occupancy -- are those of the largest cloud for every cloud of the call; a cloud stages and walks only its own
// n points.  (1100 .. 4000 points, the clusters of a file: 13 .. 47 KB of the CU's 160 KB, and the 16 waves of a workgroup bound the
// residency before LDS does.  Callers whose sizes differ by an order of magnitude can bucket them as fps_indices_ragged does;
// tools/prof_pn2_ragged.py measures the unbucketed call.)
#include "cloud_search.h"

namespace ampnet {

constexpr int BQ_WAVES = 16;

template <int K>
struct BqArgs {                                          // a kernel argument: K scales take K scales' bytes
    float r2[K];
    int nsample[K];
    int32_t *out[K], *count[K];
};

// The walk of this workgroup's centres of cloud `cloud_i` (n points, staged) at K radii: the distance of a candidate is formed once, with
// one ballot / prefix count per scale.  Every filled[k] and first[k] is wave-uniform; K is a template parameter so that they stay in
// registers.  A scale whose list is full takes no further part, and the walk ends with the step after which every list is full.  Stored
// indices are relative to the cloud, plus `add`; `clamp` brings a centre outside the cloud into it (the ragged entry point, whose centres
// the host cannot see).
template <int K>
__device__ __forceinline__ void ball_walk(const float *s_cloud, int cloud_i, int n, int add, bool clamp, const int32_t *__restrict__ centres, int s,
                                          const BqArgs<K> &a, int centres_per_block)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c_begin = blockIdx.x * centres_per_block, c_end = min(c_begin + centres_per_block, s);
    for (int ci = c_begin + wave; ci < c_end; ci += BQ_WAVES) {
        const size_t row = (size_t)cloud_i * s + ci;
        int cidx = centres[row];
        if (clamp) cidx = min(max(cidx, 0), n - 1);
        const float cx = s_cloud[cidx], cy = s_cloud[n + cidx], cz = s_cloud[2 * n + cidx];
        int filled[K], first[K];                          // wave-uniform
#pragma unroll
        for (int k = 0; k < K; ++k) {
            filled[k] = 0;
            first[k] = cidx;
        }
        bool open = true;                                 // some list is not full yet
        for (int base = 0; base < n && open; base += 64) {
            const int j = base + lane;
            const float d = staged_dist2(s_cloud, n, min(j, n - 1), cx, cy, cz);
            open = false;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (K > 1 && filled[k] >= a.nsample[k]) continue;      // (K = 1: `open` has said so)
                const bool in = j < n && d <= a.r2[k];
                const unsigned long long m = __ballot(in);
                if (m != 0) {
                    if (filled[k] == 0) first[k] = base + __builtin_ctzll(m);
                    const int slot = filled[k] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (in && slot < a.nsample[k]) a.out[k][row * a.nsample[k] + slot] = j + add;
                    filled[k] += __popcll(m);
                }
                open = open || filled[k] < a.nsample[k];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int nsample = a.nsample[k], cnt = min(filled[k], nsample);
            int32_t *dst = a.out[k] + row * nsample;
            for (int t = cnt + lane; t < nsample; t += 64) dst[t] = first[k] + add;
            if (a.count[k] && lane == 0) a.count[k][row] = cnt;
        }
    }
}

template <int K>
__global__ __launch_bounds__(64 * BQ_WAVES) void ball_query_kernel(const float *__restrict__ xyz, int n, int ld, const int32_t *__restrict__ centres,
                                                                  int s, BqArgs<K> a, int centres_per_block)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[n], y[n], z[n]
    const int cloud_i = blockIdx.y;
    stage_cloud<64 * BQ_WAVES>(s_cloud, xyz + (size_t)cloud_i * n * ld, n, ld);
    ball_walk<K>(s_cloud, cloud_i, n, 0, false, centres, s, a, centres_per_block);
}

__global__ __launch_bounds__(64 * BQ_WAVES) void ball_query_ragged_kernel(const float *__restrict__ rows, int ld, const int32_t *__restrict__ cloud_off,
                                                                          int total, int max_n, const int32_t *__restrict__ centres, int s, BqArgs<1> a,
                                                                          int centres_per_block, int global_index)
{
    extern __shared__ __attribute__((aligned(16))) float s_cloud[];      // x[n], y[n], z[n]
    const int cloud_i = blockIdx.y;
    const int row0 = cloud_off[cloud_i];
    const int n = min(cloud_off[cloud_i + 1] - row0, max_n);            // (a table that disagrees with max_n must not run past the LDS)
    if (n < 1 || row0 < 0 || row0 > total - n) return;                   // the whole workgroup: no barrier is split
    stage_cloud<64 * BQ_WAVES>(s_cloud, rows + (size_t)row0 * ld, n, ld);
    ball_walk<1>(s_cloud, cloud_i, n, global_index ? row0 : 0, true, centres, s, a, centres_per_block);
}

// The rules of every scale of entry point `who` -> the kernels' argument block.  `named`: the entry point takes several scales and its
// messages say which.
template <int K>
static int bq_scales(const char *who, bool named, const float *radii, const int *nsamples, int32_t *const *outs, int32_t *const *counts,
                     BqArgs<K> &a)
{
    for (int k = 0; k < K; ++k) {
        char tag[24] = "";
        if (named) snprintf(tag, sizeof tag, "scale %d: ", k);
        AMPNET_REQUIRE(outs[k], "%s: %snull output", who, tag);
        AMPNET_REQUIRE(nsamples[k] >= 1 && nsamples[k] <= AMPNET_SA_MAX_NSAMPLE, "%s: %snsample=%d must be in [1, %d]", who, tag, nsamples[k],
                       AMPNET_SA_MAX_NSAMPLE);
        AMPNET_REQUIRE(radii[k] >= 0.0f, "%s: %sradius=%g must be >= 0", who, tag, (double)radii[k]);
        a.r2[k] = radii[k] * radii[k];
        a.nsample[k] = nsamples[k];
        a.out[k] = outs[k];
        a.count[k] = counts ? counts[k] : nullptr;
    }
    return AMPNET_OK;
}

// The dense entry points behind their null-pointer check: shape, scales, launch
template <int K>
static int ball_query_dense(const char *who, bool named, const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                            const float *radii, const int *nsamples, int32_t *const *outs, int32_t *const *counts, void *stream)
{
    AMPNET_TRY(check_dense_clouds(who, n_clouds, n, ld, s));
    BqArgs<K> a;
    AMPNET_TRY(bq_scales<K>(who, named, radii, nsamples, outs, counts, a));
    AMPNET_TRY(allow_dynamic_lds<ball_query_kernel<K>>(CLOUD_LDS_MAX, who));
    const int per_block = centres_per_block(s, n_clouds);
    hipLaunchKernelGGL(ball_query_kernel<K>, dim3(cdiv(s, per_block), n_clouds), dim3(64 * BQ_WAVES), (size_t)n * 12, (hipStream_t)stream, xyz, n, ld,
                       centres, s, a, per_block);
    return check_launch("ball_query_kernel");
}

}  // namespace ampnet

extern "C" int ampnet_ball_query_msg_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const float *radii_host,
                                         const int *nsample_host, int K, int32_t *const *out_host, int32_t *const *count_host, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_ball_query_msg_f32";
    AMPNET_REQUIRE(xyz && centres && radii_host && nsample_host && out_host, "%s: null pointer", what);
    AMPNET_REQUIRE(K >= 1 && K <= AMPNET_SA_MSG_MAX_SCALES, "%s: K=%d scales, the kernel is built for 1 .. %d", what, K, AMPNET_SA_MSG_MAX_SCALES);
    switch (K) {
    case 1: return ball_query_dense<1>(what, true, xyz, n_clouds, n, ld, centres, s, radii_host, nsample_host, out_host, count_host, stream);
    case 2: return ball_query_dense<2>(what, true, xyz, n_clouds, n, ld, centres, s, radii_host, nsample_host, out_host, count_host, stream);
    case 3: return ball_query_dense<3>(what, true, xyz, n_clouds, n, ld, centres, s, radii_host, nsample_host, out_host, count_host, stream);
    default: return ball_query_dense<4>(what, true, xyz, n_clouds, n, ld, centres, s, radii_host, nsample_host, out_host, count_host, stream);
    }
}

extern "C" int ampnet_ball_query_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, float radius, int nsample,
                                     int32_t *out, int32_t *count, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_ball_query_f32";
    AMPNET_REQUIRE(xyz && centres && out, "%s: null pointer", what);
    return ball_query_dense<1>(what, false, xyz, n_clouds, n, ld, centres, s, &radius, &nsample, &out, &count, stream);
}

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
    AMPNET_TRY(check_cloud_lds(what, "max_n", max_n));
    BqArgs<1> a;
    AMPNET_TRY(bq_scales<1>(what, false, &radius, &nsample, &out, &count, a));
    AMPNET_TRY(allow_dynamic_lds<ball_query_ragged_kernel>(CLOUD_LDS_MAX, what));
    const int per_block = centres_per_block(s, n_clouds);
    hipLaunchKernelGGL(ball_query_ragged_kernel, dim3(cdiv(s, per_block), n_clouds), dim3(64 * BQ_WAVES), (size_t)max_n * 12, (hipStream_t)stream, rows,
                       ld, cloud_off, total, max_n, centres, s, a, per_block, global_index ? 1 : 0);
    return check_launch("ball_query_ragged_kernel");
}
