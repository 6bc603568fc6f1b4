// cloud_search.h -- what the searches over one cloud in LDS share (knn.hip, ball_query.hip, three_nn.hip): the staging of the cloud, the
// distance, the grid rule and the host checks of a dense cloud.  Included by -ffp-contract=off sources only; the pragma below keeps the
// distance at one rounding per operation whichever way the header is reached.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace ampnet {

constexpr size_t CLOUD_LDS_MAX = 144 * 1024;             // dynamic LDS of a search: 12288 points of 12 bytes, of the CU's 160 KB

// Rows 0 .. n of `rows` (leading dimension ld, columns 0 .. 2) -> the planes x[n], y[n], z[n] of s_cloud, by a workgroup of THREADS
// threads, ALL of which call this: it ends with the barrier.
template <int THREADS>
__device__ __forceinline__ void stage_cloud(float *s_cloud, const float *__restrict__ rows, int n, int ld)
{
    for (int j = threadIdx.x; j < n; j += THREADS) {
        s_cloud[j] = rows[(size_t)j * ld + 0];
        s_cloud[n + j] = rows[(size_t)j * ld + 1];
        s_cloud[2 * n + j] = rows[(size_t)j * ld + 2];
    }
    __syncthreads();
}

// float32 ((dx*dx + dy*dy) + dz*dz) from (px, py, pz) to candidate j of the staged planes: THE distance of the build-defined searches
__device__ __forceinline__ float staged_dist2(const float *s_cloud, int n, int j, float px, float py, float pz)
{
    const float dx = px - s_cloud[j], dy = py - s_cloud[n + j], dz = pz - s_cloud[2 * n + j];
    return (dx * dx + dy * dy) + dz * dz;
}

// The grid of the one-wave-per-centre searches: enough workgroups to fill 256 CUs, each amortising its copy of the cloud over >= 32 centres
inline int centres_per_block(int s, int n_clouds)
{
    int per_block = cdiv(s * n_clouds, 1024);
    if (per_block < 32) per_block = 32;
    return per_block > s ? s : per_block;
}

// n points (`name`: what the caller calls n) must fit the LDS
inline int check_cloud_lds(const char *who, const char *name, int n)
{
    AMPNET_REQUIRE((size_t)n * 12 <= CLOUD_LDS_MAX, "%s: %s=%d exceeds %d points per cloud (coordinates must fit LDS)", who, name, n,
                   (int)(CLOUD_LDS_MAX / 12));
    return AMPNET_OK;
}

// The shape rules of an entry point over [n_clouds, n, ld] clouds with s centres each
inline int check_dense_clouds(const char *who, int n_clouds, int n, int ld, int s)
{
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld >= 3 && s >= 1, "%s: bad shape n_clouds=%d n=%d ld=%d s=%d", who, n_clouds, n, ld, s);
    return check_cloud_lds(who, "n", n);
}

}  // namespace ampnet
