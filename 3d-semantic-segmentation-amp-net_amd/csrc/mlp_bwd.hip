// mlp_bwd.hip -- the kernels both fused backwards share (mlp_bwd.h) and their launchers.
//
//   fp_wgrad_kernel, fp_wgrad_reduce_kernel   dW_l = dz_l^T x_l as a split-K MFMA GEMM over the rows: a wave takes a 32 x 128 block of dW and
//       one chunk of rows (ascending, k-step i of half h takes row k0 + 2 i + h), the chunks' partials are added in ascending chunk order.
//       The project's pw_wgrad / sgemm_wgrad_bias are built around windows and slots of the AMP-Net encoder (per-slot partials, BatchNorm
//       constants folded in); these layers have neither, so they get a kernel of their own.
//   fp_bwd_finalize_kernel  adds the workgroups' partials in a fixed order (a wave per channel) and derives dbeta, dgamma and dbias.
#include "mlp_bwd.h"

namespace ampnet {

// dW partial of one chunk of rows: block (c0 / 128, o0 / 32, chunk), one wave; part [chunks][cout][ldxs]
__global__ __launch_bounds__(64) void fp_wgrad_kernel(const float *__restrict__ dz, int cout, const float *__restrict__ xs, int ldxs, long long M,
                                                     int chunk_rows, float *__restrict__ part)
{
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.x * 128, o0 = blockIdx.y * 32;
    const long long k_begin = (long long)blockIdx.z * chunk_rows, k_end = min(M, k_begin + chunk_rows);
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    for (long long k0 = k_begin; k0 < k_end; k0 += 8) {
        float av[4], bv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long row = k0 + 2 * i + h;
            av[i] = row < k_end ? dz[(size_t)row * cout + o0 + r] : 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) bv[t][i] = row < k_end && c0 + 32 * t < ldxs ? xs[(size_t)row * ldxs + c0 + 32 * t + r] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
    float *dst = part + (size_t)blockIdx.z * cout * ldxs;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c0 + 32 * t < ldxs)
#pragma unroll
            for (int i = 0; i < 16; ++i) dst[(size_t)(o0 + mlp_acc_row(i, h)) * ldxs + c0 + 32 * t + r] = acc[t][i];
}

__global__ void fp_wgrad_reduce_kernel(const float *__restrict__ part, int chunks, int cout, int cin, int ldxs, float *__restrict__ dW)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cout * cin) return;
    const int o = e / cin, c = e - o * cin;
    float v = 0.0f;
    for (int q = 0; q < chunks; ++q) v += part[((size_t)q * cout + o) * ldxs + c];
    dW[e] = v;
}

// next to sa_fold_kernel: the same parameters, the other direction.  One wave per channel: lane t adds the partials of workgroups t, t + 64, ..
// in ascending order, the 64 lane sums go through a fixed halving tree (32, 16, .. 1).
__global__ __launch_bounds__(256) void fp_bwd_finalize_kernel(MlpPlan p, MlpFold f, FpBwdFin g, const float *__restrict__ fold,
                                                             const float *__restrict__ parts, int n_parts, int sum_c)
{
    const int lane = threadIdx.x & 63, ch = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= sum_c) return;                      // (the whole wave)
    int l = 0;
    while (l + 1 < p.L && ch >= p.fold_off[l + 1] / 2) ++l;
    const int c = ch - p.fold_off[l] / 2;
    float dbeta = 0.0f, G = 0.0f;
    for (int q = lane; q < n_parts; q += 64) {
        dbeta += parts[(size_t)q * 2 * sum_c + ch];
        G += parts[(size_t)q * 2 * sum_c + sum_c + ch];
    }
    for (int off = 32; off; off >>= 1) {
        dbeta += __shfl_down(dbeta, off);
        G += __shfl_down(G, off);
    }
    if (lane) return;
    g.dbeta[l][c] = dbeta;
    g.dgamma[l][c] = fmaf(f.bias[l][c] - f.mean[l][c], dbeta, G) / sqrtf(f.var[l][c] + f.eps[l]);
    g.dbias[l][c] = fold[p.fold_off[l] + c] * dbeta;
}

int mlp_bwd_layout(const char *what, size_t off, int cin0, int dx0_cols, long long M, int grid, int chunks, const int *cout_host, int L,
                   MlpBwdLayout &lay)
{
    lay = {};
    size_t wmax = 0;
    for (int l = 0; l < L; ++l) {
        const int cout = cout_host[l];
        AMPNET_REQUIRE(cout >= 32 && cout <= MLP_MAX_COUT && cout % 32 == 0, "%s: layer %d has cout=%d, must be a multiple of 32 in [32, %d]", what,
                       l, cout, MLP_MAX_COUT);
        lay.cin[l] = l ? cout_host[l - 1] : cin0;
        lay.ldxs[l] = (lay.cin[l] + 31) / 32 * 32;
        lay.sum_c += cout;
        if ((size_t)cout * lay.ldxs[l] > wmax) wmax = (size_t)cout * lay.ldxs[l];
    }
    lay.off_parts = off;
    off += align_up((size_t)grid * 2 * lay.sum_c, 64);
    for (int l = 0; l < L; ++l) {
        lay.off_xs[l] = off;
        off += align_up((size_t)M * lay.ldxs[l], 64);
        lay.off_dz[l] = off;
        off += align_up((size_t)M * cout_host[l], 64);
    }
    lay.off_dx0 = off;
    off += align_up((size_t)M * dx0_cols, 64);
    lay.off_wpart = off;
    off += align_up((size_t)chunks * wmax, 64);
    lay.floats = off;
    return AMPNET_OK;
}

int fpb_wgrad_launch(const float *dz, int cout, const float *xs, int cin, int ldxs, long long M, int chunk_rows, int chunks, float *wpart,
                     float *dW, hipStream_t st)
{
    hipLaunchKernelGGL(fp_wgrad_kernel, dim3(cdiv(ldxs, 128), cout / 32, chunks), dim3(64), 0, st, dz, cout, xs, ldxs, M, chunk_rows, wpart);
    int rc = check_launch("fp_wgrad_kernel");
    if (rc != AMPNET_OK) return rc;
    hipLaunchKernelGGL(fp_wgrad_reduce_kernel, dim3(cdiv(cout * cin, 256)), dim3(256), 0, st, wpart, chunks, cout, cin, ldxs, dW);
    return check_launch("fp_wgrad_reduce_kernel");
}

int fpb_finalize_launch(const MlpPlan &p, const MlpFold &f, const FpBwdFin &g, const float *fold, const float *parts, int n_parts, int sum_c,
                        hipStream_t st)
{
    hipLaunchKernelGGL(fp_bwd_finalize_kernel, dim3(cdiv(sum_c, 4)), dim3(256), 0, st, p, f, g, fold, parts, n_parts, sum_c);
    return check_launch("fp_bwd_finalize_kernel");
}

int bwd_clouds_ragged(const char *what, const int32_t *cloud_off, int n_clouds, int total, int s, BwdClouds &c)
{
    AMPNET_REQUIRE(cloud_off, "%s: null cloud_off", what);
    AMPNET_REQUIRE(n_clouds >= 1 && total >= 1 && s >= 1, "%s: bad shape n_clouds=%d total=%d s=%d", what, n_clouds, total, s);
    AMPNET_REQUIRE((long long)n_clouds * s <= 0x7fffffffLL, "%s: n_clouds * s = %lld exceed 2^31 - 1", what, (long long)n_clouds * s);
    c = {1, total, n_clouds * s, cloud_off, n_clouds, s};
    return AMPNET_OK;
}

}  // namespace ampnet
