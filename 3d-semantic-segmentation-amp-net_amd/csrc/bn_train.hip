// bn_train.hip -- the kernels both train-mode BatchNorm paths launch (feature_propagation_train.hip, set_abstraction_train.hip), their
// launchers and the host code of bn_train.h.  None of them depends on how the rows are built.
//
//   fpt_stats_finalize_kernel   a wave per channel merges the partial rows of a statistics pass with Chan's formula (lane t the rows t,
//       t + 64, .. ascending, then a halving tree over the lanes: 16 + 6 dependent merges instead of 1024) and writes scale_l, shift_l into
//       the fold, save_mean, save_invstd, and the running-statistics update.
//   fpt_fold_kernel             the backward's fold: scale and shift of every layer from the saved statistics.
//   fpt_bwd_finalize_kernel     a wave per channel adds the partial rows of a backward phase (lane t rows t, t + 64, .. ascending, then a
//       halving tree), writes dbeta, dgamma = invstd (G - mu dbeta), dbias = 0 and the two coefficients dbeta / M and dgamma invstd / M of
//       the next phase.
#include "bn_train.h"

namespace ampnet {

// One wave per channel, as fp_bwd_finalize_kernel: lane t merges the partial rows t, t + 64, .. in ascending order, then the 64 lane results
// go through a fixed halving tree (lane t takes lane t + 32, 16, .. 1).  A lane without rows carries n = 0, which fpt_chan passes through.
__global__ __launch_bounds__(256) void fpt_stats_finalize_kernel(FptStats q, const float *__restrict__ parts, int n_parts, float M,
                                                                float *__restrict__ fold)
{
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= q.cout) return;                      // (the whole wave)
    float n = 0.0f, mean = 0.0f, m2 = 0.0f;
    for (int g = lane; g < n_parts; g += 64) {
        const float *row = parts + (size_t)g * 3 * q.cout;
        fpt_chan(n, mean, m2, row[c], row[q.cout + c], row[2 * q.cout + c]);
    }
    for (int off = 32; off; off >>= 1) {
        const float nB = __shfl_down(n, off), meanB = __shfl_down(mean, off), m2B = __shfl_down(m2, off);
        if (nB > 0.0f) fpt_chan(n, mean, m2, nB, meanB, m2B);
    }
    if (lane) return;
    const float var = m2 / M, invstd = 1.0f / sqrtf(var + q.eps);
    const float scale = q.gamma[c] * invstd;
    fold[q.fold_off + c] = scale;
    fold[q.fold_off + q.cout + c] = fmaf(-mean, scale, q.beta[c]);
    q.save_mean[c] = mean;
    q.save_invstd[c] = invstd;
    const float keep = 1.0f - q.momentum;
    q.running_mean[c] = fmaf(q.momentum, mean + q.bias[c], keep * q.running_mean[c]);
    q.running_var[c] = fmaf(q.momentum, m2 / (M - 1.0f), keep * q.running_var[c]);
}

// scale and shift of every layer from the saved statistics, as the forward's finalize formed them (the same two operations: the same bits)
__global__ void fpt_fold_kernel(MlpPlan p, MlpFold f, float *__restrict__ fold)
{
    for (int l = 0; l < p.L; ++l)
        for (int c = threadIdx.x; c < p.cout[l]; c += blockDim.x) {
            const float scale = f.gamma[l][c] * f.var[l][c];                      // (slot 5 of a layer holds save_invstd, slot 4 save_mean)
            fold[p.fold_off[l] + c] = scale;
            fold[p.fold_off[l] + p.cout[l] + c] = fmaf(-f.mean[l][c], scale, f.beta[l][c]);
        }
}

// parts [n_parts][2 cout]: a row per workgroup, sum dy then sum dy a.  One wave per channel, as fp_bwd_finalize_kernel.
__global__ __launch_bounds__(256) void fpt_bwd_finalize_kernel(int cout, const float *__restrict__ parts, int n_parts, float M,
                                                              const float *__restrict__ mean, const float *__restrict__ invstd,
                                                              float *__restrict__ dbias, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                              float *__restrict__ coef)
{
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= cout) return;                        // (the whole wave)
    float sb = 0.0f, G = 0.0f;
    for (int q = lane; q < n_parts; q += 64) {
        sb += parts[(size_t)q * 2 * cout + c];
        G += parts[(size_t)q * 2 * cout + cout + c];
    }
    for (int off = 32; off; off >>= 1) {
        sb += __shfl_down(sb, off);
        G += __shfl_down(G, off);
    }
    if (lane) return;
    const float dg = invstd[c] * fmaf(-mean[c], sb, G);
    dbeta[c] = sb;
    dgamma[c] = dg;
    dbias[c] = 0.0f;
    coef[c] = sb / M;
    coef[cout + c] = dg * invstd[c] / M;
}

int fpt_stats_finalize_launch(const FptStats &q, const float *parts, int n_parts, long long M, float *fold, hipStream_t st)
{
    hipLaunchKernelGGL(fpt_stats_finalize_kernel, dim3(cdiv(q.cout, 4)), dim3(256), 0, st, q, parts, n_parts, (float)M, fold);
    return check_launch("fpt_stats_finalize_kernel");
}

int fpt_fold_launch(const MlpPlan &p, const MlpFold &f, float *fold, hipStream_t st)
{
    hipLaunchKernelGGL(fpt_fold_kernel, dim3(1), dim3(256), 0, st, p, f, fold);
    return check_launch("fpt_fold_kernel");
}

int fpt_bwd_finalize_launch(int cout, const float *parts, int n_parts, long long M, const float *mean, const float *invstd, float *dbias,
                            float *dgamma, float *dbeta, float *coef, hipStream_t st)
{
    hipLaunchKernelGGL(fpt_bwd_finalize_kernel, dim3(cdiv(cout, 4)), dim3(256), 0, st, cout, parts, n_parts, (float)M, mean, invstd, dbias, dgamma,
                       dbeta, coef);
    return check_launch("fpt_bwd_finalize_kernel");
}

size_t bnt_bwd_plan(const MlpPlan &p, const MlpFold &f, const MlpBwdLayout &lay, float *ws, size_t off_coef, BntBwd &b)
{
    b = {};
    int widest = p.kp[0];
    for (int l = 0; l < p.L; ++l) widest = p.cout[l] > widest ? p.cout[l] : widest;
    b.ld = widest + 1;
    b.parts = ws + lay.off_parts;
    b.dx0 = ws + lay.off_dx0;
    b.coef = ws + off_coef;
    for (int l = 0; l < p.L; ++l) {
        b.ldxs[l] = lay.ldxs[l];
        b.xs[l] = ws + lay.off_xs[l];
        b.dz[l] = ws + lay.off_dz[l];
        b.mean[l] = f.mean[l];
    }
    return (size_t)2 * 32 * b.ld * sizeof(float);
}

int bnt_rows_ok(const char *what, long long M, long long max_rows, const char *rows_text)
{
    AMPNET_REQUIRE(M >= 2, "%s: batch statistics need M = %s >= 2 rows, got %lld", what, rows_text, M);
    AMPNET_REQUIRE(M <= max_rows, "%s: M = %s = %lld rows exceed %lld (the row counts of the statistics are exact floats)", what, rows_text, M,
                   max_rows);
    return AMPNET_OK;
}

}  // namespace ampnet
