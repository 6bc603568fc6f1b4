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
// With a collective registered (sync_bn.hip: sync_bn_on()) the two launchers take the GLOBAL-batch path, and with them every forward and
// backward that ends in them (feature propagation, set abstraction, the segmentation head; uniform and ragged):
//   forward   fpt_stats_pack_kernel merges the rank's partial rows into ONE row (n, mean, M2)[cout] in the plain finalize's lane and tree
//       order -> all-gather -> fpt_stats_finalize_kernel<true> over the `world` rows in rank order, dividing by the MERGED row count;
//   backward  fpt_bwd_finalize_kernel<true> writes the rank's own dbeta, dgamma, dbias = 0 (the gradient all-reduce adds them up) and the
//       rank's (sum dy, sum dy a)[cout] and row count -> all-reduce -> fpt_bwd_coef_kernel forms the two coefficients from the global sums.
// One exchange per launcher call, whatever the data.  With one rank every exchange is the identity and each value goes through the
// operations of the plain path in their order: the same bits.
#include "bn_train.h"
#include "kernels.h"

namespace ampnet {

// One wave per channel, as fp_bwd_finalize_kernel: lane t merges the partial rows t, t + 64, .. in ascending order, then the 64 lane results
// go through a fixed halving tree (lane t takes lane t + 32, 16, .. 1).  A lane without rows carries n = 0, which fpt_chan passes through.
// The merge of both statistics kernels: channel c of parts [n_parts][3 cout] into the wave's lane 0.
__device__ __forceinline__ void fpt_merge_parts(const float *__restrict__ parts, int n_parts, int cout, int c, int lane, float &n, float &mean,
                                                float &m2)
{
    n = 0.0f, mean = 0.0f, m2 = 0.0f;
    for (int g = lane; g < n_parts; g += 64) {
        const float *row = parts + (size_t)g * 3 * cout;
        fpt_chan(n, mean, m2, row[c], row[cout + c], row[2 * cout + c]);
    }
    for (int off = 32; off; off >>= 1) {
        const float nB = __shfl_down(n, off), meanB = __shfl_down(mean, off), m2B = __shfl_down(m2, off);
        if (nB > 0.0f) fpt_chan(n, mean, m2, nB, meanB, m2B);
    }
}

// GLOBAL: parts are the ranks' gathered rows (fpt_stats_pack_kernel) in rank order and the row count is the MERGED one -- the ranks of a
// ragged batch hold different numbers of rows, so no rank's own M is it; M is not read.
template <bool GLOBAL>
__global__ __launch_bounds__(256) void fpt_stats_finalize_kernel(FptStats q, const float *__restrict__ parts, int n_parts, float M,
                                                                float *__restrict__ fold)
{
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= q.cout) return;                      // (the whole wave)
    float n, mean, m2;
    fpt_merge_parts(parts, n_parts, q.cout, c, lane, n, mean, m2);
    if (lane) return;
    if (GLOBAL) M = n;
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

// The global-batch forward's first launch: the rank's partial rows merged into ONE row loc [3 cout] = (n, mean, M2), in exactly the lane and
// tree order of fpt_stats_finalize_kernel.
__global__ __launch_bounds__(256) void fpt_stats_pack_kernel(int cout, const float *__restrict__ parts, int n_parts, float *__restrict__ loc)
{
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= cout) return;                        // (the whole wave)
    float n, mean, m2;
    fpt_merge_parts(parts, n_parts, cout, c, lane, n, mean, m2);
    if (lane) return;
    loc[c] = n;
    loc[cout + c] = mean;
    loc[2 * cout + c] = m2;
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
// GLOBAL: dbeta, dgamma and dbias stay the RANK's sums; instead of the coefficients the kernel writes comm [2 cout + 1] = the rank's sum dy,
// sum dy a and row count M for the all-reduce (coef is not touched: fpt_bwd_coef_kernel writes it from the global sums).
template <bool GLOBAL>
__global__ __launch_bounds__(256) void fpt_bwd_finalize_kernel(int cout, const float *__restrict__ parts, int n_parts, float M,
                                                              const float *__restrict__ mean, const float *__restrict__ invstd,
                                                              float *__restrict__ dbias, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                              float *__restrict__ coef, float *__restrict__ comm)
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
    if (GLOBAL) {
        comm[c] = sb;
        comm[cout + c] = G;
        if (c == 0) comm[2 * cout] = M;
        return;
    }
    coef[c] = sb / M;
    coef[cout + c] = dg * invstd[c] / M;
}

// The global-batch backward's last launch: comm [2 cout + 1] holds the all-reduced sum dy, sum dy a and row count n ->
// coef = {sum dy / n, dgamma_global invstd / n}, dgamma_global = invstd (G - mean sum dy): fpt_bwd_finalize_kernel's operations on the global sums.
__global__ void fpt_bwd_coef_kernel(int cout, const float *__restrict__ comm, const float *__restrict__ mean, const float *__restrict__ invstd,
                                    float *__restrict__ coef)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cout) return;
    const float sb = comm[c], G = comm[cout + c], n = comm[2 * cout];
    const float dg = invstd[c] * fmaf(-mean[c], sb, G);
    coef[c] = sb / n;
    coef[cout + c] = dg * invstd[c] / n;
}

int fpt_stats_finalize_launch(const FptStats &q, const float *parts, int n_parts, long long M, float *fold, hipStream_t st)
{
    if (sync_bn_on()) {
        // global batch: the rank's one row -> all-gather -> finalize over the ranks' rows.  ONE exchange per call on every rank.
        const size_t seg = (size_t)3 * q.cout;
        float *loc = nullptr, *all = nullptr;
        AMPNET_TRY(sync_bn_gather(seg, &loc, &all));
        hipLaunchKernelGGL(fpt_stats_pack_kernel, dim3(cdiv(q.cout, 4)), dim3(256), 0, st, q.cout, parts, n_parts, loc);
        AMPNET_TRY(check_launch("fpt_stats_pack_kernel"));
        AMPNET_TRY(sync_bn_exchange(AMPNET_COLLECTIVE_ALLGATHER, loc, all, seg, st));
        hipLaunchKernelGGL(fpt_stats_finalize_kernel<true>, dim3(cdiv(q.cout, 4)), dim3(256), 0, st, q, all, sync_bn_world(), 0.0f, fold);
        return check_launch("fpt_stats_finalize_kernel (global batch)");
    }
    hipLaunchKernelGGL(fpt_stats_finalize_kernel<false>, dim3(cdiv(q.cout, 4)), dim3(256), 0, st, q, parts, n_parts, (float)M, fold);
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
    if (sync_bn_on()) {
        // global batch: the rank's gradients and its sums -> all-reduce -> the coefficients.  ONE exchange per call on every rank.
        const size_t seg = (size_t)2 * cout + 1;
        float *comm = nullptr, *unused = nullptr;
        AMPNET_TRY(sync_bn_gather(seg, &comm, &unused));
        hipLaunchKernelGGL(fpt_bwd_finalize_kernel<true>, dim3(cdiv(cout, 4)), dim3(256), 0, st, cout, parts, n_parts, (float)M, mean, invstd,
                           dbias, dgamma, dbeta, coef, comm);
        AMPNET_TRY(check_launch("fpt_bwd_finalize_kernel (global batch)"));
        AMPNET_TRY(sync_bn_exchange(AMPNET_COLLECTIVE_ALLREDUCE_SUM, comm, comm, seg, st));
        hipLaunchKernelGGL(fpt_bwd_coef_kernel, dim3(cdiv(cout, 256)), dim3(256), 0, st, cout, comm, mean, invstd, coef);
        return check_launch("fpt_bwd_coef_kernel");
    }
    hipLaunchKernelGGL(fpt_bwd_finalize_kernel<false>, dim3(cdiv(cout, 4)), dim3(256), 0, st, cout, parts, n_parts, (float)M, mean, invstd, dbias,
                       dgamma, dbeta, coef, (float *)nullptr);
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
    if (sync_bn_on()) {
        // the merged row count of the global batch must be an exact float too.  The ranks' rows differ and no rank knows the others' here, so
        // the rule is this rank's M times the world size: conservative, decided on the host, the same on every call.
        const long long world = sync_bn_world();
        AMPNET_REQUIRE(M <= max_rows / world, "%s: M = %s = %lld rows x %lld ranks exceed %lld: with a registered collective the statistics are "
                       "the global batch's, and the rule is the conservative M * world_size (the ranks' row counts differ)", what, rows_text, M,
                       world, max_rows);
    }
    return AMPNET_OK;
}

}  // namespace ampnet
