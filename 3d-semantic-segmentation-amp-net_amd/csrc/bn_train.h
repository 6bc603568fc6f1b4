// bn_train.h -- what the two train-mode BatchNorm paths share (feature_propagation_train.hip, set_abstraction_train.hip): Chan's merge of
// the centred statistics, what a statistics finalize reads and writes, and the launchers of the kernels that do not depend on how the rows
// are built (they live in feature_propagation_train.hip): the statistics finalize, the fold from the saved statistics, the backward's
// finalize.
#pragma once
#include "fused_mlp.h"

namespace ampnet {

// Chan's merge of (nA, meanA, M2A) and (nB, meanB, M2B) into A; nA = 0 takes B as it is
__device__ __forceinline__ void fpt_chan(float &nA, float &meanA, float &m2A, float nB, float meanB, float m2B)
{
    if (nA == 0.0f) {
        nA = nB;
        meanA = meanB;
        m2A = m2B;
        return;
    }
    const float n = nA + nB, delta = meanB - meanA;
    meanA = fmaf(delta, nB / n, meanA);
    m2A = fmaf(delta * delta, nA * nB / n, m2A + m2B);
    nA = n;
}

struct FptStats {                         // what the finalize of pass l reads and writes
    const float *bias, *gamma, *beta;
    float *running_mean, *running_var, *save_mean, *save_invstd;
    float eps, momentum;
    int cout, fold_off;
};

// fpt_stats_finalize_kernel on `st`: parts [n_parts][3 q.cout] (count, mean, sum of squared deviations per partial row) -> scale and shift of
// the layer in `fold`, save_mean, save_invstd and the running-statistics update over M rows
int fpt_stats_finalize_launch(const FptStats &q, const float *parts, int n_parts, long long M, float *fold, hipStream_t st);
// fpt_fold_kernel on `st`: scale and shift of every layer from save_mean (f.mean) and save_invstd (f.var), by the forward's two operations
int fpt_fold_launch(const MlpPlan &p, const MlpFold &f, float *fold, hipStream_t st);
// fpt_bwd_finalize_kernel on `st`: parts [n_parts][2 cout] (a row per workgroup: sum dy, then sum dy a) -> dbeta, dgamma, dbias = 0 and
// coef [2 cout] = dbeta / M, then dgamma invstd / M
int fpt_bwd_finalize_launch(int cout, const float *parts, int n_parts, long long M, const float *mean, const float *invstd, float *dbias,
                            float *dgamma, float *dbeta, float *coef, hipStream_t st);

}  // namespace ampnet
