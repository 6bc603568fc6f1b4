// bn_desc.h -- the BatchNorm state of one layer as the AMP-Net hot path (encoder, head, their backward) carries it: one descriptor per
// group of arrays, and ONE statement of the two formulas that turn merged sums into the constants the kernels apply.
//
// Who uses the formulas: bn_finalize_kernel, pool_finalize_bn_kernel (pw_misc.hip), bn_bwd_finalize_kernel and pw_input_wgrad_kernel
// (bwd_misc.hip) call bn_fwd_constants / bn_fwd_store and bn_bwd_constants.  The matrix-core kernels -- pw_gemm_kernel (pw_gemm.hip: the pfin prologue and the direct epilogue),
// pw_bwd_kernel (pw_bwd_fused.hip), pw_bwd_x3_kernel and pw_bwd_x3n_kernel (pw_bwd_x3.hip) -- keep their own lines under the rule of
// pw_bwd_common.h (a helper only where every instantiation keeps its register metadata and its instruction stream); each of those
// sites points here for the definition.  Compared on the device assembly: bn_fwd_constants / bn_fwd_store in the direct epilogue alone
// change all 131 instantiations of pw_gemm_kernel, bn_bwd_constants changes 11 of the 13 of pw_bwd_kernel; the split kernels state the
// same lines as pw_bwd_kernel and were left with them.
#pragma once
#include <cstddef>

namespace ampnet {

// forward products of a train-mode BatchNorm, each [n_slots, C]: y = z * scale + shift; mean / invstd are kept for the backward,
// smean / suvar (batch mean, unbiased variance) for the running-statistics update
struct BnFwd {
    float *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr, *smean = nullptr, *suvar = nullptr;
};
// the layer's parameters, [C]
struct BnLayer {
    const float *gamma = nullptr, *beta = nullptr;
};
// per-workgroup statistics partials a producer left: sum / sq [parts, C] = (mean, M2) of the rows[p] rows partial p covers;
// partial p belongs to slot p % n_slots, parts is a multiple of n_slots (empty partials carry rows 0)
struct BnPartials {
    const float *sum = nullptr, *sq = nullptr;
    const int *rows = nullptr;
    int parts = 0;
};
// "finish this BatchNorm": from the workgroup's own rows (PwGemm.fin) ...
struct BnFin {
    BnLayer layer;
    BnFwd out;
};
// ... or from the partials of the producer (PwGemm.pfin, PoolFinalize.pfin)
struct BnPfin {
    BnPartials part;
    BnLayer layer;
    BnFwd out;
};
// per-layer arrays of a workspace
struct BnSlot : BnFwd {
    int C = 0;
};

// backward products, [n_slots, C]: dz = P1 dy + P2 z + P3; slot_ab [n_slots, C, 2] = (sum dy, sum dy zhat) for the parameter gradients
struct BnBwd {
    float *P1 = nullptr, *P2 = nullptr, *P3 = nullptr, *slot_ab = nullptr;
};
// the backward products formed inside their consumer (PwBwd.fin, PwInputWgrad.fin): the producer's per-workgroup sums
// part_a / part_b [parts, C] (partial i belongs to slot i % n_slots), rows of one slot (uniform windows), the layer and its forward statistics
struct BnBwdFin {
    const float *part_a = nullptr, *part_b = nullptr;
    int parts = 0;
    int rows = 0;
    const float *gamma = nullptr, *mean = nullptr, *invstd = nullptr;   // [C], [n_slots, C] x2
    BnBwd out;
};

#if defined(__HIPCC__) || defined(__HIP__)
// merged (N rows, mean, M2) of one channel -> what the forward applies and keeps
struct BnFwdVal {
    float scale, shift, mean, invstd, uvar;
};
__device__ __forceinline__ BnFwdVal bn_fwd_constants(double N, double mean, double m2, float gamma, float beta, float eps)
{
    const double var = N > 0.0 ? m2 / N : 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma * invstd;
    return BnFwdVal{sc, beta - (float)mean * sc, (float)mean, invstd, (float)(N > 1.0 ? m2 / (N - 1.0) : m2)};
}
// element o of the arrays; mean / invstd and the smean / suvar pair are optional
__device__ __forceinline__ void bn_fwd_store(const BnFwd &out, size_t o, const BnFwdVal &v)
{
    out.scale[o] = v.scale;
    out.shift[o] = v.shift;
    if (out.mean) out.mean[o] = v.mean;
    if (out.invstd) out.invstd[o] = v.invstd;
    if (out.smean) {
        out.smean[o] = v.mean;
        out.suvar[o] = v.uvar;
    }
}
// A = sum dy, Bs = sum dy zhat over the n rows of one slot -> P1 = s, P2 = -s invstd Bs / n, P3 = -s A / n - P2 mean, s = gamma invstd.
// Returned for the caller's own rows and, if `write`, stored as element o of `out` with (A, Bs).
// EMPTY_OK: a slot with no row (n = 0) gets P2 = P3 = 0 -- the launched finalize can meet one; the in-kernel forms never do.
// (The stores sit between the two quotients on purpose: with both double divisions in one block bn_bwd_finalize_kernel needs more registers.)
struct BnBwdVal {
    float p1, p2, p3;
};
template <bool EMPTY_OK = false>
__device__ __forceinline__ BnBwdVal bn_bwd_constants(double A, double Bs, double n, float gamma, float invstd_f, float mean_f, const BnBwd &out, size_t o,
                                                     bool write)
{
    const double invstd = invstd_f, mean = mean_f;
    const double s = (double)gamma * invstd;
    const double p2 = (!EMPTY_OK || n > 0.0) ? -s * invstd * Bs / n : 0.0;
    BnBwdVal v;
    v.p1 = (float)s;
    v.p2 = (float)p2;
    if (write) {
        out.P1[o] = v.p1;
        out.P2[o] = v.p2;
    }
    v.p3 = (float)((!EMPTY_OK || n > 0.0) ? -s * A / n - p2 * mean : 0.0);
    if (write) {
        out.P3[o] = v.p3;
        out.slot_ab[o * 2 + 0] = (float)A;
        out.slot_ab[o * 2 + 1] = (float)Bs;
    }
    return v;
}
#endif

}  // namespace ampnet
