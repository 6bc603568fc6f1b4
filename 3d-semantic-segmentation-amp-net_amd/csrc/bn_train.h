// bn_train.h -- the train-mode BatchNorm that feature_propagation_train.hip and set_abstraction_train.hip share.  The two files differ in
// how a wave's rows come to be (fp_rows.h / the group gather), in their tiling and in the last layer (set abstraction's max); everything
// from the rows to the statistics and back is here, once:
//   * the tile core, templated on <NT, KORDER, VEC> as fused_mlp.h's mlp_accumulate, which forms the raw accumulators a = W x in the
//     forward's order: bnt_tile_stats (a 32-row tile's count, mean, M2 merged into the wave's partial row), bnt_form_dy (part B of a
//     backward phase: dy and its two sums) and bnt_form_dz (part A: dz through the statistics);
//   * Chan's merge of the centred statistics;
//   * the backward's plan (BntBwd) and the host code that fills it, and the row-count limits of the batch statistics;
//   * the launchers of the kernels that do not depend on how the rows are built (bn_train.hip): the statistics finalize, the fold from the
//     saved statistics, the backward's finalize.
// One wrong mask or a swapped summation order here changes bits silently in both paths: the masks (rows past `rows` enter nothing) and the
// orders (the accumulator's 16 rows ascending, lane half 0 before half 1, tiles ascending into a row that ONE lane owns) are what the
// bit-exact tests of both paths pin.
#pragma once
#include "mlp_bwd.h"

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

// The statistics of NT column tiles from n0 of a layer over the first `rows` of the 32 rows from m0 of x [.][ldx] (w [cout][cin] global),
// merged into the wave's partial row: two passes over the accumulators (mean, then the squared deviations from it), the lane halves joined by
// __shfl_xor, then Chan's merge by the lane of half 0, which alone ever touches these three words of the partials.
template <int NT, int KORDER, bool VEC>
__device__ __forceinline__ void bnt_tile_stats(const float *x, int ldx, int m0, const float *__restrict__ w, int cin, int kp, int n0, int rows,
                                               float *part_n, float *part_mean, float *part_m2, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    mlp_accumulate<NT, KORDER, VEC>(acc, mlp_operand<KORDER>(x, ldx, m0 + r, h), w, cin, cin, kp, n0, r, h);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (mlp_acc_row(i, h) < rows) sum += acc[t][i];
        sum += __shfl_xor(sum, 32);
        const float mean = sum / (float)rows;
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (mlp_acc_row(i, h) < rows) {
                const float d = acc[t][i] - mean;
                q = fmaf(d, d, q);
            }
        q += __shfl_xor(q, 32);
        if (h == 0) {
            float nA = part_n[col], meanA = part_mean[col], m2A = part_m2[col];
            fpt_chan(nA, meanA, m2A, (float)rows, mean, q);
            part_n[col] = nA;
            part_mean[col] = meanA;
            part_m2[col] = m2A;
        }
    }
}

// Part A of a backward phase: a of layer j recomputed on tile x; dy of the tile's rows from dz_ws or, arg_g != nullptr (set abstraction's
// last layer, whose dy has one nonzero per group and column), dout_g at the row arg_g names when its y > 0; dz through the statistics into
// tile d and into dz_ws (over dy).  row0: the tile's first row inside its group.  Pass arg_g and dout_g as literal nullptr where they are
// never set: the branch and the read of `shift` then fold away.
template <int NT, int KORDER, bool VEC>
__device__ __forceinline__ void bnt_form_dz(const float *x, int ldx, const float *__restrict__ w, int cin, int kp, int cout, int n0,
                                            const float *__restrict__ scale, const float *__restrict__ shift, const float *__restrict__ mean,
                                            const float *__restrict__ c1, const float *__restrict__ c2, float *d, int ldd, int rows, int row0,
                                            const int32_t *__restrict__ arg_g, const float *__restrict__ dout_g, float *dz_ws, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    mlp_accumulate<NT, KORDER, VEC>(acc, mlp_operand<KORDER>(x, ldx, r, h), w, cin, cin, kp, n0, r, h);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        const float sc = scale[col], sh = shift[col], mu = mean[col], k1 = c1[col], k2 = c2[col];
        const int arow = arg_g ? arg_g[col] - row0 : -1;
        const float dsel = arg_g ? dout_g[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mlp_acc_row(i, h);
            float dzv = 0.0f;
            if (row < rows) {
                const float a = acc[t][i];
                float dy;
                if (arg_g) dy = row == arow && fmaf(a, sc, sh) > 0.0f ? dsel : 0.0f;
                else dy = dz_ws[(size_t)row * cout + col];
                dzv = sc * fmaf(-(a - mu), k2, dy - k1);
                dz_ws[(size_t)row * cout + col] = dzv;
            }
            d[row * ldd + col] = dzv;
        }
    }
}

// Part B of a backward phase: a of layer l recomputed on tile x; dy = dx [y > 0] to dz_ws, and sum dy, sum dy a added into the workgroup's
// partial row by the lane of half 0, which alone ever touches these two words of the partials.  dx comes from tile d or, DOUT and dout !=
// nullptr, from `dout` (global, row stride cout).  With DOUT dx is read BEFORE the mask is known, without it the tile is read under the mask:
// the same values, but each phase kernel keeps the form its registers were budgeted for (sat_bwd_phase_kernel spills with the other one).
template <int NT, int KORDER, bool VEC, bool DOUT>
__device__ __forceinline__ void bnt_form_dy(const float *x, int ldx, const float *__restrict__ w, int cin, int kp, int cout, int n0,
                                            const float *__restrict__ scale, const float *__restrict__ shift, const float *d, int ldd,
                                            const float *__restrict__ dout, int rows, float *dz_ws, float *part_b, float *part_g, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    mlp_accumulate<NT, KORDER, VEC>(acc, mlp_operand<KORDER>(x, ldx, r, h), w, cin, cin, kp, n0, r, h);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        const float sc = scale[col], sh = shift[col];
        float sb = 0.0f, sg = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mlp_acc_row(i, h);
            const float a = acc[t][i];
            float dy = 0.0f;
            if (row < rows) {
                if (DOUT) {
                    const float din = dout ? dout[(size_t)row * cout + col] : d[row * ldd + col];
                    dy = fmaf(a, sc, sh) > 0.0f ? din : 0.0f;
                } else {
                    dy = fmaf(a, sc, sh) > 0.0f ? d[row * ldd + col] : 0.0f;
                }
                dz_ws[(size_t)row * cout + col] = dy;
            }
            sb += dy;
            sg = fmaf(dy, a, sg);
        }
        const float ob = __shfl_down(sb, 32), og = __shfl_down(sg, 32);
        if (h == 0) {
            part_b[col] += sb + ob;
            part_g[col] += sg + og;
        }
    }
}

// the plan of a backward's phase kernels: two LDS tiles of 32 rows and the workspace arrays
struct BntBwd {
    int ld;                                                    // odd row stride of both LDS tiles
    int ldxs[MLP_MAX_LAYERS];                                  // row stride of x_l in the workspace: cin_l rounded up to 32 (zeros)
    float *xs[MLP_MAX_LAYERS], *dz[MLP_MAX_LAYERS], *dx0, *parts, *coef;     // coef: per layer (fold_off) dbeta / M, then dgamma invstd / M
    const float *mean[MLP_MAX_LAYERS];
    int32_t *arg;                                              // set abstraction: [n_groups][cout_{L-1}], the row the max selected; else null
};

// fills b (arg stays null) from the plan, the fold's save_mean and the layout's offsets into ws, the coefficients at float offset off_coef;
// returns the dynamic LDS bytes of a phase kernel: two tiles of 32 rows of the widest layer input or output, plus one float
size_t bnt_bwd_plan(const MlpPlan &p, const MlpFold &f, const MlpBwdLayout &lay, float *ws, size_t off_coef, BntBwd &b);

// the two limits of the batch statistics on top of the eval entry points' (`what` opens the message; rows_text says what M is the product of).
// With a registered collective the statistics are the GLOBAL batch's and its merged row count must be an exact float too: the call then
// also refuses M * world_size > max_rows -- a host-side rule, conservative because the ranks' row counts differ and no rank knows the others'.
int bnt_rows_ok(const char *what, long long M, long long max_rows, const char *rows_text);

struct FptStats {                         // what the finalize of pass l reads and writes
    const float *bias, *gamma, *beta;
    float *running_mean, *running_var, *save_mean, *save_invstd;
    float eps, momentum;
    int cout, fold_off;
};

// The two finalize launchers follow a registered collective (kernels.h: sync_bn_on()): each call then issues exactly ONE exchange through
// sync_bn_exchange, whatever the data, so every rank must make the same sequence of calls; a failing callback comes back as the launcher's
// status.  Forward: the rank's partial rows packed into one row (n, mean, M2)[cout], all-gathered, finalized over the ranks' rows in rank order
// with the MERGED row count (M is not used) -- every rank writes the same fold, saved and running statistics, bit for bit.  Backward: dbeta,
// dgamma, dbias stay the rank's own sums (the gradient all-reduce adds them); (sum dy, sum dy a)[cout] and M are all-reduced and coef comes
// from the global sums.  With one rank both reproduce the plain path's bits.
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
