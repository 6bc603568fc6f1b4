// seg_loss.hip -- the loss of the PointNet++ segmentation model behind its head (C ABI: ampnet_seg_nll_forward_f32,
// ampnet_seg_nll_backward_f32; the arithmetic: include/ampnet_hip.h).  Over the rows of logp [M][C] with targets [M]:
//     loss = sum_live w[t] * -logp[m, t] / sum_live w[t]      (torch's nll_loss(weight, ignore_index=-1, reduction='mean'))
//     pred = the lowest arg-max of the row                    counts = the confusion counts of (target, pred), ampnet_confusion_i64's layout
// in ONE pass over logp, where the torch composition (nll_loss, argmax, confusion_device) takes about eight launches over the same array.
//
// The pass moves 4 M C bytes (24 MB at M = 576 * 2048, C = 5: microseconds at HBM rate), so the cost is the launches.  Nothing here is
// tuned beyond that: one thread per row, a row's C floats read by plain loads (consecutive lanes read consecutive rows, a wave covers one
// contiguous span of 64 C floats), no vector loads, no LDS staging of the rows.
//
//   * forward: 256-thread workgroups, grid-stride over the rows, grid = min(cdiv(M, 256), SEGL_MAX_GRID).  The class weights and an int32
//     count table [C * C + 1] of the workgroup live in LDS; the table goes to the caller's int64 counts once per workgroup, by integer
//     atomics on its non-zero cells (exact, order-independent).  The two sums are float64 from the first addition on: per thread over its
//     rows ascending, across the wave by a butterfly of shuffles, across the waves through LDS in wave order.  A workgroup writes one
//     double[2] row of the workspace, and a second, one-workgroup kernel adds the rows ascending and writes sums and loss.
//   * every order above is a function of (M, C) alone: two runs give the same bits.  No float atomics.
//   * backward: one thread per row writes all C values of its row (zeros and the one entry), so the caller hands an uninitialised buffer:
//     no memset plus scatter.  The upstream gradient is read from device memory: no host synchronisation.  The C values a row can take,
//     (float)(-(w[c] g) / sums[1]) in float64, are formed once per workgroup in LDS.
#include "common.h"

namespace ampnet {

constexpr int SEGL_T = 256;
constexpr int SEGL_MAX_GRID = 1024;
constexpr int SEGL_MAX_C = AMPNET_SEG_HEAD_MAX_CLASSES;

inline int segl_grid(long long M)
{
    const long long g = (M + SEGL_T - 1) / SEGL_T;
    return (int)(g < SEGL_MAX_GRID ? g : SEGL_MAX_GRID);
}

__global__ __launch_bounds__(SEGL_T) void seg_nll_forward_kernel(const float *__restrict__ logp, long long M, int C,
                                                                const long long *__restrict__ target, const float *__restrict__ class_w,
                                                                double *__restrict__ parts, long long *__restrict__ preds,
                                                                unsigned long long *__restrict__ counts)
{
    __shared__ float s_w[SEGL_MAX_C];
    __shared__ unsigned int s_cnt[SEGL_MAX_C * SEGL_MAX_C + 1];
    __shared__ double s_red[SEGL_T / WAVE][2];
    const int tid = threadIdx.x;
    if (tid < C) s_w[tid] = class_w ? class_w[tid] : 1.0f;
    if (counts)
        for (int i = tid; i <= C * C; i += SEGL_T) s_cnt[i] = 0u;
    __syncthreads();
    double num = 0.0, den = 0.0;
    for (long long m = blockIdx.x * (long long)SEGL_T + tid; m < M; m += (long long)gridDim.x * SEGL_T) {
        const float *row = logp + (size_t)m * C;
        const long long t = target[m];
        const bool live = t >= 0 && t < C;
        float best = row[0], at_t = live && t == 0 ? best : 0.f;
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = row[c];
            if (v > best) {                                    // strict: the lowest class among equal largest entries
                best = v;
                arg = c;
            }
            if (live && c == (int)t) at_t = v;
        }
        if (live) {
            const double w = (double)s_w[t];
            num += w * -(double)at_t;                          // (the product of two floats is exact in float64)
            den += w;
        }
        if (preds) preds[m] = arg;
        if (counts) atomicAdd(&s_cnt[live ? (int)t * C + arg : C * C], 1u);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        num += __shfl_xor(num, off);
        den += __shfl_xor(den, off);
    }
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = num;
        s_red[tid >> 6][1] = den;
    }
    __syncthreads();
    if (tid == 0) {
        double a = s_red[0][0], b = s_red[0][1];
#pragma unroll
        for (int w = 1; w < SEGL_T / WAVE; ++w) {
            a += s_red[w][0];
            b += s_red[w][1];
        }
        parts[2 * blockIdx.x] = a;
        parts[2 * blockIdx.x + 1] = b;
    }
    if (counts)
        for (int i = tid; i <= C * C; i += SEGL_T)
            if (s_cnt[i]) atomicAdd(&counts[i], (unsigned long long)s_cnt[i]);
}

// one workgroup: the partial rows through LDS, then one thread adds them ascending
__global__ __launch_bounds__(SEGL_T) void seg_nll_finalize_kernel(const double *__restrict__ parts, int n, double *__restrict__ sums,
                                                                 float *__restrict__ loss)
{
    __shared__ double s_p[2 * SEGL_MAX_GRID];
    for (int i = threadIdx.x; i < 2 * n; i += SEGL_T) s_p[i] = parts[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = s_p[0], b = s_p[1];
        for (int i = 1; i < n; ++i) {
            a += s_p[2 * i];
            b += s_p[2 * i + 1];
        }
        sums[0] = a;
        sums[1] = b;
        loss[0] = (float)(a / b);                              // every row ignored: 0 / 0 = NaN, as torch
    }
}

__global__ __launch_bounds__(SEGL_T) void seg_nll_backward_kernel(const long long *__restrict__ target, const float *__restrict__ class_w,
                                                                 const double *__restrict__ sums, const float *__restrict__ grad_loss,
                                                                 long long M, int C, float *__restrict__ dlogp)
{
    // the C values a row can take, once per workgroup: the float64 quotient rounded ONCE.  (The float32 statement -(w g) / (float)sums[1]
    // rounds three times and can land 2.5 float32 ulp from the exact value; this is within half an ulp for the price of C divisions.)
    __shared__ float s_v[SEGL_MAX_C];
    if ((int)threadIdx.x < C)
        s_v[threadIdx.x] = (float)(-((double)(class_w ? class_w[threadIdx.x] : 1.0f) * (double)grad_loss[0]) / sums[1]);
    __syncthreads();
    for (long long m = blockIdx.x * (long long)SEGL_T + threadIdx.x; m < M; m += (long long)gridDim.x * SEGL_T) {
        const long long t = target[m];
        const bool live = t >= 0 && t < C;
        const float v = live ? s_v[t] : 0.f;                   // (a table entry is never read when every row is ignored: sums[1] == 0)
        float *row = dlogp + (size_t)m * C;
        for (int c = 0; c < C; ++c) row[c] = live && c == (int)t ? v : 0.f;
    }
}

static int segl_shape(const char *what, long long M, int C)
{
    AMPNET_REQUIRE(C >= 2 && C <= AMPNET_SEG_HEAD_MAX_CLASSES, "%s: C=%d classes must be in [2, %d]", what, C, AMPNET_SEG_HEAD_MAX_CLASSES);
    AMPNET_REQUIRE(M >= 1 && M <= AMPNET_SEG_HEAD_MAX_ROWS, "%s: M=%lld rows must be in [1, %lld]", what, M, (long long)AMPNET_SEG_HEAD_MAX_ROWS);
    return AMPNET_OK;
}

}  // namespace ampnet

using namespace ampnet;

extern "C" size_t ampnet_seg_nll_forward_workspace_bytes(long long M)
{
    if (segl_shape("ampnet_seg_nll_forward_workspace_bytes", M, 2) != AMPNET_OK) return 0;
    return (size_t)segl_grid(M) * 2 * sizeof(double);
}

extern "C" int ampnet_seg_nll_forward_f32(const float *logp, long long M, int C, const long long *target, const float *class_w, double *sums,
                                          float *loss, long long *preds, long long *counts, void *workspace, size_t workspace_bytes,
                                          void *stream)
{
    const char *what = "ampnet_seg_nll_forward_f32";
    AMPNET_REQUIRE(logp && target && sums && loss, "%s: null pointer", what);
    AMPNET_TRY(segl_shape(what, M, C));
    const int grid = segl_grid(M);
    const size_t need = (size_t)grid * 2 * sizeof(double);
    AMPNET_REQUIRE(workspace && workspace_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed", what, workspace ? workspace_bytes : 0,
                   need);
    AMPNET_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % sizeof(double) == 0, "%s: the workspace must be aligned to 8 bytes", what);
    hipStream_t st = (hipStream_t)stream;
    if (counts && hipMemsetAsync(counts, 0, (size_t)(C * C + 1) * sizeof(long long), st) != hipSuccess)
        return fail(AMPNET_E_LAUNCH, "%s: memset failed", what);
    double *parts = static_cast<double *>(workspace);
    hipLaunchKernelGGL(seg_nll_forward_kernel, dim3(grid), dim3(SEGL_T), 0, st, logp, M, C, target, class_w, parts, preds,
                       reinterpret_cast<unsigned long long *>(counts));
    hipLaunchKernelGGL(seg_nll_finalize_kernel, dim3(1), dim3(SEGL_T), 0, st, parts, grid, sums, loss);
    return check_launch("seg_nll_forward");
}

extern "C" int ampnet_seg_nll_backward_f32(const long long *target, const float *class_w, const double *sums, const float *grad_loss, long long M,
                                           int C, float *dlogp, void *stream)
{
    const char *what = "ampnet_seg_nll_backward_f32";
    AMPNET_REQUIRE(target && sums && grad_loss && dlogp, "%s: null pointer", what);
    AMPNET_TRY(segl_shape(what, M, C));
    const long long blocks = (M + SEGL_T - 1) / SEGL_T;
    const int grid = (int)(blocks < (1LL << 20) ? blocks : (1LL << 20));
    hipLaunchKernelGGL(seg_nll_backward_kernel, dim3(grid), dim3(SEGL_T), 0, (hipStream_t)stream, target, class_w, sums, grad_loss, M, C, dlogp);
    return check_launch("seg_nll_backward");
}
