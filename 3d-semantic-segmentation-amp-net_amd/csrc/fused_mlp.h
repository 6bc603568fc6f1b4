// fused_mlp.h -- the shared MLP  relu(bn_eval(W row + b))  x <= 3 layers of the fused PointNet++ forwards, on rows a wave keeps in LDS
// (set_abstraction.hip, feature_propagation.hip; host side and the BatchNorm fold kernel: fused_mlp.hip).
//
//   * A wave owns R = 32 or 64 rows; 32 of them are the M tile of v_mfma_f32_32x32x2_f32 (exact fp32: the matrix-precision scope is not
//     consulted).  Lane (r = l & 31, h = l >> 5) supplies row r of A and row n0 + r of W, the accumulator holds column n0 + r of rows
//     mlp_acc_row(i, h), i < 16.  The ORDER of the contraction inside a block of 8 is the caller's (KORDER): it fixes the
//     summation order and so the bits.  K_PAIRS: k-step i < 4 takes k = k0 + 2 i + h.  K_QUADS: k = k0 + 4 h + i, a lane's four weights are
//     16 contiguous bytes, and unstaged weights with cin a multiple of 8 (plan.w_vec) are read with one global_load_dwordx4 per lane and
//     block, a quarter of the cache lines per MFMA that four strided dwords touch.
//   * LDS rows have an ODD stride in floats.  ds_read_b32 / ds_write_b32 conflict inside a 32-lane half on (address / 4) % 32: the
//     operand reads walk r at a fixed k (32 rows, odd stride -> 32 banks), the epilogue's stores walk the column at a fixed row.
//   * Two tiles per wave ping-pong: layer 0 reads A (the caller built the rows there, kp[0] columns, zeros past cin[0]) and writes B,
//     layer 1 reads B and writes A; the last layer's relu'd accumulators go to the caller's EPILOGUE and never to LDS.
//   * BatchNorm is folded once per call, ahead of the main kernel, into scale = gamma / sqrt(var + eps) and
//     shift = (b - mean) * scale + beta (sa_fold_kernel; the parameters live in device memory), applied as fma(acc, scale, shift).
//   * A layer's weights are staged in LDS (rows padded to the odd stride, once per workgroup) while they fit next to the waves' tiles, in
//     layer order; the layers that do not fit are read through L2 by the same lane map.  The plan halves the waves per workgroup (4, 2, 1)
//     until their tiles fit the 160 KB LDS.
#pragma once
#include "common.h"
#include "mfma_types.h"

namespace ampnet {


constexpr int MLP_MAX_LAYERS = AMPNET_SA_MAX_LAYERS;
constexpr int MLP_MAX_COUT = AMPNET_SA_MAX_COUT;
constexpr int MLP_LDS_BYTES = 160 * 1024;
static_assert(AMPNET_FP_MAX_LAYERS == MLP_MAX_LAYERS && AMPNET_FP_MAX_COUT == MLP_MAX_COUT, "one plan and one fold serve both forwards");

enum { K_PAIRS, K_QUADS };

// the lane map of the header, once: the row (of the 32-row tile) that accumulator register i < 16 of lane half h holds
__device__ __forceinline__ constexpr int mlp_acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

struct MlpPlan {
    int L, nw, R;                         // layers, waves per workgroup, rows of a wave's tile (32 / 64)
    int cin[MLP_MAX_LAYERS], cout[MLP_MAX_LAYERS];
    int kp[MLP_MAX_LAYERS];               // contraction length padded to a multiple of 8 (zeros)
    int ld_a, ld_b;                       // odd row strides of the two tiles, floats
    int w_off[MLP_MAX_LAYERS];            // float offset of the layer's staged weights in LDS, -1 = read through L2
    int w_vec[MLP_MAX_LAYERS];            // global weights: rows are 16-byte aligned and cin % 8 == 0 -> K_QUADS loads dwordx4
    int fold_off[MLP_MAX_LAYERS];         // float offset of the layer's scale[cout], shift[cout] in the workspace
    const float *w[MLP_MAX_LAYERS];
};

struct MlpFold {                          // what sa_fold_kernel reads besides the plan's L, cout and fold_off
    const float *bias[MLP_MAX_LAYERS], *gamma[MLP_MAX_LAYERS], *beta[MLP_MAX_LAYERS], *mean[MLP_MAX_LAYERS], *var[MLP_MAX_LAYERS];
    float eps[MLP_MAX_LAYERS];
};

// Checks the layers (`what`, the entry point's name, opens every message), fills p and f for rows_per_wave rows per wave and returns the
// dynamic LDS bytes of the launch; 0 after a failure (ampnet_last_error is set, the code is AMPNET_E_ARG).
int mlp_plan_build(const char *what, int cin0, int rows_per_wave, const float *const *params_host, const int *cout_host, const float *eps_host,
                   int L, MlpPlan &p, MlpFold &f);
// launches sa_fold_kernel on `st`: fold[off_l .. off_l + cout_l) = scale_l, the next cout_l floats shift_l
int mlp_fold_launch(const MlpPlan &p, const MlpFold &f, float *fold, hipStream_t st);
// raises the kernel's dynamic LDS limit to MLP_LDS_BYTES, once per kernel (`done` is the caller's latch)
int mlp_allow_full_lds(const char *what, const void *kernel, bool &done);
// Every workgroup stages the weights once: at most 4 workgroups per CU's worth of them, each wave walking several items (groups, row
// tiles).  This is min(cdiv(items, nw), 1024), written so that items near 2^31 do not overflow.
inline int mlp_grid(int items, int nw) { return items / nw >= 1024 ? 1024 : cdiv(items, nw); }
// the plan of a kernel that is one wave per workgroup and stages no weights: every layer is read through L2
inline void mlp_plan_unstaged(MlpPlan &p)
{
    p.nw = 1;
    for (int l = 0; l < p.L; ++l) p.w_off[l] = -1;
}

// orders a wave's own LDS writes before its later LDS reads (every tile is private to one wave)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the workgroup's LDS: per wave tile A [R][ld_a] and tile B [R][ld_b], then the staged weights
struct MlpLds {
    float *tile_a, *tile_b, *s_w;
};

__device__ __forceinline__ MlpLds mlp_lds(const MlpPlan &p, int R, float *s_mem, int wave)
{
    const int tile_floats = R * (p.ld_a + p.ld_b);
    float *tile_a = s_mem + wave * tile_floats;
    return {tile_a, tile_a + R * p.ld_a, s_mem + p.nw * tile_floats};
}

// stage the weights that fit: [cout][kp + 1], columns past cin zero.  The caller's __syncthreads() publishes them.
__device__ __forceinline__ void mlp_stage_weights(const MlpPlan &p, float *s_w, int tid, int nthreads)
{
    for (int l = 0; l < p.L; ++l) {
        if (p.w_off[l] < 0) continue;
        const int ldw = p.kp[l] + 1, cin = p.cin[l], total = p.cout[l] * p.kp[l];
        const float *__restrict__ src = p.w[l];
        float *dstw = s_w + p.w_off[l];
        for (int e = tid; e < total; e += nthreads) {
            const int o = e / p.kp[l], k = e - o * p.kp[l];
            dstw[o * ldw + k] = k < cin ? src[(size_t)o * cin + k] : 0.0f;
        }
    }
}

// An EPILOGUE takes the values v = relu(fma(acc, scale, shift)) of one call of mlp_tiles: init() starts a lane's state for one output
// column, put() takes the value of (row, col), done() ends the column after the last row tile.  `dst`, the last layer's output in global
// memory, reaches them as a __restrict__ parameter of every function on the way down (a struct member cannot carry the qualifier): the
// compiler may then order the weight loads and the output stores freely.  This epilogue stores to the wave's other tile.
struct MlpToTile {
    float *y;
    int ldy;
    __device__ static float init() { return 0.0f; }
    __device__ void put(float &, float *, int row, int col, float v) const { y[row * ldy + col] = v; }
    __device__ static void done(float, float *, int, int) {}
};

// what mlp_accumulate takes as xr: the operand pointer of the lane of half h that supplies row `row` of x [.][ldx]
template <int KORDER>
__device__ __forceinline__ const float *mlp_operand(const float *x, int ldx, int row, int h)
{
    return x + row * ldx + (KORDER == K_PAIRS ? 1 : 4) * h;
}

// The raw accumulator outside the forward: acc = W x for NT column tiles from n0 on the 32 rows whose operand pointer is xr, k ascending in
// blocks of 8 in the order KORDER names.  Every backward and train-mode kernel that has to find the forward's bits again (its ReLU mask, its
// max, its statistics) runs this one loop; it is mlp_tiles' loop below, statement for statement, and the two must stay so.  (mlp_tiles does
// not call it: hipcc lays the forward kernels' blocks out differently when the loop arrives through a call, and the forward stays as it
// was tuned.)  w: weights [cout][ldw], k_valid = columns of w that exist (the rest of kp counts as zero); VEC: 16-byte aligned rows,
// k_valid == kp.  Lane (r, h) ends with column n0 + 32 t + r of row mlp_acc_row(i, h) in acc[t][i].
template <int NT, int KORDER, bool VEC>
__device__ __forceinline__ void mlp_accumulate(f32x16 (&acc)[NT], const float *xr, const float *__restrict__ w, int ldw, int k_valid, int kp, int n0,
                                               int r, int h)
{
    static_assert(!VEC || KORDER == K_QUADS, "only K_QUADS gives a lane four contiguous weights");
    constexpr int KH = KORDER == K_PAIRS ? 1 : 4, KI = KORDER == K_PAIRS ? 2 : 1;      // k-step i of lane half h takes k = k0 + KH h + KI i
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    for (int k0 = 0; k0 < kp; k0 += 8) {
        float av[4], bv[NT][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = xr[k0 + KI * i];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float *wr = w + (size_t)(n0 + 32 * t + r) * ldw + k0 + KH * h;
            if (VEC) {
                const float4 q = *reinterpret_cast<const float4 *>(wr);
                bv[t][0] = q.x;
                bv[t][1] = q.y;
                bv[t][2] = q.z;
                bv[t][3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) bv[t][i] = k0 + KH * h + KI * i < k_valid ? wr[KI * i] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
}

// NT column tiles of one layer over the R / 32 row tiles of the wave.  x: the wave's input tile [R][ldx]; w: weights [cout][ldw] (LDS or
// global), k_valid = columns of w that exist (the rest of kp counts as zero); VEC: w is global, 16-byte aligned rows, k_valid == kp.
template <int NT, int KORDER, bool VEC, class EPILOGUE>
__device__ __forceinline__ void mlp_tiles(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int R, int n0,
                                          const float *__restrict__ scale, const float *__restrict__ shift, const EPILOGUE &ep,
                                          float *__restrict__ dst, int lane)
{
    static_assert(!VEC || KORDER == K_QUADS, "only K_QUADS gives a lane four contiguous weights");
    constexpr int KH = KORDER == K_PAIRS ? 1 : 4, KI = KORDER == K_PAIRS ? 2 : 1;      // k-step i of lane half h takes k = k0 + KH h + KI i
    const int r = lane & 31, h = lane >> 5;
    float sc[NT], sh[NT], st[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sc[t] = scale[n0 + 32 * t + r];
        sh[t] = shift[n0 + 32 * t + r];
        st[t] = EPILOGUE::init();
    }
    for (int m0 = 0; m0 < R; m0 += 32) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
        const float *xr = x + (m0 + r) * ldx + KH * h;
        for (int k0 = 0; k0 < kp; k0 += 8) {
            float av[4], bv[NT][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = xr[k0 + KI * i];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float *wr = w + (size_t)(n0 + 32 * t + r) * ldw + k0 + KH * h;
                if (VEC) {
                    const float4 q = *reinterpret_cast<const float4 *>(wr);
                    bv[t][0] = q.x;
                    bv[t][1] = q.y;
                    bv[t][2] = q.z;
                    bv[t][3] = q.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) bv[t][i] = k0 + KH * h + KI * i < k_valid ? wr[KI * i] : 0.0f;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[t][i], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                ep.put(st[t], dst, m0 + mlp_acc_row(i, h), n0 + 32 * t + r, fmaxf(fmaf(acc[t][i], sc[t], sh[t]), 0.0f));
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) ep.done(st[t], dst, n0 + 32 * t + r, h);
}

// one layer: its cout / 32 column tiles, four at a time (four independent accumulator chains), then two, then one
template <int KORDER, bool VEC, class EPILOGUE>
__device__ __forceinline__ void mlp_layer(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int R, int cout,
                                          const float *__restrict__ scale, const float *__restrict__ shift, const EPILOGUE &ep,
                                          float *__restrict__ dst, int lane)
{
    int n0 = 0;
    for (; n0 + 128 <= cout; n0 += 128) mlp_tiles<4, KORDER, VEC>(x, ldx, w, ldw, k_valid, kp, R, n0, scale, shift, ep, dst, lane);
    if (n0 + 64 <= cout) {
        mlp_tiles<2, KORDER, VEC>(x, ldx, w, ldw, k_valid, kp, R, n0, scale, shift, ep, dst, lane);
        n0 += 64;
    }
    if (n0 + 32 <= cout) mlp_tiles<1, KORDER, VEC>(x, ldx, w, ldw, k_valid, kp, R, n0, scale, shift, ep, dst, lane);
}

// layer l from its weight source: staged in LDS, global by dwordx4 (K_QUADS only), global by dwords
template <int KORDER, class EPILOGUE>
__device__ __forceinline__ void mlp_dispatch(const MlpPlan &p, int l, int R, const float *s_w, const float *x, int ldx,
                                             const float *__restrict__ fold, const EPILOGUE &ep, float *__restrict__ dst, int lane)
{
    const float *scale = fold + p.fold_off[l], *shift = scale + p.cout[l];
    if (p.w_off[l] >= 0) {
        mlp_layer<KORDER, false>(x, ldx, s_w + p.w_off[l], p.kp[l] + 1, p.kp[l], p.kp[l], R, p.cout[l], scale, shift, ep, dst, lane);
        return;
    }
    if constexpr (KORDER == K_QUADS)
        if (p.w_vec[l]) {
            mlp_layer<KORDER, true>(x, ldx, p.w[l], p.cin[l], p.cin[l], p.kp[l], R, p.cout[l], scale, shift, ep, dst, lane);
            return;
        }
    mlp_layer<KORDER, false>(x, ldx, p.w[l], p.cin[l], p.cin[l], p.kp[l], R, p.cout[l], scale, shift, ep, dst, lane);
}

// All layers on the rows the caller built in tile A (and ordered with wave_lds_sync()); the last layer's values go to `last` and `dst`.
// R: the wave's rows, a multiple of 32 (a literal where the caller has one row tile: the row-tile loop then folds away).
template <int KORDER, class EPILOGUE>
__device__ __forceinline__ void mlp_run(const MlpPlan &p, int R, const float *s_w, float *tile_a, float *tile_b, const float *__restrict__ fold,
                                        const EPILOGUE &last, float *__restrict__ dst, int lane)
{
    float *x = tile_a, *y = tile_b;
    int ldx = p.ld_a, ldy = p.ld_b;
    for (int l = 0; l < p.L; ++l) {
        if (l == p.L - 1) {                                 // (one loop with the test inside: the form hipcc schedules best)
            mlp_dispatch<KORDER>(p, l, R, s_w, x, ldx, fold, last, dst, lane);
        } else {
            mlp_dispatch<KORDER>(p, l, R, s_w, x, ldx, fold, MlpToTile{y, ldy}, dst, lane);
            wave_lds_sync();
            float *nx = y;
            y = x;
            x = nx;
            const int t = ldx;
            ldx = ldy;
            ldy = t;
        }
    }
}

}  // namespace ampnet
