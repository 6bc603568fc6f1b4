// fused_mlp_bf16.h -- the bf16 sibling of fused_mlp.h: the same MLP  relu(bn_eval(W row + b))  x <= 3 layers on rows a wave keeps in LDS, with
// the matrix products on v_mfma_f32_32x32x16_bf16 (set_abstraction_bf16.hip, feature_propagation_bf16.hip; host side and the weight
// conversion kernel: fused_mlp_bf16.hip).  The rounding model is stated in include/ampnet_hip.h (ampnet_sa_forward_bf16): the input row
// and every weight are rounded to bf16 once, a layer accumulates in fp32 and applies relu(fma(acc, scale, shift)) in fp32, the result is
// rounded to bf16 on its way to the next layer's tile, and the last layer's values reach the caller's EPILOGUE as fp32.
//
//   * A wave owns R = 32 or 64 rows; 32 of them are the M tile of the MFMA.  Lane (r = l & 31, h = l >> 5) supplies A[row r][k = 8 h + j]
//     and B[k = 8 h + j][col n0 + r], j < 8: eight contiguous bf16 of a row of x and of a row of W, one 16-byte read each.  The
//     accumulator layout is the fp32 instruction's (mlp_acc_row), so the epilogues of fused_mlp.h's callers carry over.  k ascends in
//     blocks of 16; the order of the sum is a function of the shape alone.
//   * Contraction lengths are padded to a multiple of 16 with zeros (layer 0: by the row builder and the weight conversion; the other
//     layers' cin is a multiple of 32).
//   * LDS rows -- both tiles and the staged weights -- have a stride of 8 * odd bf16 = 16 * odd bytes (kp + 8, cout + 8).  ds_read_b128
//     serves four groups of 16 lanes, each of them 16 rows r that are distinct mod 16 at one h: their 16-byte slots (r * odd + const)
//     mod 16 are distinct, so the operand reads are conflict-free.  The epilogue's stores walk the column at a fixed row: the 32 lanes of
//     a half write 64 contiguous bytes, the other half four rows on (64 * odd bytes: the other 16 banks); two lanes share a dword, each
//     writing its own half of it with ds_write_b16.  What that sharing costs is not measured.
//   * Two tiles per wave ping-pong exactly as in fused_mlp.h.
//   * The weights arrive as bf16 [cout][kp] rows (mlp_bf16_weights_kernel writes them into the workspace once per call, behind the
//     BatchNorm fold).  A layer is staged in LDS while it fits next to the waves' tiles, in layer order, by 16-byte copies; the layers
//     that do not fit are read through L2 by the same lane map, one global_load_dwordx4 per lane and block of 16.  The plan halves the
//     waves per workgroup (4, 2, 1) until their tiles fit the 160 KB LDS.
#pragma once
#include "fused_mlp.h"

namespace ampnet {

// a host rule of a function that answers 0 after a failure (a size, the LDS bytes of a plan): ampnet_last_error is set, AMPNET_E_ARG
#define MLP_BF16_REQUIRE(cond, ...)               \
    do {                                          \
        if (!(cond)) {                            \
            ::ampnet::fail(AMPNET_E_ARG, __VA_ARGS__); \
            return 0;                             \
        }                                         \
    } while (0)

constexpr int MLP_BF16_PAD = 8;          // bf16 elements between the rows of an LDS image: kp + 8 and cout + 8 are 8 * odd

struct MlpPlanBf16 {
    int L, nw, R;                         // layers, waves per workgroup, rows of a wave's tile (32 / 64)
    int cin[MLP_MAX_LAYERS], cout[MLP_MAX_LAYERS];
    int kp[MLP_MAX_LAYERS];               // contraction length padded to a multiple of 16 (zeros)
    int ld_a, ld_b;                       // row strides of the two tiles, bf16 elements
    int w_off[MLP_MAX_LAYERS];            // bf16 offset of the layer's staged weights in LDS, -1 = read through L2
    int wb_off[MLP_MAX_LAYERS];           // bf16 offset of the layer's converted weights [cout][kp] in the workspace's weight region
    int fold_off[MLP_MAX_LAYERS];         // float offset of the layer's scale[cout], shift[cout] in the workspace
    const float *w[MLP_MAX_LAYERS];       // the fp32 weights [cout][cin] (read by the conversion only)
};

// bytes of the bf16 weight region for layers of widths cout_host behind cin0 (the region starts MLP_BF16_FOLD_BYTES into the workspace);
// checks the widths as mlp_plan_build does.  0 after a failure (ampnet_last_error is set).
constexpr size_t MLP_BF16_FOLD_BYTES = (size_t)MLP_MAX_LAYERS * 2 * MLP_MAX_COUT * sizeof(float);
size_t mlp_bf16_weight_bytes(const char *what, int cin0, const int *cout_host, int L);
// mlp_plan_build (its checks, the fold's inputs f and the plan p32 the fold launch takes), then the bf16 plan p for rows_per_wave rows per
// wave.  Returns the dynamic LDS bytes of the launch; 0 after a failure.
int mlp_bf16_plan_build(const char *what, int cin0, int rows_per_wave, const float *const *params_host, const int *cout_host,
                        const float *eps_host, int L, MlpPlan &p32, MlpFold &f, MlpPlanBf16 &p);
// launches mlp_bf16_weights_kernel on `st`: wb[wb_off_l + o kp_l + k] = bf16(W_l[o][k]), zeros for cin_l <= k < kp_l
int mlp_bf16_weights_launch(const MlpPlanBf16 &p, __bf16 *wb, hipStream_t st);

// the workgroup's LDS: per wave tile A [R][ld_a] and tile B [R][ld_b], then the staged weights
struct MlpLdsBf16 {
    __bf16 *tile_a, *tile_b, *s_w;
};

__device__ __forceinline__ MlpLdsBf16 mlp_bf16_lds(const MlpPlanBf16 &p, int R, __bf16 *s_mem, int wave)
{
    const int tile_elems = R * (p.ld_a + p.ld_b);
    __bf16 *tile_a = s_mem + wave * tile_elems;
    return {tile_a, tile_a + R * p.ld_a, s_mem + p.nw * tile_elems};
}

// stage the weights that fit: [cout][kp + 8] from the converted rows [cout][kp], 16 bytes at a time.  The caller's __syncthreads()
// publishes them.
__device__ __forceinline__ void mlp_bf16_stage_weights(const MlpPlanBf16 &p, __bf16 *s_w, const __bf16 *__restrict__ wb, int tid, int nthreads)
{
    for (int l = 0; l < p.L; ++l) {
        if (p.w_off[l] < 0) continue;
        const int chunks = p.kp[l] / 8, ldw = p.kp[l] + MLP_BF16_PAD, total = p.cout[l] * chunks;
        const __bf16 *src = wb + p.wb_off[l];
        __bf16 *dstw = s_w + p.w_off[l];
        for (int e = tid; e < total; e += nthreads) {
            const int o = e / chunks, c = e - o * chunks;
            *reinterpret_cast<u32x4 *>(dstw + o * ldw + 8 * c) = *reinterpret_cast<const u32x4 *>(src + (size_t)o * p.kp[l] + 8 * c);
        }
    }
}

// the epilogue of every layer but the last: round to bf16 and store to the wave's other tile
struct MlpToTileBf16 {
    __bf16 *y;
    int ldy;
    __device__ static float init() { return 0.0f; }
    __device__ void put(float &, float *, int row, int col, float v) const { y[row * ldy + col] = (__bf16)v; }
    __device__ static void done(float, float *, int, int) {}
};

// NT column tiles of one layer over the R / 32 row tiles of the wave.  x: the wave's input tile [R][ldx]; w: weights [cout][ldw] (LDS or
// the workspace), kp columns of each row exist.  EPILOGUE as in fused_mlp.h.
template <int NT, class EPILOGUE>
__device__ __forceinline__ void mlp_bf16_tiles(const __bf16 *x, int ldx, const __bf16 *w, int ldw, int kp, int R, int n0,
                                               const float *__restrict__ scale, const float *__restrict__ shift, const EPILOGUE &ep,
                                               float *__restrict__ dst, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    float sc[NT], sh[NT], st[NT];
    const __bf16 *wr[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sc[t] = scale[n0 + 32 * t + r];
        sh[t] = shift[n0 + 32 * t + r];
        st[t] = EPILOGUE::init();
        wr[t] = w + (size_t)(n0 + 32 * t + r) * ldw + 8 * h;
    }
    for (int m0 = 0; m0 < R; m0 += 32) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
        const __bf16 *xr = x + (m0 + r) * ldx + 8 * h;
        for (int k0 = 0; k0 < kp; k0 += 16) {
            const bf16x8 av = *reinterpret_cast<const bf16x8 *>(xr + k0);
            bf16x8 bv[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const bf16x8 *>(wr[t] + k0);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv[t], acc[t], 0, 0, 0);
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

// one layer: its cout / 32 column tiles, four at a time, then two, then one (the walk of fused_mlp.h)
template <class EPILOGUE>
__device__ __forceinline__ void mlp_bf16_layer(const __bf16 *x, int ldx, const __bf16 *w, int ldw, int kp, int R, int cout,
                                               const float *__restrict__ scale, const float *__restrict__ shift, const EPILOGUE &ep,
                                               float *__restrict__ dst, int lane)
{
    int n0 = 0;
    for (; n0 + 128 <= cout; n0 += 128) mlp_bf16_tiles<4>(x, ldx, w, ldw, kp, R, n0, scale, shift, ep, dst, lane);
    if (n0 + 64 <= cout) {
        mlp_bf16_tiles<2>(x, ldx, w, ldw, kp, R, n0, scale, shift, ep, dst, lane);
        n0 += 64;
    }
    if (n0 + 32 <= cout) mlp_bf16_tiles<1>(x, ldx, w, ldw, kp, R, n0, scale, shift, ep, dst, lane);
}

// layer l from its weight source: staged in LDS, or the converted rows in the workspace through L2
template <class EPILOGUE>
__device__ __forceinline__ void mlp_bf16_dispatch(const MlpPlanBf16 &p, int l, int R, const __bf16 *s_w, const __bf16 *__restrict__ wb,
                                                  const __bf16 *x, int ldx, const float *__restrict__ fold, const EPILOGUE &ep,
                                                  float *__restrict__ dst, int lane)
{
    const float *scale = fold + p.fold_off[l], *shift = scale + p.cout[l];
    if (p.w_off[l] >= 0)
        mlp_bf16_layer(x, ldx, s_w + p.w_off[l], p.kp[l] + MLP_BF16_PAD, p.kp[l], R, p.cout[l], scale, shift, ep, dst, lane);
    else
        mlp_bf16_layer(x, ldx, wb + p.wb_off[l], p.kp[l], p.kp[l], R, p.cout[l], scale, shift, ep, dst, lane);
}

// All layers on the rows the caller built in tile A (and ordered with wave_lds_sync()); the last layer's fp32 values go to `last` and `dst`.
template <class EPILOGUE>
__device__ __forceinline__ void mlp_bf16_run(const MlpPlanBf16 &p, int R, const __bf16 *s_w, const __bf16 *__restrict__ wb, __bf16 *tile_a,
                                             __bf16 *tile_b, const float *__restrict__ fold, const EPILOGUE &last, float *__restrict__ dst,
                                             int lane)
{
    __bf16 *x = tile_a, *y = tile_b;
    int ldx = p.ld_a, ldy = p.ld_b;
    for (int l = 0; l < p.L; ++l) {
        if (l == p.L - 1) {
            mlp_bf16_dispatch(p, l, R, s_w, wb, x, ldx, fold, last, dst, lane);
        } else {
            mlp_bf16_dispatch(p, l, R, s_w, wb, x, ldx, fold, MlpToTileBf16{y, ldy}, dst, lane);
            wave_lds_sync();
            __bf16 *nx = y;
            y = x;
            x = nx;
            const int t = ldx;
            ldx = ldy;
            ldy = t;
        }
    }
}

}  // namespace ampnet
