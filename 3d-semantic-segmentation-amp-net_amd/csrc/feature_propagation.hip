// feature_propagation.hip -- one PointNet++ feature-propagation layer in eval mode, fused (C ABI: ampnet_fp_forward_f32).
//
// The input row of fine point i of cloud c is  [points1[i] (D1 values, or none), sum_k w_k points2[idx_k] (D2 values)],  the column order of
// the usual cat([points1, interpolated]); w_k = r_k / sum_k r_k, r_k = 1 / (dist2_k + 1e-8f), over the k <= 3 neighbours
// ampnet_three_nn_f32 found (k = 1: weight 1, the usual implementation's "repeat" branch).  Every layer computes relu(bn_eval(W row + b))
// and the last layer's activations are the output: there is no reduction over rows.  Nothing interpolated, concatenated or intermediate
// reaches HBM: a WAVE owns 32 consecutive fine points of one cloud, builds their rows straight into its own LDS tile and keeps them there
// through all layers.
//
//   * The 32 points are the M tile of v_mfma_f32_32x32x2_f32 (exact fp32: the matrix-precision scope is not consulted).  A tile never
//     spans two clouds; the rows past n of a cloud's last tile are zero-filled in LDS (nothing is read for them) and never stored.
//   * Lane map: that of set_abstraction.hip -- lane (r = l & 31, h = l >> 5) supplies row r of A and row n0 + r of W, the accumulator holds
//     column n0 + r of rows (i & 3) + 8 (i >> 2) + 4 h -- except for the ORDER of the contraction inside a block of 8: k-step i < 4 takes
//     k = k0 + 4 h + i (there: k0 + 2 i + h), so a lane's four weights are 16 contiguous bytes.  Weights that are not staged are then
//     read through L2 with one global_load_dwordx4 per lane and block (cin a multiple of 8: every shape of pointnet_2), a quarter of
//     the cache lines per MFMA that four strided dwords touch.
//   * LDS rows have an ODD stride in floats: ds_read_b32 / ds_write_b32 conflict inside a 32-lane half on (address / 4) % 32; the operand
//     reads walk r at a fixed k (32 rows, odd stride -> 32 banks), the epilogue's stores walk the column at a fixed row, the row
//     builder's stores walk the column too.
//   * Two tiles per wave ping-pong as in set_abstraction.hip; the last layer stores its relu'd accumulators straight to `out` (for a
//     fixed register the 32 lanes of a half write 128 contiguous bytes of one output row).
//   * A 384-wide input tile plus a 256-wide output tile (fp3 of pointnet_2) is 82 KB per wave and 320 + 256 (fp2) 74 KB: the plan halves
//     the waves per workgroup until the tiles fit the 160 KB LDS -- ONE wave per workgroup for fp3 (B * 256 rows in all: the layer is
//     small), two for fp2, four for fp1.  Layer 0's input is NOT built in K chunks.
//   * No reduction ties a wave to a group, so the waves of a workgroup (up to 128 rows) share the weights staged in LDS (rows padded to
//     the odd stride, once per workgroup, in layer order) while they fit next to the tiles; the rest is read through L2.
//   * BatchNorm is folded once per call by sa_fold_kernel (sa_fold.h), applied as fma(acc, scale, shift).
#include "sa_fold.h"

namespace ampnet {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FP_MAX_LAYERS = AMPNET_FP_MAX_LAYERS;
constexpr int FP_LDS_BYTES = 160 * 1024;
static_assert(AMPNET_FP_MAX_LAYERS == AMPNET_SA_MAX_LAYERS && AMPNET_FP_MAX_COUT == AMPNET_SA_MAX_COUT, "the fold kernel is shared");

struct FpPlan {
    int L, nw;                            // layers, waves per workgroup
    int cin[FP_MAX_LAYERS], cout[FP_MAX_LAYERS];
    int kp[FP_MAX_LAYERS];                // contraction length padded to a multiple of 8 (zeros)
    int ld_a, ld_b;                       // odd row strides of the two tiles, floats
    int w_off[FP_MAX_LAYERS];             // float offset of the layer's staged weights in LDS, -1 = read through L2
    int w_vec[FP_MAX_LAYERS];             // unstaged weights: rows are 16-byte aligned and cin % 8 == 0 -> dwordx4 loads
    int fold_off[FP_MAX_LAYERS];          // float offset of the layer's scale[cout], shift[cout] in the workspace
    const float *w[FP_MAX_LAYERS];
};

// NT column tiles of one layer over the wave's 32 rows.  x: the input tile [32][ldx]; w: weights [cout][ldw] (LDS or global), k_valid =
// columns of w that exist (the rest of kp counts as zero); VEC: w is global, 16-byte aligned rows, k_valid == kp.  LAST: store rows
// < rows to `dst` (global, row stride ldo); otherwise store the activations to the wave's other tile y [32][ldy].
template <int NT, bool LAST, bool VEC>
__device__ __forceinline__ void fp_tiles(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int n0,
                                         const float *__restrict__ scale, const float *__restrict__ shift, float *y, int ldy,
                                         float *__restrict__ dst, int ldo, int rows, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    float sc[NT], sh[NT];
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sc[t] = scale[n0 + 32 * t + r];
        sh[t] = shift[n0 + 32 * t + r];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    }
    const float *xr = x + r * ldx + 4 * h;
    for (int k0 = 0; k0 < kp; k0 += 8) {
        float av[4], bv[NT][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = xr[k0 + i];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float *wr = w + (size_t)(n0 + 32 * t + r) * ldw + k0 + 4 * h;
            if (VEC) {
                const float4 q = *reinterpret_cast<const float4 *>(wr);
                bv[t][0] = q.x;
                bv[t][1] = q.y;
                bv[t][2] = q.z;
                bv[t][3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) bv[t][i] = k0 + 4 * h + i < k_valid ? wr[i] : 0.0f;
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
        for (int i = 0; i < 16; ++i) {
            const float v = fmaxf(fmaf(acc[t][i], sc[t], sh[t]), 0.0f);
            const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
            if (LAST) {
                if (row < rows) dst[(size_t)row * ldo + n0 + 32 * t + r] = v;
            } else {
                y[row * ldy + n0 + 32 * t + r] = v;
            }
        }
}

template <bool LAST, bool VEC>
__device__ __forceinline__ void fp_layer(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int cout,
                                         const float *__restrict__ scale, const float *__restrict__ shift, float *y, int ldy,
                                         float *__restrict__ dst, int rows, int lane)
{
    int n0 = 0;
    for (; n0 + 128 <= cout; n0 += 128) fp_tiles<4, LAST, VEC>(x, ldx, w, ldw, k_valid, kp, n0, scale, shift, y, ldy, dst, cout, rows, lane);
    if (n0 + 64 <= cout) {
        fp_tiles<2, LAST, VEC>(x, ldx, w, ldw, k_valid, kp, n0, scale, shift, y, ldy, dst, cout, rows, lane);
        n0 += 64;
    }
    if (n0 + 32 <= cout) fp_tiles<1, LAST, VEC>(x, ldx, w, ldw, k_valid, kp, n0, scale, shift, y, ldy, dst, cout, rows, lane);
}

template <bool LAST>
__device__ __forceinline__ void fp_dispatch(const FpPlan &p, int l, const float *s_w, const float *x, int ldx, const float *__restrict__ fold,
                                            float *y, int ldy, float *__restrict__ dst, int rows, int lane)
{
    const float *scale = fold + p.fold_off[l], *shift = scale + p.cout[l];
    if (p.w_off[l] >= 0)
        fp_layer<LAST, false>(x, ldx, s_w + p.w_off[l], p.kp[l] + 1, p.kp[l], p.kp[l], p.cout[l], scale, shift, y, ldy, dst, rows, lane);
    else if (p.w_vec[l])
        fp_layer<LAST, true>(x, ldx, p.w[l], p.cin[l], p.cin[l], p.kp[l], p.cout[l], scale, shift, y, ldy, dst, rows, lane);
    else
        fp_layer<LAST, false>(x, ldx, p.w[l], p.cin[l], p.cin[l], p.kp[l], p.cout[l], scale, shift, y, ldy, dst, rows, lane);
}

__global__ __launch_bounds__(256) void fp_forward_kernel(FpPlan p, const float *__restrict__ points1, int D1, const float *__restrict__ points2,
                                                        int D2, int n, int s, const int32_t *__restrict__ idx, const float *__restrict__ dist2,
                                                        int k, const float *__restrict__ fold, int tiles_per_cloud, int n_tiles,
                                                        float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = 64 * p.nw;
    const int tile_floats = 32 * (p.ld_a + p.ld_b);
    float *tile_a = s_mem + wave * tile_floats, *tile_b = tile_a + 32 * p.ld_a;
    float *s_w = s_mem + p.nw * tile_floats;
    // stage the weights that fit: [cout][kp + 1], columns past cin zero
    for (int l = 0; l < p.L; ++l) {
        if (p.w_off[l] < 0) continue;
        const int ldw = p.kp[l] + 1, cin = p.cin[l], total = p.cout[l] * p.kp[l];
        const float *__restrict__ src = p.w[l];
        float *dstw = s_w + p.w_off[l];
        for (int e = tid; e < total; e += nthreads) {
            const int o = e / p.kp[l], c = e - o * p.kp[l];
            dstw[o * ldw + c] = c < cin ? src[(size_t)o * cin + c] : 0.0f;
        }
    }
    __syncthreads();
    const int cin0 = p.cin[0], kp0 = p.kp[0], cout_last = p.cout[p.L - 1];
    for (int tile = blockIdx.x * p.nw + wave; tile < n_tiles; tile += gridDim.x * p.nw) {
        const int cloud_i = tile / tiles_per_cloud, row0 = (tile - cloud_i * tiles_per_cloud) * 32;
        const int rows = min(32, n - row0);
        const float *p1 = points1 ? points1 + ((size_t)cloud_i * n + row0) * D1 : nullptr;
        const float *p2 = points2 + (size_t)cloud_i * s * D2;
        // lane t (and t + 32) holds the neighbours and weights of row t; indices are clamped into the coarse cloud
        int nb[3] = {0, 0, 0};
        float wk[3] = {0.0f, 0.0f, 0.0f};
        if ((lane & 31) < rows) {
            const size_t o = ((size_t)cloud_i * n + row0 + (lane & 31)) * k;
            float rk[3] = {0.0f, 0.0f, 0.0f};
            for (int q = 0; q < k; ++q) {
                nb[q] = min(max(idx[o + q], 0), s - 1);
                rk[q] = 1.0f / (dist2[o + q] + 1e-8f);
            }
            float sum = rk[0];
            if (k > 1) sum += rk[1];
            if (k > 2) sum += rk[2];
            for (int q = 0; q < k; ++q) wk[q] = rk[q] / sum;
        }
        // build the rows into tile A, the columns fastest across the lanes: a row's features load contiguously
#pragma unroll 2
        for (int t = 0; t < 32; ++t) {
            const int j0 = __shfl(nb[0], t), j1 = __shfl(nb[1], t), j2 = __shfl(nb[2], t);
            const float w0 = __shfl(wk[0], t), w1 = __shfl(wk[1], t), w2 = __shfl(wk[2], t);
            const float *f0 = p2 + (size_t)j0 * D2, *f1 = p2 + (size_t)j1 * D2, *f2 = p2 + (size_t)j2 * D2;
            for (int c = lane; c < kp0; c += 64) {
                float v = 0.0f;
                if (t < rows) {
                    if (c < D1) {
                        v = p1[(size_t)t * D1 + c];
                    } else if (c < cin0) {
                        v = w0 * f0[c - D1];
                        if (k > 1) v = fmaf(w1, f1[c - D1], v);
                        if (k > 2) v = fmaf(w2, f2[c - D1], v);
                    }
                }
                tile_a[t * p.ld_a + c] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float *dst = out + ((size_t)cloud_i * n + row0) * cout_last;
        const float *x = tile_a;
        float *y = tile_b;
        int ldx = p.ld_a, ldy = p.ld_b;
        for (int l = 0; l < p.L; ++l) {
            if (l == p.L - 1) {
                fp_dispatch<true>(p, l, s_w, x, ldx, fold, y, ldy, dst, rows, lane);
            } else {
                fp_dispatch<false>(p, l, s_w, x, ldx, fold, y, ldy, dst, rows, lane);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                float *nx = y;
                y = const_cast<float *>(x);
                x = nx;
                const int t = ldx;
                ldx = ldy;
                ldy = t;
            }
        }
        // the next tile's rows overwrite tile A: every read of this tile is done (the last layer's results went out from registers)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

static int fp_round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace ampnet

extern "C" int ampnet_fp_forward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                                     const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host,
                                     int L, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(points2 && idx && dist2 && params_host && cout_host && eps_host && out, "ampnet_fp_forward_f32: null pointer");
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && s >= 1, "ampnet_fp_forward_f32: bad shape n_clouds=%d n=%d s=%d", n_clouds, n, s);
    AMPNET_REQUIRE(k >= 1 && k <= 3 && k <= s, "ampnet_fp_forward_f32: k=%d must be 1, 2 or 3 and <= s=%d", k, s);
    AMPNET_REQUIRE(L >= 1 && L <= AMPNET_FP_MAX_LAYERS, "ampnet_fp_forward_f32: L=%d layers, the kernel is built for 1 .. %d", L, AMPNET_FP_MAX_LAYERS);
    AMPNET_REQUIRE(D1 >= 0 && (D1 == 0) == (points1 == nullptr), "ampnet_fp_forward_f32: points1 must be NULL exactly when D1 = 0 (D1=%d)", D1);
    AMPNET_REQUIRE(D2 >= 1 && D1 <= AMPNET_FP_MAX_CIN && D2 <= AMPNET_FP_MAX_CIN && D1 + D2 <= AMPNET_FP_MAX_CIN,
                   "ampnet_fp_forward_f32: cin_0 = D1 + D2 = %d + %d must be in [1, %d] with D2 >= 1", D1, D2, AMPNET_FP_MAX_CIN);
    AMPNET_REQUIRE(workspace && workspace_bytes >= AMPNET_FP_WORKSPACE_BYTES, "ampnet_fp_forward_f32: workspace of %zu bytes, need %d",
                   workspace_bytes, AMPNET_FP_WORKSPACE_BYTES);
    const int tiles_per_cloud = (int)(((long long)n + 31) / 32);
    // (the tile counter of a wave steps by at most 4096 past the last tile: keep that inside an int)
    AMPNET_REQUIRE((long long)n_clouds * tiles_per_cloud <= 0x7fff0000LL, "ampnet_fp_forward_f32: n_clouds * ceil(n / 32) = %lld tiles exceed %lld",
                   (long long)n_clouds * tiles_per_cloud, 0x7fff0000LL);
    FpPlan p = {};
    SaFold f = {};
    p.L = f.L = L;
    int fold_off = 0;
    for (int l = 0; l < L; ++l) {
        const int cout = cout_host[l];
        AMPNET_REQUIRE(cout >= 32 && cout <= AMPNET_FP_MAX_COUT && cout % 32 == 0,
                       "ampnet_fp_forward_f32: layer %d has cout=%d, must be a multiple of 32 in [32, %d]", l, cout, AMPNET_FP_MAX_COUT);
        for (int q = 0; q < 6; ++q) AMPNET_REQUIRE(params_host[6 * l + q], "ampnet_fp_forward_f32: null parameter %d of layer %d", q, l);
        p.cin[l] = l ? cout_host[l - 1] : D1 + D2;
        p.cout[l] = f.cout[l] = cout;
        p.kp[l] = fp_round_up(p.cin[l], 8);
        p.w[l] = params_host[6 * l];
        p.w_vec[l] = p.cin[l] % 8 == 0 && reinterpret_cast<uintptr_t>(p.w[l]) % 16 == 0;
        f.bias[l] = params_host[6 * l + 1];
        f.gamma[l] = params_host[6 * l + 2];
        f.beta[l] = params_host[6 * l + 3];
        f.mean[l] = params_host[6 * l + 4];
        f.var[l] = params_host[6 * l + 5];
        f.eps[l] = eps_host[l];
        p.fold_off[l] = f.off[l] = fold_off;
        fold_off += 2 * cout;
    }
    // tile A holds layer 0's input and layer 1's output, tile B layer 0's output
    p.ld_a = (L == 3 ? (p.kp[0] > p.cout[1] ? p.kp[0] : p.cout[1]) : p.kp[0]) + 1;
    p.ld_b = L >= 2 ? p.cout[0] + 1 : 1;
    const size_t tile_bytes = (size_t)32 * (p.ld_a + p.ld_b) * sizeof(float);
    AMPNET_REQUIRE(tile_bytes <= (size_t)FP_LDS_BYTES, "ampnet_fp_forward_f32: a wave's tiles (%zu bytes) exceed the LDS", tile_bytes);
    p.nw = 4;
    while (p.nw > 1 && p.nw * tile_bytes > (size_t)FP_LDS_BYTES) p.nw /= 2;
    size_t lds = p.nw * tile_bytes;
    int w_floats = 0;
    for (int l = 0; l < L; ++l) {
        const size_t need = (size_t)p.cout[l] * (p.kp[l] + 1) * sizeof(float);
        if (lds + need <= (size_t)FP_LDS_BYTES) {
            p.w_off[l] = w_floats;
            w_floats += p.cout[l] * (p.kp[l] + 1);
            lds += need;
        } else {
            p.w_off[l] = -1;
        }
    }
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fp_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, FP_LDS_BYTES);
        if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "ampnet_fp_forward_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    float *fold = static_cast<float *>(workspace);
    int rc = sa_fold_launch(f, fold, (hipStream_t)stream);
    if (rc != AMPNET_OK) return rc;
    const int n_tiles = n_clouds * tiles_per_cloud;
    // every workgroup stages the weights once: at most 4 workgroups per CU's worth of them, each wave walking several tiles
    const int grid = n_tiles / p.nw >= 1024 ? 1024 : cdiv(n_tiles, p.nw);
    hipLaunchKernelGGL(fp_forward_kernel, dim3(grid), dim3(64 * p.nw), lds, (hipStream_t)stream, p, points1, D1, points2, D2, n, s, idx, dist2, k,
                       fold, tiles_per_cloud, n_tiles, out);
    return check_launch("fp_forward_kernel");
}
