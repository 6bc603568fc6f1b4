// set_abstraction.hip -- one PointNet++ set-abstraction layer in eval mode, fused (C ABI: ampnet_sa_forward_f32).
//
// For centre i of cloud c the group is the nsample rows  [xyz[idx_t] - xyz[centre_i] (3), feats[idx_t] (D)]  of group_idx[c][i][:];
// every layer computes relu(bn_eval(W row + b)) and the output is the per-channel max over the rows.  Nothing grouped reaches HBM:
// a WAVE owns a centre, gathers its rows straight into its own LDS tile and keeps them there through all layers.
//
//   * The group is the M tile of v_mfma_f32_32x32x2_f32 (exact fp32: the matrix-precision scope is not consulted): nsample is padded
//     to R = 32 or 64 rows by repeating row 0, which cannot change the max.  Lane (r = l & 31, h = l >> 5) supplies A = X[r][2 s + h]
//     and B = W[n0 + r][2 s + h] in k-step s; the accumulator holds column n0 + r of rows (i & 3) + 8 (i >> 2) + 4 h, i < 16.
//   * LDS rows have an ODD stride in floats.  ds_read_b32 / ds_write_b32 conflict inside a 32-lane half on (address / 4) % 32: the
//     operand reads walk r at a fixed k (32 rows, odd stride -> 32 banks), the epilogue's stores walk the column at a fixed row.
//   * Two tiles per wave ping-pong: layer 0 reads A (the gathered rows) and writes B, layer 1 reads B and writes A, the last layer
//     writes nothing -- its relu'd accumulators are reduced over their 16 registers and the two lane halves (the row dimension) and
//     lanes h = 0 store the maxima.
//   * BatchNorm is folded once per call, ahead of the main kernel, into scale = gamma / sqrt(var + eps) and
//     shift = (b - mean) * scale + beta (sa_fold_kernel, declared in sa_fold.h; the parameters live in device memory), applied as fma(acc, scale, shift).
//   * A layer's weights are staged in LDS (rows padded to the odd stride, once per workgroup) while they fit next to the waves'
//     tiles, in layer order; the layers that do not fit are read through L2 by the same lane map.
#include "sa_fold.h"

namespace ampnet {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SA_LDS_BYTES = 160 * 1024;

struct SaPlan {
    int L, R, nw;                         // layers, rows of a wave's tile (32 / 64), waves per workgroup
    int cin[SA_MAX_LAYERS], cout[SA_MAX_LAYERS];
    int kp[SA_MAX_LAYERS];                // contraction length padded to a multiple of 8 (zeros)
    int ld_a, ld_b;                       // odd row strides of the two tiles, floats
    int w_off[SA_MAX_LAYERS];             // float offset of the layer's staged weights in LDS, -1 = read through L2
    int fold_off[SA_MAX_LAYERS];          // float offset of the layer's scale[cout], shift[cout] in the workspace
    const float *w[SA_MAX_LAYERS];
};

__global__ void sa_fold_kernel(SaFold f, float *__restrict__ fold)
{
    for (int l = 0; l < f.L; ++l)
        for (int c = threadIdx.x; c < f.cout[l]; c += blockDim.x) {
            const float scale = f.gamma[l][c] / sqrtf(f.var[l][c] + f.eps[l]);
            fold[f.off[l] + c] = scale;
            fold[f.off[l] + f.cout[l] + c] = fmaf(f.bias[l][c] - f.mean[l][c], scale, f.beta[l][c]);
        }
}

// NT column tiles of one layer over every row tile of the wave.  x: the wave's input tile [R][ldx]; w: weights [cout][ldw] (LDS or
// global), k_valid = columns of w that exist (the rest of kp counts as zero).  LAST: reduce over the rows and store the maxima to
// `dst` (global, this centre's output row); otherwise store the activations to the wave's other tile y [R][ldy].
template <int NT, bool LAST>
__device__ __forceinline__ void sa_tiles(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int R, int n0,
                                         const float *__restrict__ scale, const float *__restrict__ shift, float *y, int ldy,
                                         float *__restrict__ dst, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    float sc[NT], sh[NT], mx[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sc[t] = scale[n0 + 32 * t + r];
        sh[t] = shift[n0 + 32 * t + r];
        mx[t] = -INFINITY;
    }
    for (int m0 = 0; m0 < R; m0 += 32) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
        const float *xr = x + (m0 + r) * ldx + h;
        for (int k0 = 0; k0 < kp; k0 += 8) {
            float av[4], bv[NT][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + 2 * i + h;
                av[i] = xr[k0 + 2 * i];
#pragma unroll
                for (int t = 0; t < NT; ++t) bv[t][i] = k < k_valid ? w[(n0 + 32 * t + r) * ldw + k] : 0.0f;
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
                if (LAST) mx[t] = fmaxf(mx[t], v);
                else y[(m0 + (i & 3) + 8 * (i >> 2) + 4 * h) * ldy + n0 + 32 * t + r] = v;
            }
    }
    if (LAST) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float o = fmaxf(mx[t], __shfl_xor(mx[t], 32));
            if (h == 0) dst[n0 + 32 * t + r] = o;
        }
    }
}

template <bool LAST>
__device__ __forceinline__ void sa_layer(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int R, int cout,
                                         const float *__restrict__ scale, const float *__restrict__ shift, float *y, int ldy,
                                         float *__restrict__ dst, int lane)
{
    int n0 = 0;
    for (; n0 + 128 <= cout; n0 += 128) sa_tiles<4, LAST>(x, ldx, w, ldw, k_valid, kp, R, n0, scale, shift, y, ldy, dst, lane);
    if (n0 + 64 <= cout) {
        sa_tiles<2, LAST>(x, ldx, w, ldw, k_valid, kp, R, n0, scale, shift, y, ldy, dst, lane);
        n0 += 64;
    }
    if (n0 + 32 <= cout) sa_tiles<1, LAST>(x, ldx, w, ldw, k_valid, kp, R, n0, scale, shift, y, ldy, dst, lane);
}

__global__ __launch_bounds__(256) void sa_forward_kernel(SaPlan p, const float *__restrict__ xyz, int n, int ld, const int32_t *__restrict__ centres,
                                                        int s, const int32_t *__restrict__ group_idx, int nsample,
                                                        const float *__restrict__ feats, int D, const float *__restrict__ fold,
                                                        int n_groups, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = 64 * p.nw;
    const int tile_floats = p.R * (p.ld_a + p.ld_b);
    float *tile_a = s_mem + wave * tile_floats, *tile_b = tile_a + p.R * p.ld_a;
    float *s_w = s_mem + p.nw * tile_floats;
    // stage the weights that fit: [cout][kp + 1], columns past cin zero
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
    __syncthreads();
    const int cin0 = p.cin[0], kp0 = p.kp[0], cout_last = p.cout[p.L - 1];
    for (int g = blockIdx.x * p.nw + wave; g < n_groups; g += gridDim.x * p.nw) {
        const int cloud_i = g / s;
        const float *cloud = xyz + (size_t)cloud_i * n * ld;
        const float *fcloud = feats ? feats + (size_t)cloud_i * n * D : nullptr;
        const int cidx = min(max(centres[g], 0), n - 1);
        const float cx = cloud[(size_t)cidx * ld], cy = cloud[(size_t)cidx * ld + 1], cz = cloud[(size_t)cidx * ld + 2];
        // lane t holds the point of row t; rows past nsample repeat row 0
        const int my_idx = min(max(group_idx[(size_t)g * nsample + (lane < nsample ? lane : 0)], 0), n - 1);
        // gather the rows into tile A: element e = (row, column) with the columns fastest, so a row's features load contiguously
        for (int e = lane; e < p.R * kp0; e += 64) {
            const int t = e / kp0, c = e - t * kp0;
            const int j = __shfl(my_idx, t);
            float v = 0.0f;
            if (c < 3) v = cloud[(size_t)j * ld + c] - (c == 0 ? cx : c == 1 ? cy : cz);
            else if (c < cin0) v = fcloud[(size_t)j * D + (c - 3)];
            tile_a[t * p.ld_a + c] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float *dst = out + (size_t)g * cout_last;
        const float *x = tile_a;
        float *y = tile_b;
        int ldx = p.ld_a, ldy = p.ld_b;
        for (int l = 0; l < p.L; ++l) {
            const bool staged = p.w_off[l] >= 0;
            const float *scale = fold + p.fold_off[l], *shift = scale + p.cout[l];
            if (l == p.L - 1) {
                if (staged) sa_layer<true>(x, ldx, s_w + p.w_off[l], p.kp[l] + 1, p.kp[l], p.kp[l], p.R, p.cout[l], scale, shift, y, ldy, dst, lane);
                else sa_layer<true>(x, ldx, p.w[l], p.cin[l], p.cin[l], p.kp[l], p.R, p.cout[l], scale, shift, y, ldy, dst, lane);
            } else {
                if (staged) sa_layer<false>(x, ldx, s_w + p.w_off[l], p.kp[l] + 1, p.kp[l], p.kp[l], p.R, p.cout[l], scale, shift, y, ldy, dst, lane);
                else sa_layer<false>(x, ldx, p.w[l], p.cin[l], p.cin[l], p.kp[l], p.R, p.cout[l], scale, shift, y, ldy, dst, lane);
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
        // the next centre's gather overwrites tile A: every read of this centre is done (the last layer's results are in registers)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

int sa_fold_launch(const SaFold &f, float *fold, hipStream_t st)
{
    hipLaunchKernelGGL(sa_fold_kernel, dim3(1), dim3(256), 0, st, f, fold);
    return check_launch("sa_fold_kernel");
}

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace ampnet

extern "C" int ampnet_sa_forward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                                     int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                                     const float *eps_host, int L, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(xyz && centres && group_idx && params_host && cout_host && eps_host && out, "ampnet_sa_forward_f32: null pointer");
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1 && ld >= 3 && s >= 1, "ampnet_sa_forward_f32: bad shape n_clouds=%d n=%d ld=%d s=%d", n_clouds, n, ld, s);
    AMPNET_REQUIRE((long long)n_clouds * s <= 0x7fffffffLL, "ampnet_sa_forward_f32: n_clouds * s = %lld groups exceed 2^31 - 1", (long long)n_clouds * s);
    AMPNET_REQUIRE(nsample >= 1 && nsample <= AMPNET_SA_MAX_NSAMPLE, "ampnet_sa_forward_f32: nsample=%d must be in [1, %d]", nsample, AMPNET_SA_MAX_NSAMPLE);
    AMPNET_REQUIRE(L >= 1 && L <= AMPNET_SA_MAX_LAYERS, "ampnet_sa_forward_f32: L=%d layers, the kernel is built for 1 .. %d", L, AMPNET_SA_MAX_LAYERS);
    AMPNET_REQUIRE(D >= 0 && (D == 0) == (feats == nullptr), "ampnet_sa_forward_f32: feats must be NULL exactly when D = 0 (D=%d)", D);
    AMPNET_REQUIRE(3 + D <= AMPNET_SA_MAX_CIN, "ampnet_sa_forward_f32: cin_0 = 3 + D = %d exceeds %d", 3 + D, AMPNET_SA_MAX_CIN);
    AMPNET_REQUIRE(workspace && workspace_bytes >= AMPNET_SA_WORKSPACE_BYTES, "ampnet_sa_forward_f32: workspace of %zu bytes, need %d",
                   workspace_bytes, AMPNET_SA_WORKSPACE_BYTES);
    SaPlan p = {};
    SaFold f = {};
    p.L = f.L = L;
    p.R = nsample <= 32 ? 32 : 64;
    int fold_off = 0;
    for (int l = 0; l < L; ++l) {
        const int cout = cout_host[l];
        AMPNET_REQUIRE(cout >= 32 && cout <= AMPNET_SA_MAX_COUT && cout % 32 == 0,
                       "ampnet_sa_forward_f32: layer %d has cout=%d, must be a multiple of 32 in [32, %d]", l, cout, AMPNET_SA_MAX_COUT);
        for (int q = 0; q < 6; ++q) AMPNET_REQUIRE(params_host[6 * l + q], "ampnet_sa_forward_f32: null parameter %d of layer %d", q, l);
        p.cin[l] = l ? cout_host[l - 1] : 3 + D;
        p.cout[l] = f.cout[l] = cout;
        p.kp[l] = round_up(p.cin[l], 8);
        p.w[l] = params_host[6 * l];
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
    const size_t tile_bytes = (size_t)p.R * (p.ld_a + p.ld_b) * sizeof(float);
    AMPNET_REQUIRE(tile_bytes <= (size_t)SA_LDS_BYTES, "ampnet_sa_forward_f32: a group's tiles (%zu bytes) exceed the LDS", tile_bytes);
    p.nw = 4;
    while (p.nw > 1 && p.nw * tile_bytes > (size_t)SA_LDS_BYTES) p.nw /= 2;
    size_t lds = p.nw * tile_bytes;
    int w_floats = 0;
    for (int l = 0; l < L; ++l) {
        const size_t need = (size_t)p.cout[l] * (p.kp[l] + 1) * sizeof(float);
        if (lds + need <= (size_t)SA_LDS_BYTES) {
            p.w_off[l] = w_floats;
            w_floats += p.cout[l] * (p.kp[l] + 1);
            lds += need;
        } else {
            p.w_off[l] = -1;
        }
    }
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(sa_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SA_LDS_BYTES);
        if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "ampnet_sa_forward_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    float *fold = static_cast<float *>(workspace);
    int rc = sa_fold_launch(f, fold, (hipStream_t)stream);
    if (rc != AMPNET_OK) return rc;
    const int n_groups = n_clouds * s;
    // every workgroup stages the weights once: at most 4 workgroups per CU's worth of them, each wave walking several centres
    int grid = cdiv(n_groups, p.nw);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(sa_forward_kernel, dim3(grid), dim3(64 * p.nw), lds, (hipStream_t)stream, p, xyz, n, ld, centres, s, group_idx, nsample, feats,
                       D, fold, n_groups, out);
    return check_launch("sa_forward_kernel");
}
