// fused_mlp_bf16.hip -- host side of the bf16 fused MLP (fused_mlp_bf16.h): the plan, the weight conversion kernel and its launch.
#include "fused_mlp_bf16.h"

namespace ampnet {

// wb[wb_off_l + o kp_l + k] = bf16(W_l[o][k]), round to nearest even; zeros for cin_l <= k < kp_l.  One grid-stride walk per layer.
__global__ void mlp_bf16_weights_kernel(MlpPlanBf16 p, __bf16 *__restrict__ wb)
{
    for (int l = 0; l < p.L; ++l) {
        const int kp = p.kp[l], cin = p.cin[l], total = p.cout[l] * kp;
        const float *__restrict__ src = p.w[l];
        __bf16 *dst = wb + p.wb_off[l];
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
            const int o = e / kp, k = e - o * kp;
            dst[e] = (__bf16)(k < cin ? src[(size_t)o * cin + k] : 0.0f);
        }
    }
}

int mlp_bf16_weights_launch(const MlpPlanBf16 &p, __bf16 *wb, hipStream_t st)
{
    int most = 0;
    for (int l = 0; l < p.L; ++l) most = p.cout[l] * p.kp[l] > most ? p.cout[l] * p.kp[l] : most;
    hipLaunchKernelGGL(mlp_bf16_weights_kernel, dim3(cdiv(most, 256)), dim3(256), 0, st, p, wb);
    return check_launch("mlp_bf16_weights_kernel");
}

static int kp16(int cin) { return (cin + 15) / 16 * 16; }

size_t mlp_bf16_weight_bytes(const char *what, int cin0, const int *cout_host, int L)
{
    size_t elems = 0;
    for (int l = 0, cin = cin0; l < L; ++l) {
        const int cout = cout_host[l];
        MLP_BF16_REQUIRE(cout >= 32 && cout <= MLP_MAX_COUT && cout % 32 == 0, "%s: layer %d has cout=%d, must be a multiple of 32 in [32, %d]",
                         what, l, cout, MLP_MAX_COUT);
        elems += (size_t)cout * kp16(cin);
        cin = cout;
    }
    return elems * sizeof(__bf16);
}

int mlp_bf16_plan_build(const char *what, int cin0, int rows_per_wave, const float *const *params_host, const int *cout_host,
                        const float *eps_host, int L, MlpPlan &p32, MlpFold &f, MlpPlanBf16 &p)
{
    if (!mlp_plan_build(what, cin0, rows_per_wave, params_host, cout_host, eps_host, L, p32, f)) return 0;
    p = {};
    p.L = L;
    p.R = rows_per_wave;
    int wb_off = 0;
    for (int l = 0; l < L; ++l) {
        p.cin[l] = p32.cin[l];
        p.cout[l] = p32.cout[l];
        p.kp[l] = kp16(p.cin[l]);
        p.w[l] = p32.w[l];
        p.fold_off[l] = p32.fold_off[l];
        p.wb_off[l] = wb_off;
        wb_off += p.cout[l] * p.kp[l];
    }
    // tile A holds layer 0's input and layer 1's output, tile B layer 0's output
    p.ld_a = (L == 3 ? (p.kp[0] > p.cout[1] ? p.kp[0] : p.cout[1]) : p.kp[0]) + MLP_BF16_PAD;
    p.ld_b = (L >= 2 ? p.cout[0] : 0) + MLP_BF16_PAD;
    const size_t tile_bytes = (size_t)p.R * (p.ld_a + p.ld_b) * sizeof(__bf16);
    MLP_BF16_REQUIRE(tile_bytes <= (size_t)MLP_LDS_BYTES, "%s: a wave's tiles (%zu bytes) exceed the LDS", what, tile_bytes);
    p.nw = 4;
    while (p.nw > 1 && p.nw * tile_bytes > (size_t)MLP_LDS_BYTES) p.nw /= 2;
    size_t lds = p.nw * tile_bytes;
    // the weights that fit beside the tiles, in layer order
    int w_elems = 0;
    for (int l = 0; l < L; ++l) {
        const int elems = p.cout[l] * (p.kp[l] + MLP_BF16_PAD);
        p.w_off[l] = lds + elems * sizeof(__bf16) <= (size_t)MLP_LDS_BYTES ? w_elems : -1;
        if (p.w_off[l] < 0) continue;
        w_elems += elems;
        lds += elems * sizeof(__bf16);
    }
    return (int)lds;
}

}  // namespace ampnet
