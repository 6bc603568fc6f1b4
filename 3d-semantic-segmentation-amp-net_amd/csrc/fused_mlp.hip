// fused_mlp.hip -- host side of the shared fused MLP (fused_mlp.h): the plan, the BatchNorm fold kernel, the launch helpers.
#include "fused_mlp.h"

namespace ampnet {

__global__ void sa_fold_kernel(MlpPlan p, MlpFold f, float *__restrict__ fold)
{
    for (int l = 0; l < p.L; ++l)
        for (int c = threadIdx.x; c < p.cout[l]; c += blockDim.x) {
            const float scale = f.gamma[l][c] / sqrtf(f.var[l][c] + f.eps[l]);
            fold[p.fold_off[l] + c] = scale;
            fold[p.fold_off[l] + p.cout[l] + c] = fmaf(f.bias[l][c] - f.mean[l][c], scale, f.beta[l][c]);
        }
}

int mlp_fold_launch(const MlpPlan &p, const MlpFold &f, float *fold, hipStream_t st)
{
    hipLaunchKernelGGL(sa_fold_kernel, dim3(1), dim3(256), 0, st, p, f, fold);
    return check_launch("sa_fold_kernel");
}

int mlp_allow_full_lds(const char *what, const void *kernel, bool &done)
{
    if (done) return AMPNET_OK;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_BYTES);
    if (e != hipSuccess) return fail(AMPNET_E_LAUNCH, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
    done = true;
    return AMPNET_OK;
}

#define MLP_REQUIRE(cond, ...)                    \
    do {                                          \
        if (!(cond)) {                            \
            fail(AMPNET_E_ARG, __VA_ARGS__);      \
            return 0;                             \
        }                                         \
    } while (0)

int mlp_plan_build(const char *what, int cin0, int rows_per_wave, const float *const *params_host, const int *cout_host, const float *eps_host,
                   int L, MlpPlan &p, MlpFold &f)
{
    p = {};
    f = {};
    p.L = L;
    p.R = rows_per_wave;
    int fold_off = 0;
    for (int l = 0; l < L; ++l) {
        const int cout = cout_host[l];
        MLP_REQUIRE(cout >= 32 && cout <= MLP_MAX_COUT && cout % 32 == 0, "%s: layer %d has cout=%d, must be a multiple of 32 in [32, %d]", what,
                    l, cout, MLP_MAX_COUT);
        for (int q = 0; q < 6; ++q) MLP_REQUIRE(params_host[6 * l + q], "%s: null parameter %d of layer %d", what, q, l);
        p.cin[l] = l ? cout_host[l - 1] : cin0;
        p.cout[l] = cout;
        p.kp[l] = (p.cin[l] + 7) / 8 * 8;
        p.w[l] = params_host[6 * l];
        p.w_vec[l] = p.cin[l] % 8 == 0 && reinterpret_cast<uintptr_t>(p.w[l]) % 16 == 0;
        f.bias[l] = params_host[6 * l + 1];
        f.gamma[l] = params_host[6 * l + 2];
        f.beta[l] = params_host[6 * l + 3];
        f.mean[l] = params_host[6 * l + 4];
        f.var[l] = params_host[6 * l + 5];
        f.eps[l] = eps_host[l];
        p.fold_off[l] = fold_off;
        fold_off += 2 * cout;
    }
    // tile A holds layer 0's input and layer 1's output, tile B layer 0's output
    p.ld_a = (L == 3 ? (p.kp[0] > p.cout[1] ? p.kp[0] : p.cout[1]) : p.kp[0]) + 1;
    p.ld_b = L >= 2 ? p.cout[0] + 1 : 1;
    const size_t tile_bytes = (size_t)p.R * (p.ld_a + p.ld_b) * sizeof(float);
    MLP_REQUIRE(tile_bytes <= (size_t)MLP_LDS_BYTES, "%s: a wave's tiles (%zu bytes) exceed the LDS", what, tile_bytes);
    p.nw = 4;
    while (p.nw > 1 && p.nw * tile_bytes > (size_t)MLP_LDS_BYTES) p.nw /= 2;
    size_t lds = p.nw * tile_bytes;
    // the weights that fit beside the tiles, in layer order
    int w_floats = 0;
    for (int l = 0; l < L; ++l) {
        const int floats = p.cout[l] * (p.kp[l] + 1);
        p.w_off[l] = lds + floats * sizeof(float) <= (size_t)MLP_LDS_BYTES ? w_floats : -1;
        if (p.w_off[l] < 0) continue;
        w_floats += floats;
        lds += floats * sizeof(float);
    }
    return (int)lds;
}

}  // namespace ampnet
