// set_abstraction_train.hip -- one fused set-abstraction layer with TRAIN-mode BatchNorm: batch statistics over all M = n_clouds s nsample
// rows, running-statistics update, and the backward through the statistics (C ABI: ampnet_sa_train_forward_f32,
// ampnet_sa_train_backward_f32, their _workspace_bytes and the test hook ampnet_sa_train_backward_tape).  The arithmetic is stated in
// include/ampnet_hip.h.  Everything runs on the caller's stream, no float atomics, every summation order a function of the shape alone;
// exact fp32 MFMA whatever the matrix precision is.  The slots that ball query filled by repeating its first member are rows like any
// other; the tile-padding rows t >= nsample enter nothing.
//
// FORWARD: L statistics passes, then the eval forward's kernel, unchanged.
//   sat_stats_kernel (pass l)   The forward's workgroup (its plan: up to four waves that share the staged weights of layers < l); a wave owns
//       a group at a time.  It gathers the group's R rows as the forward does, runs layers < l with the forward's own code
//       (mlp_dispatch<K_PAIRS>, reading the scale and shift that the earlier passes' finalizes wrote), forms layer l's raw accumulators
//       a = W x in the forward's contraction order (mlp_accumulate) and, per column and 32-row tile, the count, mean and sum (a - mean)^2
//       over the rows t < nsample.  The groups r, r + P, .. (P = min(groups, 1024)) are merged in ascending order, a group's tiles
//       ascending, into row r of a partials array with Chan's formula; a row belongs to one wave, so every word of it is read and written
//       by the same lane only, and the order does not depend on the plan.
//   fpt_stats_finalize_kernel   (bn_train.hip) merges the rows and writes the fold, save_mean, save_invstd and the
//       running-statistics update.
//   sa_forward_kernel           the eval forward's kernel on that fold (sa_forward_launch): eval and train share the hot kernel, and `out`
//       is the max of what the statistics were taken from, bit for bit.
//   The passes recompute layers < l instead of spilling them, as the feature-propagation train forward does: the forward keeps no
//   activation in memory and its workspace is the fold plus the partial rows.
//
// BACKWARD: L + 1 phases in descending layer order, a finalize between them, then the eval backward's dW and gather.
//   sat_bwd_last_kernel (phase L-1), one wave per workgroup, a group at a time, two LDS tiles T0 and T1 of 32 rows:
//       per 32-row tile of the group it gathers the rows, runs layers < L-1 forward and stores every layer input x_j of the rows
//       t < nsample to the workspace (dW reads them, and so do the later phases: the rows are never built again).  Then x_{L-1} of the
//       group's one or two tiles comes back into T0 and T1, a_{L-1} is formed, and per column the largest relu(y), the row that attains
//       it and that row's a are kept (SaArgMax, sa_tiles.h; only the rows t < nsample are offered: the padding rows are zeros here, not
//       copies of row 0, and must not compete).  dy of the last layer has one nonzero per (group, column):
//       it stays as arg (workspace, and arg_out) plus dout, never as a dense array; the one term per group enters sum dy and sum dy a.
//   sat_bwd_phase_kernel (phase l = L-2 .. -1), one wave per workgroup, a 32-row tile (g, m) at a time:
//       part A for layer j = l+1: x_j from the workspace into T0, a_j recomputed, dy_j from the workspace (j = L-1: dout at the row arg
//       names when its y > 0), dz_j = scale fma(-(a - mu), dgamma invstd / M, dy - dbeta / M) for EVERY row t < nsample (zero for the padding
//       rows) into T1 and the workspace;  dx_l = dz_j W_j (mlp_dgrad) over T0;  l = -1 ends here, dx_0's feature columns going to the
//       gather's rows (skipped when nobody wants dfeats).
//       part B for layer l:  x_l from the workspace into T1, a_l recomputed, dy_l = dx_l [fma(a, scale, shift) > 0] stored to the workspace,
//       sum dy and sum dy a added into the workgroup's own partial row.
//   fpt_bwd_finalize_kernel     (bn_train.hip) after every phase l >= 0.
//   fpb_wgrad_launch, sa_gather_launch   dW_l = dz_l^T x_l and dfeats, exactly the eval backward's (the gather ragged when the clouds are), on
//       the eval backward's workspace layout.
//   A phase holds two 32-row tiles of the widest layer input (at most 82 KB) whatever nsample is.
//   The statistics, part A and part B of a tile are bn_train.h's (bnt_tile_stats, bnt_form_dz, bnt_form_dy), shared with feature propagation;
//   this file keeps what is set abstraction's own: the gathers, the tiling, the max of the last layer (sat_last).
#include "bn_train.h"
#include "sa_tiles.h"

namespace ampnet {

constexpr long long SAT_MAX_ROWS = AMPNET_SA_TRAIN_MAX_ROWS;    // the merges carry row counts as floats: exact up to here, larger M is refused
constexpr int SAT_MAX_PARTS = 1024;                            // partial rows of the statistics passes

// the statistics of NT column tiles of layer l from n0 over the rows t < nsample of the wave's group, a 32-row tile at a time
template <int NT>
__device__ __forceinline__ void sat_group_stats(const float *x, int ldx, const float *__restrict__ w, int cin, int kp, int n0, int R, int nsample,
                                                float *part_n, float *part_mean, float *part_m2, int lane)
{
    for (int m0 = 0; m0 < R; m0 += 32)            // (rows >= 1: R = 64 only when nsample > 32)
        bnt_tile_stats<NT, K_PAIRS, false>(x, ldx, m0, w, cin, kp, n0, min(32, nsample - m0), part_n, part_mean, part_m2, lane);
}

// parts [n_parts][3 cout_l]: per partial row the count, mean and sum of squared deviations of every channel of layer l.  Row r takes the
// groups r, r + n_parts, .. in ascending order and belongs to ONE wave, whatever the plan's waves per workgroup are.
__global__ __launch_bounds__(256) void sat_stats_kernel(MlpPlan p, int l, const float *__restrict__ xyz, int n, int ld,
                                                       const int32_t *__restrict__ centres, int s, const int32_t *__restrict__ group_idx,
                                                       int nsample, const float *__restrict__ feats, int D, const float *__restrict__ fold,
                                                       int n_groups, int n_parts, float *__restrict__ parts)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MlpLds m = mlp_lds(p, p.R, s_mem, wave);
    mlp_stage_weights(p, m.s_w, tid, 64 * p.nw);                  // (the layers < l: the host took the others out of the staging)
    __syncthreads();
    const int cin0 = p.cin[0], kp0 = p.kp[0], cin = p.cin[l], cout = p.cout[l], kp = p.kp[l];
    float *tile[2] = {m.tile_a, m.tile_b};
    const int ldt[2] = {p.ld_a, p.ld_b};
    for (int row = blockIdx.x * p.nw + wave; row < n_parts; row += gridDim.x * p.nw) {
        float *part_n = parts + (size_t)row * 3 * cout, *part_mean = part_n + cout, *part_m2 = part_mean + cout;
        if (lane < 32)
            for (int c = lane; c < cout; c += 32) part_n[c] = part_mean[c] = part_m2[c] = 0.0f;  // channel c belongs to lane c % 32
        for (int g = row; g < n_groups; g += n_parts) {
            sa_gather_group(m.tile_a, p.ld_a, p.R, kp0, cin0, xyz, n, ld, centres, s, group_idx, nsample, feats, D, g, lane);
            // (the rows past nsample repeat row 0 and enter no statistic)
            wave_lds_sync();
            for (int j = 0; j < l; ++j) {
                mlp_dispatch<K_PAIRS>(p, j, p.R, m.s_w, tile[j & 1], ldt[j & 1], fold, MlpToTile{tile[(j + 1) & 1], ldt[(j + 1) & 1]}, nullptr, lane);
                wave_lds_sync();
            }
            const float *x = tile[l & 1];
            const int ldx = ldt[l & 1];
            int n0 = 0;
            for (; n0 + 128 <= cout; n0 += 128) sat_group_stats<4>(x, ldx, p.w[l], cin, kp, n0, p.R, nsample, part_n, part_mean, part_m2, lane);
            for (; n0 < cout; n0 += 32) sat_group_stats<1>(x, ldx, p.w[l], cin, kp, n0, p.R, nsample, part_n, part_mean, part_m2, lane);
            wave_lds_sync();                      // the next group's gather overwrites tile A
        }
    }
}

// The last layer of one group: x_{L-1} of its row tiles in T0 (rows 0 .. 31) and T1 (32 .. 63).  Per column the SaArgMax over the rows
// t < nsample; the group's one term of sum dy and sum dy a; arg to the workspace and to arg_out.
template <int NT>
__device__ __forceinline__ void sat_last(const float *t0, const float *t1, int ldx, const float *__restrict__ w, int cin, int kp, int n0,
                                         const float *__restrict__ scale, const float *__restrict__ shift, int R, int nsample,
                                         const float *__restrict__ dout_g, float *part_b, float *part_g, int32_t *__restrict__ arg_ws,
                                         int32_t *__restrict__ arg_g, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    float sc[NT], sh[NT];
    SaArgMax am[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sc[t] = scale[n0 + 32 * t + r];
        sh[t] = shift[n0 + 32 * t + r];
        am[t].init();
    }
    for (int m0 = 0; m0 < R; m0 += 32) {
        const float *x = m0 ? t1 : t0;
        f32x16 acc[NT];
        mlp_accumulate<NT, K_PAIRS, false>(acc, mlp_operand<K_PAIRS>(x, ldx, r, h), w, cin, cin, kp, n0, r, h);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;   // ascending in (m0, i), as SaArgMax asks; spelled out: see sab_last
                const float a = acc[t][i], y = fmaxf(fmaf(a, sc[t], sh[t]), 0.0f);
                if (row < nsample) am[t].put(a, y, row);   // (only the rows t < nsample compete)
            }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        am[t].merge_halves();
        if (h == 0) {                             // (this lane alone ever touches these words of the workgroup's partials)
            const float dy = am[t].best > 0.0f ? dout_g[col] : 0.0f;
            part_b[col] += dy;
            part_g[col] += dy * am[t].a;
            arg_ws[col] = am[t].row;
            if (arg_g) arg_g[col] = am[t].row;
        }
    }
}

__global__ __launch_bounds__(64) void sat_bwd_last_kernel(MlpPlan p, BntBwd b, const float *__restrict__ xyz, int n, int ldc,
                                                         const int32_t *__restrict__ centres, int s, const int32_t *__restrict__ group_idx,
                                                         int nsample, const float *__restrict__ feats, int D, const float *__restrict__ fold,
                                                         const float *__restrict__ dout, int n_groups, int32_t *__restrict__ arg_out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x;
    const int L = p.L, R = p.R, ld = b.ld, l = L - 1;
    const int cin0 = p.cin[0], kp0 = p.kp[0], cout = p.cout[l];
    float *T[2] = {s_mem, s_mem + 32 * ld};
    float *part_b = b.parts + (size_t)blockIdx.x * 2 * cout, *part_g = part_b + cout;
    if (lane < 32)
        for (int c = lane; c < cout; c += 32) part_b[c] = part_g[c] = 0.0f;          // channel c belongs to lane c % 32
    const float *scale = fold + p.fold_off[l], *shift = scale + cout;
    for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int cloud_i = g / s;
        const float *cloud = xyz + (size_t)cloud_i * n * ldc;
        const float *fcloud = feats ? feats + (size_t)cloud_i * n * D : nullptr;
        const int cidx = min(max(centres[g], 0), n - 1);
        const float cx = cloud[(size_t)cidx * ldc], cy = cloud[(size_t)cidx * ldc + 1], cz = cloud[(size_t)cidx * ldc + 2];
        const size_t grow = (size_t)g * nsample;
        for (int m0 = 0; m0 < R; m0 += 32) {
            const int rows = min(32, nsample - m0);
            sat_gather_rows(T[0], ld, kp0, cin0, cloud, ldc, fcloud, D, n, group_idx + grow, cx, cy, cz, m0, rows, lane);
            wave_lds_sync();
            fpb_store_rows(T[0], ld, kp0, b.xs[0] + (grow + m0) * b.ldxs[0], b.ldxs[0], rows, lane);
            for (int j = 0; j + 1 < L; ++j) {
                float *y = T[(j + 1) & 1];
                mlp_dispatch<K_PAIRS>(p, j, 32, s_mem, T[j & 1], ld, fold, MlpToTile{y, ld}, nullptr, lane);
                wave_lds_sync();
                fpb_store_rows(y, ld, p.cout[j], b.xs[j + 1] + (grow + m0) * b.ldxs[j + 1], b.ldxs[j + 1], rows, lane);
            }
            wave_lds_sync();                      // the next tile's gather overwrites T0
        }
        for (int m0 = 0; m0 < R; m0 += 32)
            fpb_load_rows(T[m0 >> 5], ld, p.kp[l], b.xs[l] + (grow + m0) * b.ldxs[l], b.ldxs[l], min(32, nsample - m0), lane);
        wave_lds_sync();
        const float *dout_g = dout + (size_t)g * cout;
        int32_t *arg_ws = b.arg + (size_t)g * cout, *arg_g = arg_out ? arg_out + (size_t)g * cout : nullptr;
        int n0 = 0;
        for (; n0 + 128 <= cout; n0 += 128)
            sat_last<4>(T[0], T[1], ld, p.w[l], p.cin[l], p.kp[l], n0, scale, shift, R, nsample, dout_g, part_b, part_g, arg_ws, arg_g, lane);
        for (; n0 < cout; n0 += 32)
            sat_last<1>(T[0], T[1], ld, p.w[l], p.cin[l], p.kp[l], n0, scale, shift, R, nsample, dout_g, part_b, part_g, arg_ws, arg_g, lane);
        wave_lds_sync();                          // the next group overwrites both tiles
    }
}

// Two column tiles per step, not four, and two waves per SIMD asked of the compiler (256 registers, two of them spilled): the phases wait on
// the workspace, not on the MFMAs, and at sa1's shape a second wave per SIMD takes the backward from 3.18 ms to 2.12 ms.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void sat_bwd_phase_kernel(MlpPlan p, BntBwd b, int l, int nsample, int D, const float *__restrict__ fold,
                                                          const float *__restrict__ dout, int n_tiles, int want_dx0)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x;
    const int L = p.L, ld = b.ld, tpg = p.R >> 5;
    float *T[2] = {s_mem, s_mem + 32 * ld};
    float *part_b = nullptr, *part_g = nullptr;
    if (l >= 0) {
        part_b = b.parts + (size_t)blockIdx.x * 2 * p.cout[l];
        part_g = part_b + p.cout[l];
        if (lane < 32)
            for (int c = lane; c < p.cout[l]; c += 32) part_b[c] = part_g[c] = 0.0f;             // channel c belongs to lane c % 32
    }
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int g = tile / tpg, m0 = (tile - g * tpg) * 32;
        const int rows = min(32, nsample - m0);
        const size_t grow = (size_t)g * nsample + m0;
        {
            const int j = l + 1, cin = p.cin[j], cout = p.cout[j], kp = p.kp[j];
            fpb_load_rows_flat(T[0], ld, kp, b.xs[j] + grow * b.ldxs[j], b.ldxs[j], rows, lane);
            wave_lds_sync();
            const float *scale = fold + p.fold_off[j], *shift = scale + cout, *c1 = b.coef + p.fold_off[j], *c2 = c1 + cout;
            const int32_t *arg_g = j == L - 1 ? b.arg + (size_t)g * cout : nullptr;
            const float *dout_g = j == L - 1 ? dout + (size_t)g * cout : nullptr;
            float *dz_ws = b.dz[j] + grow * cout;
            int n0 = 0;
            for (; n0 + 64 <= cout; n0 += 64)
                bnt_form_dz<2, K_PAIRS, false>(T[0], ld, p.w[j], cin, kp, cout, n0, scale, shift, b.mean[j], c1, c2, T[1], ld, rows, m0, arg_g, dout_g, dz_ws, lane);
            for (; n0 < cout; n0 += 32)
                bnt_form_dz<1, K_PAIRS, false>(T[0], ld, p.w[j], cin, kp, cout, n0, scale, shift, b.mean[j], c1, c2, T[1], ld, rows, m0, arg_g, dout_g, dz_ws, lane);
            wave_lds_sync();
            if (j == 0 && !want_dx0) continue;    // (wave-uniform) nobody asked for dfeats: dx_0 is not needed
            // dx_l = dz_j W_j over T0 (x_j has been used), or its feature columns to the gather's rows
            float *xo = j ? T[0] : nullptr;
            float *dx0 = b.dx0 + grow * D;
            int c0 = 0;
            for (; c0 + 64 <= cin; c0 += 64) mlp_dgrad<2, true>(T[1], ld, p.w[j], cin, cout, c0, xo, ld, nullptr, 3, dx0, D, rows, lane);
            for (; c0 < cin; c0 += 32) mlp_dgrad<1, true>(T[1], ld, p.w[j], cin, cout, c0, xo, ld, nullptr, 3, dx0, D, rows, lane);
            wave_lds_sync();
        }
        if (l >= 0) {
            const int cin = p.cin[l], cout = p.cout[l], kp = p.kp[l];
            fpb_load_rows_flat(T[1], ld, kp, b.xs[l] + grow * b.ldxs[l], b.ldxs[l], rows, lane);
            wave_lds_sync();
            const float *scale = fold + p.fold_off[l], *shift = scale + cout;
            float *dz_ws = b.dz[l] + grow * cout;
            int n0 = 0;
            for (; n0 + 64 <= cout; n0 += 64)
                bnt_form_dy<2, K_PAIRS, false, false>(T[1], ld, p.w[l], cin, kp, cout, n0, scale, shift, T[0], ld, nullptr, rows, dz_ws, part_b, part_g, lane);
            for (; n0 < cout; n0 += 32)
                bnt_form_dy<1, K_PAIRS, false, false>(T[1], ld, p.w[l], cin, kp, cout, n0, scale, shift, T[0], ld, nullptr, rows, dz_ws, part_b, part_g, lane);
        }
        wave_lds_sync();                          // the next tile overwrites both tiles
    }
}

// what the forward's two entry points derive from the shape (the limits are the backward's: what trains has a backward)
struct SatFwdShape {
    long long M;
    int R, n_groups, n_parts;
    size_t off_parts, floats;
};

static int sat_fwd_shape(const char *what, int D, int n_clouds, int s, int nsample, const int *cout_host, int L, SatFwdShape &sh)
{
    SaBwdShape b;
    AMPNET_TRY(sab_shape(what, D, n_clouds, s, nsample, cout_host, L, b));
    AMPNET_TRY(bnt_rows_ok(what, b.M, SAT_MAX_ROWS, "n_clouds * s * nsample"));
    sh = {};
    sh.M = b.M;
    sh.R = b.R;
    sh.n_groups = b.n_groups;
    sh.n_parts = b.n_groups < SAT_MAX_PARTS ? b.n_groups : SAT_MAX_PARTS;
    int widest = 0;
    for (int l = 0; l < L; ++l) widest = cout_host[l] > widest ? cout_host[l] : widest;
    sh.off_parts = align_up((size_t)AMPNET_SA_WORKSPACE_BYTES / sizeof(float), 64);
    sh.floats = sh.off_parts + align_up((size_t)sh.n_parts * 3 * widest, 64);
    return AMPNET_OK;
}

// the backward's layout: the eval backward's, then two coefficients per channel and the max's rows
static int sat_bwd_shape(const char *what, int D, int n_clouds, int s, int nsample, const int *cout_host, int L, SaBwdShape &sh, size_t &off_coef,
                         size_t &off_arg, size_t &floats)
{
    AMPNET_TRY(sab_shape(what, D, n_clouds, s, nsample, cout_host, L, sh));
    AMPNET_TRY(bnt_rows_ok(what, sh.M, SAT_MAX_ROWS, "n_clouds * s * nsample"));
    off_coef = sh.floats;
    off_arg = off_coef + align_up((size_t)2 * sh.sum_c, 64);
    floats = off_arg + align_up((size_t)sh.n_groups * cout_host[L - 1], 64);
    return AMPNET_OK;
}

}  // namespace ampnet

extern "C" size_t ampnet_sa_train_forward_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L)
{
    using namespace ampnet;
    SatFwdShape sh;
    if (sat_fwd_shape("ampnet_sa_train_forward_workspace_bytes", D, n_clouds, s, nsample, cout_host, L, sh) != AMPNET_OK) return 0;
    return sh.floats * sizeof(float);
}

extern "C" int ampnet_sa_train_forward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                                           int nsample, const float *feats, int D, float *const *params_host, const int *cout_host,
                                           const float *eps_host, int L, float momentum, float *out, float *save_mean, float *save_invstd,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_sa_train_forward_f32";
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(xyz && centres && group_idx && params_host && cout_host && eps_host && out, "%s: null pointer", what);
    AMPNET_REQUIRE(save_mean && save_invstd, "%s: null save_mean or save_invstd", what);
    AMPNET_TRY(sa_check_cloud(what, n, ld, feats, D, nullptr));
    AMPNET_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "%s: momentum=%g must be in [0, 1]", what, (double)momentum);
    SatFwdShape sh;
    AMPNET_TRY(sat_fwd_shape(what, D, n_clouds, s, nsample, cout_host, L, sh));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.floats * sizeof(float)));
    MlpPlan p;
    MlpFold f;
    const int lds = mlp_plan_build(what, 3 + D, sh.R, params_host, cout_host, eps_host, L, p, f);
    if (!lds) return AMPNET_E_ARG;
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sat_stats_kernel), attr_set));
    float *ws = static_cast<float *>(workspace), *parts = ws + sh.off_parts;
    int ch = 0;
    for (int l = 0; l < L; ++l) {
        MlpPlan pl = p;                                        // pass l runs layers < l from staged weights and reads layer l through L2
        for (int j = l; j < L; ++j) pl.w_off[j] = -1;
        hipLaunchKernelGGL(sat_stats_kernel, dim3(cdiv(sh.n_parts, p.nw)), dim3(64 * p.nw), lds, st, pl, l, xyz, n, ld, centres, s, group_idx,
                           nsample, feats, D, ws, sh.n_groups, sh.n_parts, parts);
        AMPNET_TRY(check_launch("sat_stats_kernel"));
        FptStats q = {f.bias[l], f.gamma[l], f.beta[l], params_host[6 * l + 4], params_host[6 * l + 5], save_mean + ch, save_invstd + ch,
                      f.eps[l],  momentum,   p.cout[l], p.fold_off[l]};
        AMPNET_TRY(fpt_stats_finalize_launch(q, parts, sh.n_parts, sh.M, ws, st));
        ch += p.cout[l];
    }
    return sa_forward_launch(what, p, lds, xyz, n_clouds, n, ld, centres, s, group_idx, nsample, feats, D, ws, out, st);
}

extern "C" size_t ampnet_sa_train_backward_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L)
{
    using namespace ampnet;
    SaBwdShape sh;
    size_t off_coef, off_arg, floats;
    if (sat_bwd_shape("ampnet_sa_train_backward_workspace_bytes", D, n_clouds, s, nsample, cout_host, L, sh, off_coef, off_arg, floats) != AMPNET_OK)
        return 0;
    return floats * sizeof(float);
}

extern "C" int ampnet_sa_train_backward_tape(int D, int n_clouds, int s, int nsample, const int *cout_host, int L, int l, size_t *x_offset_bytes,
                                             int *x_stride, size_t *dz_offset_bytes, int *dz_stride)
{
    using namespace ampnet;
    const char *what = "ampnet_sa_train_backward_tape";
    AMPNET_REQUIRE(x_offset_bytes && x_stride && dz_offset_bytes && dz_stride, "%s: null pointer", what);
    SaBwdShape sh;
    size_t off_coef, off_arg, floats;
    AMPNET_TRY(sat_bwd_shape(what, D, n_clouds, s, nsample, cout_host, L, sh, off_coef, off_arg, floats));
    AMPNET_REQUIRE(l >= 0 && l < L, "%s: layer %d of %d", what, l, L);
    *x_offset_bytes = sh.off_xs[l] * sizeof(float);
    *x_stride = sh.ldxs[l];
    *dz_offset_bytes = sh.off_dz[l] * sizeof(float);
    *dz_stride = cout_host[l];
    return AMPNET_OK;
}

namespace ampnet {

// The body of ampnet_sa_train_backward_f32 and ampnet_sa_train_backward_ragged_f32 (sa_tiles.h, BwdClouds): the phases and the statistics
// over c's groups as one batch, the dfeats gather alone ragged.
static int sa_train_backward_run(const char *what, const float *xyz, const BwdClouds &c, int ld, const int32_t *centres, const int32_t *group_idx,
                                 int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                                 const float *eps_host, int L, const float *dout, float *dfeats, float *const *grads_host, int32_t *arg_out,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    const int n_clouds = c.n_clouds, n = c.n, s = c.s;
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(xyz && centres && group_idx && params_host && cout_host && eps_host && dout && grads_host, "%s: null pointer", what);
    SaBwdShape sh;
    size_t off_coef, off_arg, floats;
    AMPNET_TRY(sa_check_cloud(what, n, ld, feats, D, dfeats));
    AMPNET_TRY(sat_bwd_shape(what, D, n_clouds, s, nsample, cout_host, L, sh, off_coef, off_arg, floats));
    AMPNET_REQUIRE((long long)n_clouds * n <= 0x7fffffffLL, "%s: n_clouds * n = %lld points exceed 2^31 - 1", what, (long long)n_clouds * n);
    AMPNET_TRY(sa_check_tables(what, nullptr, grads_host, L));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, floats * sizeof(float)));
    MlpPlan p;
    MlpFold f;
    if (!mlp_plan_build(what, 3 + D, sh.R, params_host, cout_host, eps_host, L, p, f)) return AMPNET_E_ARG;
    mlp_plan_unstaged(p);
    float *ws = static_cast<float *>(workspace);
    BntBwd b;
    const size_t lds = bnt_bwd_plan(p, f, sh, ws, off_coef, b);
    b.arg = reinterpret_cast<int32_t *>(ws + off_arg);
    static bool attr_last = false, attr_phase = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sat_bwd_last_kernel), attr_last));
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sat_bwd_phase_kernel), attr_phase));
    AMPNET_TRY(fpt_fold_launch(p, f, ws, st));
    const int n_tiles = sh.n_groups * (sh.R / 32);             // (n_groups <= 2^24: M is)
    for (int l = L - 1; l >= -1; --l) {
        if (l == L - 1) {
            hipLaunchKernelGGL(sat_bwd_last_kernel, dim3(sh.grid), dim3(64), lds, st, p, b, xyz, n, ld, centres, s, group_idx, nsample, feats, D, ws,
                               dout, sh.n_groups, arg_out);
            AMPNET_TRY(check_launch("sat_bwd_last_kernel"));
        } else {
            hipLaunchKernelGGL(sat_bwd_phase_kernel, dim3(sh.grid), dim3(64), lds, st, p, b, l, nsample, D, ws, dout, n_tiles, dfeats ? 1 : 0);
            AMPNET_TRY(check_launch("sat_bwd_phase_kernel"));
        }
        if (l < 0) break;
        AMPNET_TRY(fpt_bwd_finalize_launch(p.cout[l], b.parts, sh.grid, sh.M, f.mean[l], f.var[l], grads_host[4 * l + 1], grads_host[4 * l + 2],
                                           grads_host[4 * l + 3], b.coef + p.fold_off[l], st));
    }
    for (int l = 0; l < L; ++l) {
        AMPNET_TRY(fpb_wgrad_launch(b.dz[l], p.cout[l], b.xs[l], p.cin[l], sh.ldxs[l], sh.M, sh.chunk_rows, sh.chunks, ws + sh.off_wpart,
                                    grads_host[4 * l], st));
    }
    if (dfeats) return sa_gather_launch(b.dx0, D, c, nsample, group_idx, dfeats, st);
    return AMPNET_OK;
}

}  // namespace ampnet

extern "C" int ampnet_sa_train_backward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s,
                                            const int32_t *group_idx, int nsample, const float *feats, int D, const float *const *params_host,
                                            const int *cout_host, const float *eps_host, int L, const float *dout, float *dfeats,
                                            float *const *grads_host, int32_t *arg_out, void *workspace, size_t workspace_bytes, void *stream)
{
    const ampnet::BwdClouds c = {n_clouds, n, s, nullptr, 0, 0};
    return ampnet::sa_train_backward_run("ampnet_sa_train_backward_f32", xyz, c, ld, centres, group_idx, nsample, feats, D, params_host, cout_host,
                                         eps_host, L, dout, dfeats, grads_host, arg_out, workspace, workspace_bytes, stream);
}

extern "C" int ampnet_sa_train_backward_ragged_f32(const float *xyz, const int32_t *cloud_off, int n_clouds, int total, int ld,
                                                   const int32_t *centres, int s, const int32_t *group_idx, int nsample, const float *feats,
                                                   int D, const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                                                   const float *dout, float *dfeats, float *const *grads_host, int32_t *arg_out,
                                                   void *workspace, size_t workspace_bytes, void *stream)
{
    ampnet::BwdClouds c;
    const int rc = ampnet::bwd_clouds_ragged("ampnet_sa_train_backward_ragged_f32", cloud_off, n_clouds, total, s, c);
    if (rc != AMPNET_OK) return rc;
    return ampnet::sa_train_backward_run("ampnet_sa_train_backward_ragged_f32", xyz, c, ld, centres, group_idx, nsample, feats, D, params_host,
                                         cout_host, eps_host, L, dout, dfeats, grads_host, arg_out, workspace, workspace_bytes, stream);
}
