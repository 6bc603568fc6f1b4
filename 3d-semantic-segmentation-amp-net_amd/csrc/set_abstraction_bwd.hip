// set_abstraction_bwd.hip -- the backward of one fused set-abstraction layer with BatchNorm's running statistics frozen (C ABI:
// ampnet_sa_backward_f32, ampnet_sa_backward_workspace_bytes).  The math per layer is that of feature_propagation_bwd.hip's header
// (dy, dbeta, G, dgamma, dz, dbias, dW, dx); the rows are the forward's, [xyz[idx_t] - xyz[centre], feats[idx_t]], and dx of the last layer
// is `dout` routed through the max over the group.  The forward keeps nothing, so everything is recomputed.  Kernels on the caller's stream:
//
//   fold (sa_fold_kernel)   scale and shift, as in the forward.
//   sa_backward_kernel      A workgroup is ONE wave and a wave owns a group, as in the forward.  It gathers the group's rows with the
//       forward's code into tile X_0 (R = 32 or 64 rows, rows past nsample repeat row 0), runs layers 0 .. L-2 forward with the forward's own
//       code (mlp_dispatch<K_PAIRS>, weights read through L2) into tiles X_1 .. X_{L-1} and keeps ALL of them, then walks the layers
//       backward as fp_backward_kernel does: the accumulators a of layer l are computed AGAIN from X_l in the forward's contraction order
//       (K_PAIRS: k-step i of lane half h takes k = k0 + 2 i + h; the same bits, so the same ReLU mask and the same max), dx_{l+1} becomes
//       dz in place in X_{l+1}, and dx_l = dz W overwrites X_l.  L + 1 tiles of R rows: at R = 32 every shape of the forward fits the 160 KB
//       (cin_0 = 320 with three layers of 256: 140 KB); at R = 64 the shapes whose tiles do not fit are refused.
//       The max.  In the last layer a lane holds, per row tile, column c of 16 rows in its accumulator; it keeps the largest relu(y), the
//       row that attains it and that row's a over both row tiles in a SaArgMax (sa_tiles.h: the walk, and the rule that the LOWEST row
//       wins a tie).  Rows past nsample and the slots ball query filled by repeating its first member are bit-identical to an earlier row
//       and never win.  dz of the last layer is zero except at (winner, c), where it is dout[g, c] scale if the winner's y > 0: the walk
//       stores the zeros as it goes, and the lane that stored the winner's zero writes the value over it.
//       The wave stores x_l and dz_l of its nsample real rows to the workspace (dW below) and adds its per-channel sums of dy and dy a
//       (rows in the accumulator's order, row tiles ascending, lane half 0 before half 1, groups ascending) into ITS OWN row of a partials
//       array: every element is read and written by the same lane only.  dx_0's columns [3, cin_0) go to the workspace for the gather
//       below; when the caller wants no dfeats, layer 0's dx is not computed at all.
//   fp_wgrad_kernel, fp_wgrad_reduce_kernel, fp_bwd_finalize_kernel   mlp_bwd.hip, shared with the feature-propagation backward.
//   sa_dfeats_kernel        dfeats as a GATHER: one wave per point j scans its cloud's s nsample group entries in ascending order, 64 at a
//       time, takes the entries equal to j (clamped as in the forward) by ballot and adds dx_0[entry, 3:] in ascending entry order, a lane
//       per column.  No float atomics; a point in no group gets zeros.
//
// Every order above is a function of the shape alone: two runs give the same bits.  Exact fp32 MFMA whatever the matrix precision is.
#include "sa_tiles.h"

namespace ampnet {

struct SaBwdPlan {
    int off_x[MLP_MAX_LAYERS + 1], ld_x[MLP_MAX_LAYERS + 1];   // tile X_l: float offset in LDS, odd row stride
    int ldxs[MLP_MAX_LAYERS];                                  // row stride of x_l in the workspace: cin_l rounded up to 32 (zeros)
    int sum_c;                                                 // sum of cout_l; layer l's channels start at fold_off[l] / 2
    float *xs[MLP_MAX_LAYERS], *dz[MLP_MAX_LAYERS], *dx0, *parts;
};

// A layer below the last: d [R][ldd] holds dx_{l+1} on entry and dz on exit; dz_ws: the group's rows of the workspace.
template <int NT>
__device__ __forceinline__ void sab_hidden(const float *x, int ldx, const float *__restrict__ w, int cin, int kp, int cout, int n0,
                                           const float *__restrict__ scale, const float *__restrict__ shift, float *d, int ldd, int R,
                                           int nsample, float *__restrict__ dz_ws, float *part_b, float *part_g, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    float sc[NT], sh[NT], sb[NT], sg[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        sc[t] = scale[n0 + 32 * t + r];
        sh[t] = shift[n0 + 32 * t + r];
        sb[t] = sg[t] = 0.0f;
    }
    for (int m0 = 0; m0 < R; m0 += 32) {
        f32x16 acc[NT];
        mlp_accumulate<NT, K_PAIRS, false>(acc, mlp_operand<K_PAIRS>(x, ldx, m0 + r, h), w, cin, cin, kp, n0, r, h);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = n0 + 32 * t + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;   // mlp_acc_row(i, h), spelled out with m0 first: see sab_last
                const float a = acc[t][i];
                const float dy = fmaf(a, sc[t], sh[t]) > 0.0f ? d[row * ldd + col] : 0.0f;
                sb[t] += dy;
                sg[t] = fmaf(dy, a, sg[t]);
                const float dzv = dy * sc[t];
                d[row * ldd + col] = dzv;
                if (row < nsample) dz_ws[(size_t)row * cout + col] = dzv;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        const float ob = __shfl_down(sb[t], 32), og = __shfl_down(sg[t], 32);
        if (h == 0) {                             // (this lane alone ever touches these two words of the workgroup's partials)
            part_b[col] += sb[t] + ob;
            part_g[col] += sg[t] + og;
        }
    }
}

// The last layer: the max over the group's rows and its row (SaArgMax), and dz = dout scale at that row alone.  dout_g, arg_g: the group's
// row of dout / arg_out (arg_g may be null).
template <int NT>
__device__ __forceinline__ void sab_last(const float *x, int ldx, const float *__restrict__ w, int cin, int kp, int cout, int n0,
                                         const float *__restrict__ scale, const float *__restrict__ shift, float *d, int ldd, int R,
                                         int nsample, const float *__restrict__ dout_g, float *__restrict__ dz_ws, float *part_b,
                                         float *part_g, int32_t *__restrict__ arg_g, int lane)
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
        f32x16 acc[NT];
        mlp_accumulate<NT, K_PAIRS, false>(acc, mlp_operand<K_PAIRS>(x, ldx, m0 + r, h), w, cin, cin, kp, n0, r, h);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = n0 + 32 * t + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                // m0 + mlp_acc_row(i, h), ascending in (m0, i) as SaArgMax asks.  Spelled out here, in sab_hidden and in sat_last: hipcc
                // folds the row into the stores' address arithmetic in the order the sum is written, and m0 + (the helper's sum) costs this
                // kernel other instructions than (m0 + ..) + 4 h does.
                const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                const float a = acc[t][i], y = fmaxf(fmaf(a, sc[t], sh[t]), 0.0f);
                am[t].put(a, y, row);
                d[row * ldd + col] = 0.0f;
                if (row < nsample) dz_ws[(size_t)row * cout + col] = 0.0f;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        am[t].merge_halves();                     // both halves agree now; rows past nsample repeat row 0 and lose the tie to it
        const int brow = am[t].row;
        const float dy = am[t].best > 0.0f ? dout_g[col] : 0.0f, dzv = dy * sc[t];
        if ((((brow & 31) >> 2) & 1) == h) {      // the lane that wrote this element's zero above
            d[brow * ldd + col] = dzv;
            if (brow < nsample) dz_ws[(size_t)brow * cout + col] = dzv;
        }
        if (h == 0) {
            part_b[col] += dy;
            part_g[col] += dy * am[t].a;
            if (arg_g) arg_g[col] = brow;
        }
    }
}

__global__ __launch_bounds__(64) void sa_backward_kernel(MlpPlan p, SaBwdPlan b, const float *__restrict__ xyz, int n, int ld,
                                                        const int32_t *__restrict__ centres, int s, const int32_t *__restrict__ group_idx,
                                                        int nsample, const float *__restrict__ feats, int D, const float *__restrict__ fold,
                                                        const float *__restrict__ dout, int n_groups, int want_dx0,
                                                        int32_t *__restrict__ arg_out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x;
    const int L = p.L, R = p.R;
    const int cin0 = p.cin[0], kp0 = p.kp[0], cout_last = p.cout[L - 1];
    float *part_b = b.parts + (size_t)blockIdx.x * 2 * b.sum_c, *part_g = part_b + b.sum_c;
    if (lane < 32)
        for (int c = lane; c < b.sum_c; c += 32) part_b[c] = part_g[c] = 0.0f;       // channel c belongs to lane c % 32, here and below
    for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
        float *x0 = s_mem + b.off_x[0];
        sa_gather_group(x0, b.ld_x[0], R, kp0, cin0, xyz, n, ld, centres, s, group_idx, nsample, feats, D, g, lane);
        wave_lds_sync();
        const size_t grow = (size_t)g * nsample;
        fpb_store_rows(x0, b.ld_x[0], kp0, b.xs[0] + grow * b.ldxs[0], b.ldxs[0], nsample, lane);
        for (int l = 0; l + 1 < L; ++l) {
            float *y = s_mem + b.off_x[l + 1];
            mlp_dispatch<K_PAIRS>(p, l, R, s_mem, s_mem + b.off_x[l], b.ld_x[l], fold, MlpToTile{y, b.ld_x[l + 1]}, nullptr, lane);
            wave_lds_sync();
            fpb_store_rows(y, b.ld_x[l + 1], p.cout[l], b.xs[l + 1] + grow * b.ldxs[l + 1], b.ldxs[l + 1], nsample, lane);
        }
        for (int l = L - 1; l >= 0; --l) {
            float *x = s_mem + b.off_x[l], *d = s_mem + b.off_x[l + 1];
            const int ldx = b.ld_x[l], ldd = b.ld_x[l + 1], cin = p.cin[l], cout = p.cout[l], ch = p.fold_off[l] / 2;
            const float *scale = fold + p.fold_off[l], *shift = scale + cout;
            float *dz_ws = b.dz[l] + grow * cout;
            int n0 = 0;
            if (l == L - 1) {
                const float *dout_g = dout + (size_t)g * cout_last;
                int32_t *arg_g = arg_out ? arg_out + (size_t)g * cout_last : nullptr;
                for (; n0 + 128 <= cout; n0 += 128)
                    sab_last<4>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, R, nsample, dout_g, dz_ws, part_b + ch, part_g + ch, arg_g, lane);
                for (; n0 < cout; n0 += 32)
                    sab_last<1>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, R, nsample, dout_g, dz_ws, part_b + ch, part_g + ch, arg_g, lane);
            } else {
                for (; n0 + 128 <= cout; n0 += 128)
                    sab_hidden<4>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, R, nsample, dz_ws, part_b + ch, part_g + ch, lane);
                for (; n0 < cout; n0 += 32)
                    sab_hidden<1>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, R, nsample, dz_ws, part_b + ch, part_g + ch, lane);
            }
            wave_lds_sync();
            if (l == 0 && !want_dx0) break;       // (wave-uniform) nobody asked for dfeats: dx_0 is not needed
            for (int m0 = 0; m0 < R; m0 += 32) {
                float *xo = l ? x + m0 * ldx : nullptr;
                float *dx0 = b.dx0 + (grow + m0) * D;
                const float *dm = d + m0 * ldd;
                int c0 = 0;
                for (; c0 + 128 <= cin; c0 += 128) mlp_dgrad<4, true>(dm, ldd, p.w[l], cin, cout, c0, xo, ldx, nullptr, 3, dx0, D, nsample - m0, lane);
                for (; c0 < cin; c0 += 32) mlp_dgrad<1, true>(dm, ldd, p.w[l], cin, cout, c0, xo, ldx, nullptr, 3, dx0, D, nsample - m0, lane);
            }
            wave_lds_sync();
        }
        wave_lds_sync();                          // the next group's gather overwrites X_0
    }
}

__global__ __launch_bounds__(64) void sa_dfeats_kernel(const float *__restrict__ dx0, int D, int n, int s, int nsample,
                                                      const int32_t *__restrict__ group_idx, float *__restrict__ dfeats)
{
    const int lane = threadIdx.x;
    const int cloud_i = blockIdx.x / n, j = blockIdx.x - cloud_i * n;
    const long long total = (long long)s * nsample;
    const int32_t *ic = group_idx + (size_t)cloud_i * total;
    const float *gx = dx0 + (size_t)cloud_i * total * D;
    constexpr int U = (AMPNET_SA_MAX_CIN + 63) / 64;
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0f;
    for (long long e0 = 0; e0 < total; e0 += 64) {
        const long long e = e0 + lane;
        const bool hit = e < total && min(max(ic[e], 0), n - 1) == j;
        unsigned long long mask = __ballot(hit);
        while (mask) {                            // wave-uniform: every lane walks the hits in ascending entry order
            const int src = __ffsll(mask) - 1;
            mask &= mask - 1;
            const float *row = gx + (size_t)(e0 + src) * D;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (lane + 64 * u < D) acc[u] += row[lane + 64 * u];
        }
    }
    float *dst = dfeats + (size_t)blockIdx.x * D;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (lane + 64 * u < D) dst[lane + 64 * u] = acc[u];
}

// sa_dfeats_kernel for clouds of UNEQUAL size packed back to back (ampnet_sa_backward_ragged_f32): one wave per point j = blockIdx.x of the
// packed array.  Its cloud b -- cloud_off[b] <= j < cloud_off[b + 1], a binary search over the table, wave-uniform -- has the centres
// [b s, (b + 1) s), and the wave scans the s nsample group entries of those centres alone, not those of the whole array.  The entries are
// GLOBAL point indices and are clamped into the cloud's own rows; the hits are added in ascending entry order with sa_dfeats_kernel's own
// statements, so cloud by cloud the result is what that kernel writes for the cloud alone, bit for bit.  b stays in [0, n_clouds - 1]
// whatever the table holds, so nothing is read past group_idx or dx0.
__global__ __launch_bounds__(64) void sa_dfeats_ragged_kernel(const float *__restrict__ dx0, int D, const int32_t *__restrict__ cloud_off,
                                                             int n_clouds, int s, int nsample, const int32_t *__restrict__ group_idx,
                                                             float *__restrict__ dfeats)
{
    const int lane = threadIdx.x;
    const int j = blockIdx.x;
    int cloud_i = 0, above = n_clouds;
    while (above - cloud_i > 1) {                 // the last cloud whose first row is <= j
        const int mid = (cloud_i + above) >> 1;
        if (cloud_off[mid] <= j) cloud_i = mid;
        else above = mid;
    }
    const int lo = cloud_off[cloud_i], hi = cloud_off[cloud_i + 1] - 1;
    const long long total = (long long)s * nsample;
    const int32_t *ic = group_idx + (size_t)cloud_i * total;
    const float *gx = dx0 + (size_t)cloud_i * total * D;
    constexpr int U = (AMPNET_SA_MAX_CIN + 63) / 64;
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0f;
    for (long long e0 = 0; e0 < total; e0 += 64) {
        const long long e = e0 + lane;
        const bool hit = e < total && min(max(ic[e], lo), hi) == j;
        unsigned long long mask = __ballot(hit);
        while (mask) {                            // wave-uniform: every lane walks the hits in ascending entry order
            const int src = __ffsll(mask) - 1;
            mask &= mask - 1;
            const float *row = gx + (size_t)(e0 + src) * D;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (lane + 64 * u < D) acc[u] += row[lane + 64 * u];
        }
    }
    float *dst = dfeats + (size_t)blockIdx.x * D;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (lane + 64 * u < D) dst[lane + 64 * u] = acc[u];
}

int sab_shape(const char *what, int D, int n_clouds, int s, int nsample, const int *cout_host, int L, SaBwdShape &sh)
{
    AMPNET_REQUIRE(cout_host, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && s >= 1, "%s: bad shape n_clouds=%d s=%d", what, n_clouds, s);
    AMPNET_TRY(sa_check_limits(what, D, n_clouds, s, nsample, L, false));
    sh = {};
    sh.R = nsample <= 32 ? 32 : 64;
    sh.n_groups = n_clouds * s;
    sh.M = (long long)sh.n_groups * nsample;
    sh.grid = sh.n_groups < SAB_MAX_GRID ? sh.n_groups : SAB_MAX_GRID;
    fpb_chunk_rule(sh.M, sh.chunk_rows, sh.chunks);
    AMPNET_TRY(mlp_bwd_layout(what, align_up((size_t)AMPNET_SA_WORKSPACE_BYTES / sizeof(float), 64), 3 + D, D, sh.M, sh.grid, sh.chunks, cout_host,
                                        L, sh));
    // the tiles X_0 .. X_L of R rows
    for (int l = 0; l <= L; ++l) {
        sh.ld_x[l] = (l ? cout_host[l - 1] : (3 + D + 7) / 8 * 8) + 1;
        sh.off_x[l] = sh.lds_floats;
        sh.lds_floats += sh.R * sh.ld_x[l];
    }
    AMPNET_REQUIRE((size_t)sh.lds_floats * sizeof(float) <= (size_t)MLP_LDS_BYTES,
                   "%s: a wave's %d tiles of %d rows (%zu bytes) exceed the LDS (%d bytes); at nsample <= 32 every shape fits", what, L + 1, sh.R,
                   (size_t)sh.lds_floats * sizeof(float), MLP_LDS_BYTES);
    return AMPNET_OK;
}

int sa_dfeats_launch(const float *dx0, int D, int n_clouds, int n, int s, int nsample, const int32_t *group_idx, float *dfeats, hipStream_t st)
{
    hipLaunchKernelGGL(sa_dfeats_kernel, dim3(n_clouds * n), dim3(64), 0, st, dx0, D, n, s, nsample, group_idx, dfeats);
    return check_launch("sa_dfeats_kernel");
}

int sa_gather_launch(const float *dx0, int D, const BwdClouds &c, int nsample, const int32_t *group_idx, float *dfeats, hipStream_t st)
{
    if (!c.cloud_off) return sa_dfeats_launch(dx0, D, c.n_clouds, c.n, c.s, nsample, group_idx, dfeats, st);
    hipLaunchKernelGGL(sa_dfeats_ragged_kernel, dim3(c.n), dim3(64), 0, st, dx0, D, c.cloud_off, c.q, c.s_cloud, nsample, group_idx, dfeats);
    return check_launch("sa_dfeats_ragged_kernel");
}

}  // namespace ampnet

extern "C" size_t ampnet_sa_backward_workspace_bytes(int D, int n_clouds, int s, int nsample, const int *cout_host, int L)
{
    using namespace ampnet;
    SaBwdShape sh;
    if (sab_shape("ampnet_sa_backward_workspace_bytes", D, n_clouds, s, nsample, cout_host, L, sh) != AMPNET_OK) return 0;
    return sh.floats * sizeof(float);
}

namespace ampnet {

// The body of ampnet_sa_backward_f32 and ampnet_sa_backward_ragged_f32: every phase runs on c's (n_clouds, n, s) -- the packed array as ONE
// cloud for the ragged entry point -- and the dfeats gather alone looks at c.cloud_off (sa_gather_launch).
static int sa_backward_run(const char *what, const float *xyz, const BwdClouds &c, int ld, const int32_t *centres, const int32_t *group_idx,
                           int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                           const float *eps_host, int L, const float *dout, float *dfeats, float *const *grads_host, int32_t *arg_out,
                           void *workspace, size_t workspace_bytes, void *stream)
{
    const int n_clouds = c.n_clouds, n = c.n, s = c.s;
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(xyz && centres && group_idx && params_host && cout_host && eps_host && dout && grads_host, "%s: null pointer", what);
    SaBwdShape sh;
    AMPNET_TRY(sa_check_cloud(what, n, ld, feats, D, dfeats));
    AMPNET_TRY(sab_shape(what, D, n_clouds, s, nsample, cout_host, L, sh));
    AMPNET_REQUIRE((long long)n_clouds * n <= 0x7fffffffLL, "%s: n_clouds * n = %lld points exceed 2^31 - 1", what, (long long)n_clouds * n);
    AMPNET_TRY(sa_check_tables(what, nullptr, grads_host, L));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.floats * sizeof(float)));
    MlpPlan p;
    MlpFold f;
    if (!mlp_plan_build(what, 3 + D, sh.R, params_host, cout_host, eps_host, L, p, f)) return AMPNET_E_ARG;
    mlp_plan_unstaged(p);
    float *ws = static_cast<float *>(workspace);
    SaBwdPlan b = {};
    b.sum_c = sh.sum_c;
    b.parts = ws + sh.off_parts;
    b.dx0 = ws + sh.off_dx0;
    for (int l = 0; l <= L; ++l) {
        b.off_x[l] = sh.off_x[l];
        b.ld_x[l] = sh.ld_x[l];
    }
    FpBwdFin g = {};
    for (int l = 0; l < L; ++l) {
        b.ldxs[l] = sh.ldxs[l];
        b.xs[l] = ws + sh.off_xs[l];
        b.dz[l] = ws + sh.off_dz[l];
        g.dbias[l] = grads_host[4 * l + 1];
        g.dgamma[l] = grads_host[4 * l + 2];
        g.dbeta[l] = grads_host[4 * l + 3];
    }
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sa_backward_kernel), attr_set));
    AMPNET_TRY(mlp_fold_launch(p, f, ws, st));
    hipLaunchKernelGGL(sa_backward_kernel, dim3(sh.grid), dim3(64), sh.lds_floats * sizeof(float), st, p, b, xyz, n, ld, centres, s, group_idx,
                       nsample, feats, D, ws, dout, sh.n_groups, dfeats ? 1 : 0, arg_out);
    AMPNET_TRY(check_launch("sa_backward_kernel"));
    for (int l = 0; l < L; ++l) {
        AMPNET_TRY(fpb_wgrad_launch(b.dz[l], p.cout[l], b.xs[l], p.cin[l], sh.ldxs[l], sh.M, sh.chunk_rows, sh.chunks, ws + sh.off_wpart,
                                    grads_host[4 * l], st));
    }
    if (dfeats) {
        AMPNET_TRY(sa_gather_launch(b.dx0, D, c, nsample, group_idx, dfeats, st));
    }
    return fpb_finalize_launch(p, f, g, ws, b.parts, sh.grid, sh.sum_c, st);
}

}  // namespace ampnet

extern "C" int ampnet_sa_backward_f32(const float *xyz, int n_clouds, int n, int ld, const int32_t *centres, int s, const int32_t *group_idx,
                                      int nsample, const float *feats, int D, const float *const *params_host, const int *cout_host,
                                      const float *eps_host, int L, const float *dout, float *dfeats, float *const *grads_host,
                                      int32_t *arg_out, void *workspace, size_t workspace_bytes, void *stream)
{
    const ampnet::BwdClouds c = {n_clouds, n, s, nullptr, 0, 0};
    return ampnet::sa_backward_run("ampnet_sa_backward_f32", xyz, c, ld, centres, group_idx, nsample, feats, D, params_host, cout_host, eps_host, L,
                                   dout, dfeats, grads_host, arg_out, workspace, workspace_bytes, stream);
}

extern "C" int ampnet_sa_backward_ragged_f32(const float *xyz, const int32_t *cloud_off, int n_clouds, int total, int ld, const int32_t *centres,
                                             int s, const int32_t *group_idx, int nsample, const float *feats, int D,
                                             const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                                             const float *dout, float *dfeats, float *const *grads_host, int32_t *arg_out, void *workspace,
                                             size_t workspace_bytes, void *stream)
{
    ampnet::BwdClouds c;
    const int rc = ampnet::bwd_clouds_ragged("ampnet_sa_backward_ragged_f32", cloud_off, n_clouds, total, s, c);
    if (rc != AMPNET_OK) return rc;
    return ampnet::sa_backward_run("ampnet_sa_backward_ragged_f32", xyz, c, ld, centres, group_idx, nsample, feats, D, params_host, cout_host,
                                   eps_host, L, dout, dfeats, grads_host, arg_out, workspace, workspace_bytes, stream);
}
