// feature_propagation_train.hip -- one fused feature-propagation layer with TRAIN-mode BatchNorm: batch statistics, running-statistics
// update, and the backward through the statistics (C ABI: ampnet_fp_train_forward_f32, ampnet_fp_train_backward_f32 and their
// _workspace_bytes).  The arithmetic is stated in include/ampnet_hip.h.  Everything runs on the caller's stream, no float atomics, every
// summation order a function of the shape alone; exact fp32 MFMA whatever the matrix precision is.
//
// FORWARD: L statistics passes, then the eval forward's kernel, unchanged.
//   fpt_stats_kernel (pass l)   The forward's workgroup (its plan: up to four waves that share the staged weights of layers < l); a wave
//       owns 32 consecutive fine points of one cloud at a time.  It rebuilds the tile's rows (fp_rows.h), runs layers < l with the
//       forward's own code (mlp_dispatch<K_QUADS>, reading the scale and shift that the earlier passes' finalizes wrote), forms layer l's
//       raw accumulators a = W x in the forward's contraction order (mlp_accumulate) and, per column, the tile's count, mean and
//       sum (a - mean)^2 over its VALID rows (the rows past n of a cloud's last tile enter none of the three).  The tiles r, r + P, ..
//       (P = min(tiles, 1024)) are merged in ascending order into row r of a partials array with Chan's pairwise formula; a row belongs to
//       one wave, so every word of it is read and written by the same lane only, and the order does not depend on the plan.
//   fpt_stats_finalize_kernel   (bn_train.hip) a wave per channel merges the rows with the same formula and writes scale_l, shift_l into
//       the fold, save_mean, save_invstd, and the running-statistics update.
//   fp_forward_kernel           the eval forward's kernel on that fold (fp_forward_launch): eval and train share the hot kernel, and the
//       accumulators the statistics were taken from are the ones it normalises, bit for bit.
//   Why recompute layers < l in every pass instead of spilling a_l: the eval forward keeps no activation in memory and neither does this;
//   the passes read only the inputs, so the forward's workspace stays a few hundred KB whatever M is.
//
// BACKWARD: L + 1 phases of one kernel in descending layer order, a finalize between them, then the eval backward's dW and gather.
//   dz_l needs sum dy and sum dy a over ALL rows, so no single kernel can go through more than one layer.
//   fpt_bwd_phase_kernel (phase l = L-1 .. -1), one wave per workgroup and tile as above, two LDS tiles T0 and T1:
//       l = L-1:  builds the rows, runs layers < L-1 forward and stores every layer input x_j to the workspace (dW reads them, and so do the
//                 later phases: the rows are never built again);  then part B below with dx = dout.
//       l < L-1:  part A for layer l+1: x_{l+1} from the workspace into T0, a_{l+1} recomputed, dy_{l+1} back from the workspace,
//                 dz_{l+1} = scale (dy - dbeta / M - (a - mu) invstd dgamma / M) with the sums final (zero for the rows past n) into T1 and
//                 over dy in the workspace;  dx_l = dz_{l+1} W_{l+1} (mlp_dgrad) over T0;  l = -1 ends here, dx_0 going to dpoints1 and the
//                 gather's rows.
//       part B for layer l:  x_l from the workspace into T1, a_l recomputed, dy_l = dx_l [fma(a, scale, shift) > 0] stored to the workspace,
//                 sum dy and sum dy a added into the workgroup's own partial row (rows in the accumulator's order, lane half 0 before
//                 half 1, tiles ascending).
//   fpt_bwd_finalize_kernel     (bn_train.hip) a wave per channel adds the partial rows and writes dbeta, dgamma = invstd (G - mu dbeta),
//       dbias = 0 and the two coefficients dbeta / M and dgamma invstd / M of the next phase.
//   fpb_wgrad_launch, fp_gather_launch    dW_l = dz_l^T x_l and dpoints2, exactly the eval backward's (the gather ragged when the clouds are).
//   A phase holds two tiles of the widest layer input (at most 131 KB), so the eval backward's shared-space special case is not needed.
//   The statistics, part A and part B of a tile are bn_train.h's (bnt_tile_stats, bnt_form_dz, bnt_form_dy), shared with the set
//   abstraction; this file keeps what is feature propagation's own: the row builder, the tiling and the entry points.
#include "bn_train.h"
#include "fp_bwd_tiles.h"

namespace ampnet {

constexpr long long FPT_MAX_ROWS = AMPNET_FP_TRAIN_MAX_ROWS;    // the merges carry row counts as floats: exact up to here, larger M is refused

// parts [n_parts][3 cout_l]: per partial row the count, mean and sum of squared deviations of every channel of layer l.  Row r takes the
// tiles r, r + n_parts, .. in ascending order and belongs to ONE wave, whatever the plan's waves per workgroup are.
__global__ __launch_bounds__(256) void fpt_stats_kernel(MlpPlan p, int l, const float *__restrict__ points1, int D1,
                                                       const float *__restrict__ points2, int D2, int n, int s,
                                                       const int32_t *__restrict__ idx, const float *__restrict__ dist2, int k,
                                                       const float *__restrict__ fold, int tiles_per_cloud, int n_tiles, int n_parts,
                                                       float *__restrict__ parts)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MlpLds m = mlp_lds(p, 32, s_mem, wave);
    mlp_stage_weights(p, m.s_w, tid, 64 * p.nw);                  // (the layers < l: the host took the others out of the staging)
    __syncthreads();
    const int cin = p.cin[l], cout = p.cout[l], kp = p.kp[l];
    float *tile[2] = {m.tile_a, m.tile_b};
    const int ld[2] = {p.ld_a, p.ld_b};
    for (int row = blockIdx.x * p.nw + wave; row < n_parts; row += gridDim.x * p.nw) {
        float *part_n = parts + (size_t)row * 3 * cout, *part_mean = part_n + cout, *part_m2 = part_mean + cout;
        if (lane < 32)
            for (int c = lane; c < cout; c += 32) part_n[c] = part_mean[c] = part_m2[c] = 0.0f;  // channel c belongs to lane c % 32
        for (int t = row; t < n_tiles; t += n_parts) {
            const int cloud_i = t / tiles_per_cloud, row0 = (t - cloud_i * tiles_per_cloud) * 32;
            const int rows = min(32, n - row0);
            fp_build_rows(tile[0], ld[0], p.kp[0], points1, D1, points2, D2, n, s, idx, dist2, k, cloud_i, row0, rows, lane);
            wave_lds_sync();
            for (int j = 0; j < l; ++j) {
                mlp_dispatch<K_QUADS>(p, j, 32, m.s_w, tile[j & 1], ld[j & 1], fold, MlpToTile{tile[(j + 1) & 1], ld[(j + 1) & 1]}, nullptr, lane);
                wave_lds_sync();
            }
            const float *x = tile[l & 1];
            const int ldx = ld[l & 1];
            int n0 = 0;
            if (p.w_vec[l]) {
                for (; n0 + 128 <= cout; n0 += 128) bnt_tile_stats<4, K_QUADS, true>(x, ldx, 0, p.w[l], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
                for (; n0 < cout; n0 += 32) bnt_tile_stats<1, K_QUADS, true>(x, ldx, 0, p.w[l], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
            } else {
                for (; n0 + 128 <= cout; n0 += 128) bnt_tile_stats<4, K_QUADS, false>(x, ldx, 0, p.w[l], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
                for (; n0 < cout; n0 += 32) bnt_tile_stats<1, K_QUADS, false>(x, ldx, 0, p.w[l], cin, kp, n0, rows, part_n, part_mean, part_m2, lane);
            }
            wave_lds_sync();                      // the next tile's rows overwrite tile A
        }
    }
}

__global__ __launch_bounds__(64) void fpt_bwd_phase_kernel(MlpPlan p, BntBwd b, int l, const float *__restrict__ points1, int D1,
                                                          const float *__restrict__ points2, int D2, int n, int s,
                                                          const int32_t *__restrict__ idx, const float *__restrict__ dist2, int k,
                                                          const float *__restrict__ fold, const float *__restrict__ dout, int tiles_per_cloud,
                                                          int n_tiles, float *__restrict__ dpoints1)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x;
    const int L = p.L, ld = b.ld;
    float *T[2] = {s_mem, s_mem + 32 * ld};
    float *part_b = nullptr, *part_g = nullptr;
    if (l >= 0) {
        part_b = b.parts + (size_t)blockIdx.x * 2 * p.cout[l];
        part_g = part_b + p.cout[l];
        if (lane < 32)
            for (int c = lane; c < p.cout[l]; c += 32) part_b[c] = part_g[c] = 0.0f;             // channel c belongs to lane c % 32
    }
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int cloud_i = tile / tiles_per_cloud, row0 = (tile - cloud_i * tiles_per_cloud) * 32;
        const int rows = min(32, n - row0);
        const size_t grow = (size_t)cloud_i * n + row0;
        const float *x_l = nullptr;               // the tile that holds x_l for part B
        if (l == L - 1) {
            fp_build_rows(T[0], ld, p.kp[0], points1, D1, points2, D2, n, s, idx, dist2, k, cloud_i, row0, rows, lane);
            wave_lds_sync();
            fpb_store_rows(T[0], ld, p.kp[0], b.xs[0] + grow * b.ldxs[0], b.ldxs[0], rows, lane);
            for (int j = 0; j + 1 < L; ++j) {
                float *y = T[(j + 1) & 1];
                mlp_dispatch<K_QUADS>(p, j, 32, s_mem, T[j & 1], ld, fold, MlpToTile{y, ld}, nullptr, lane);
                wave_lds_sync();
                fpb_store_rows(y, ld, p.cout[j], b.xs[j + 1] + grow * b.ldxs[j + 1], b.ldxs[j + 1], rows, lane);
            }
            x_l = T[(L - 1) & 1];
        } else {
            const int j = l + 1, cin = p.cin[j], cout = p.cout[j], kp = p.kp[j];
            fpb_load_rows(T[0], ld, kp, b.xs[j] + grow * b.ldxs[j], b.ldxs[j], rows, lane);
            wave_lds_sync();
            const float *scale = fold + p.fold_off[j], *shift = scale + cout, *c1 = b.coef + p.fold_off[j], *c2 = c1 + cout;
            float *dz_ws = b.dz[j] + grow * cout;
            int n0 = 0;
            if (p.w_vec[j]) {
                for (; n0 + 128 <= cout; n0 += 128)
                    bnt_form_dz<4, K_QUADS, true>(T[0], ld, p.w[j], cin, kp, cout, n0, scale, shift, b.mean[j], c1, c2, T[1], ld, rows, 0, nullptr, nullptr, dz_ws, lane);
                for (; n0 < cout; n0 += 32)
                    bnt_form_dz<1, K_QUADS, true>(T[0], ld, p.w[j], cin, kp, cout, n0, scale, shift, b.mean[j], c1, c2, T[1], ld, rows, 0, nullptr, nullptr, dz_ws, lane);
            } else {
                for (; n0 + 128 <= cout; n0 += 128)
                    bnt_form_dz<4, K_QUADS, false>(T[0], ld, p.w[j], cin, kp, cout, n0, scale, shift, b.mean[j], c1, c2, T[1], ld, rows, 0, nullptr, nullptr, dz_ws, lane);
                for (; n0 < cout; n0 += 32)
                    bnt_form_dz<1, K_QUADS, false>(T[0], ld, p.w[j], cin, kp, cout, n0, scale, shift, b.mean[j], c1, c2, T[1], ld, rows, 0, nullptr, nullptr, dz_ws, lane);
            }
            wave_lds_sync();
            // dx_l = dz_j W_j over T0 (x_j has been used), or to dpoints1 and the gather's rows
            float *xo = j ? T[0] : nullptr;
            float *dp1 = dpoints1 ? dpoints1 + grow * D1 : nullptr, *dx0 = b.dx0 + grow * D2;
            int c0 = 0;
            for (; c0 + 128 <= cin; c0 += 128) mlp_dgrad<4>(T[1], ld, p.w[j], cin, cout, c0, xo, ld, dp1, D1, dx0, D2, rows, lane);
            for (; c0 < cin; c0 += 32) mlp_dgrad<1>(T[1], ld, p.w[j], cin, cout, c0, xo, ld, dp1, D1, dx0, D2, rows, lane);
            wave_lds_sync();
            if (l >= 0) {
                fpb_load_rows(T[1], ld, p.kp[l], b.xs[l] + grow * b.ldxs[l], b.ldxs[l], rows, lane);
                wave_lds_sync();
                x_l = T[1];
            }
        }
        if (l >= 0) {
            const int cin = p.cin[l], cout = p.cout[l], kp = p.kp[l];
            const float *scale = fold + p.fold_off[l], *shift = scale + cout;
            const float *dsrc = l == L - 1 ? dout + grow * cout : nullptr;
            float *dz_ws = b.dz[l] + grow * cout;
            int n0 = 0;
            if (p.w_vec[l]) {
                for (; n0 + 128 <= cout; n0 += 128)
                    bnt_form_dy<4, K_QUADS, true, true>(x_l, ld, p.w[l], cin, kp, cout, n0, scale, shift, T[0], ld, dsrc, rows, dz_ws, part_b, part_g, lane);
                for (; n0 < cout; n0 += 32)
                    bnt_form_dy<1, K_QUADS, true, true>(x_l, ld, p.w[l], cin, kp, cout, n0, scale, shift, T[0], ld, dsrc, rows, dz_ws, part_b, part_g, lane);
            } else {
                for (; n0 + 128 <= cout; n0 += 128)
                    bnt_form_dy<4, K_QUADS, false, true>(x_l, ld, p.w[l], cin, kp, cout, n0, scale, shift, T[0], ld, dsrc, rows, dz_ws, part_b, part_g, lane);
                for (; n0 < cout; n0 += 32)
                    bnt_form_dy<1, K_QUADS, false, true>(x_l, ld, p.w[l], cin, kp, cout, n0, scale, shift, T[0], ld, dsrc, rows, dz_ws, part_b, part_g, lane);
            }
        }
        wave_lds_sync();                          // the next tile overwrites both tiles
    }
}

// what the forward's two entry points derive from the shape
struct FptFwdShape {
    long long M;
    int tiles_per_cloud, n_tiles, grid, sum_c;
    size_t off_parts, floats;
};

static int fpt_fwd_shape(const char *what, int D1, int D2, int n_clouds, int n, const int *cout_host, int L, FptFwdShape &sh)
{
    FpBwdShape b;                                 // (the limits are the backward's, which are the eval forward's)
    int rc = fpb_shape(what, D1, D2, n_clouds, n, cout_host, L, b);
    if (rc != AMPNET_OK) return rc;
    rc = bnt_rows_ok(what, b.M, FPT_MAX_ROWS, "n_clouds * n");
    if (rc != AMPNET_OK) return rc;
    sh = {};
    sh.M = b.M;
    sh.tiles_per_cloud = b.tiles_per_cloud;
    sh.n_tiles = b.n_tiles;
    sh.grid = b.grid;
    sh.sum_c = b.sum_c;
    int widest = 0;
    for (int l = 0; l < L; ++l) widest = cout_host[l] > widest ? cout_host[l] : widest;
    sh.off_parts = align_up((size_t)AMPNET_FP_WORKSPACE_BYTES / sizeof(float), 64);
    sh.floats = sh.off_parts + align_up((size_t)sh.grid * 3 * widest, 64);
    return AMPNET_OK;
}

}  // namespace ampnet

extern "C" size_t ampnet_fp_train_forward_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L)
{
    using namespace ampnet;
    FptFwdShape sh;
    if (fpt_fwd_shape("ampnet_fp_train_forward_workspace_bytes", D1, D2, n_clouds, n, cout_host, L, sh) != AMPNET_OK) return 0;
    return sh.floats * sizeof(float);
}

extern "C" int ampnet_fp_train_forward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s,
                                           const int32_t *idx, const float *dist2, int k, float *const *params_host, const int *cout_host,
                                           const float *eps_host, int L, float momentum, float *out, float *save_mean, float *save_invstd,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_fp_train_forward_f32";
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(points2 && idx && dist2 && params_host && cout_host && eps_host && out, "%s: null pointer", what);
    AMPNET_REQUIRE(save_mean && save_invstd, "%s: null save_mean or save_invstd", what);
    AMPNET_REQUIRE(s >= 1, "%s: bad shape s=%d", what, s);
    AMPNET_REQUIRE(k >= 1 && k <= 3 && k <= s, "%s: k=%d must be 1, 2 or 3 and <= s=%d", what, k, s);
    AMPNET_REQUIRE(D1 >= 0 && (D1 == 0) == (points1 == nullptr), "%s: points1 must be NULL exactly when D1 = 0 (D1=%d)", what, D1);
    AMPNET_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "%s: momentum=%g must be in [0, 1]", what, (double)momentum);
    FptFwdShape sh;
    int rc = fpt_fwd_shape(what, D1, D2, n_clouds, n, cout_host, L, sh);
    if (rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE(workspace && workspace_bytes >= sh.floats * sizeof(float), "%s: workspace of %zu bytes, need %zu", what, workspace_bytes,
                   sh.floats * sizeof(float));
    MlpPlan p;
    MlpFold f;
    const int lds = mlp_plan_build(what, D1 + D2, 32, params_host, cout_host, eps_host, L, p, f);
    if (!lds) return AMPNET_E_ARG;
    static bool attr_set = false;
    rc = mlp_allow_full_lds(what, reinterpret_cast<const void *>(fpt_stats_kernel), attr_set);
    if (rc != AMPNET_OK) return rc;
    float *ws = static_cast<float *>(workspace), *parts = ws + sh.off_parts;
    int ch = 0;
    for (int l = 0; l < L; ++l) {
        MlpPlan pl = p;                                        // pass l runs layers < l from staged weights and reads layer l through L2
        for (int j = l; j < L; ++j) pl.w_off[j] = -1;
        hipLaunchKernelGGL(fpt_stats_kernel, dim3(cdiv(sh.grid, p.nw)), dim3(64 * p.nw), lds, st, pl, l, points1, D1, points2, D2, n, s, idx, dist2,
                           k, ws, sh.tiles_per_cloud, sh.n_tiles, sh.grid, parts);
        rc = check_launch("fpt_stats_kernel");
        if (rc != AMPNET_OK) return rc;
        FptStats q = {f.bias[l], f.gamma[l], f.beta[l], params_host[6 * l + 4], params_host[6 * l + 5], save_mean + ch, save_invstd + ch,
                      f.eps[l],  momentum,   p.cout[l], p.fold_off[l]};
        rc = fpt_stats_finalize_launch(q, parts, sh.grid, sh.M, ws, st);
        if (rc != AMPNET_OK) return rc;
        ch += p.cout[l];
    }
    return fp_forward_launch(what, p, lds, points1, D1, points2, D2, n_clouds, n, s, idx, dist2, k, ws, out, st);
}

namespace ampnet {

static int fpt_bwd_shape(const char *what, int D1, int D2, int n_clouds, int n, const int *cout_host, int L, FpBwdShape &sh, size_t &off_coef,
                         size_t &floats)
{
    int rc = fpb_shape(what, D1, D2, n_clouds, n, cout_host, L, sh);
    if (rc != AMPNET_OK) return rc;
    rc = bnt_rows_ok(what, sh.M, FPT_MAX_ROWS, "n_clouds * n");
    if (rc != AMPNET_OK) return rc;
    off_coef = sh.floats;                         // behind the eval backward's layout: two coefficients per channel
    floats = off_coef + align_up((size_t)2 * sh.sum_c, 64);
    return AMPNET_OK;
}

}  // namespace ampnet

extern "C" size_t ampnet_fp_train_backward_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L)
{
    using namespace ampnet;
    FpBwdShape sh;
    size_t off_coef, floats;
    if (fpt_bwd_shape("ampnet_fp_train_backward_workspace_bytes", D1, D2, n_clouds, n, cout_host, L, sh, off_coef, floats) != AMPNET_OK) return 0;
    return floats * sizeof(float);
}

namespace ampnet {

// The body of ampnet_fp_train_backward_f32 and ampnet_fp_train_backward_ragged_f32 (fp_bwd_tiles.h, BwdClouds): the phases and the statistics
// over c's rows as one batch, the dpoints2 gather alone ragged.
static int fp_train_backward_run(const char *what, const float *points1, int D1, const float *points2, int D2, const BwdClouds &c,
                                 const int32_t *idx, const float *dist2, int k, const float *const *params_host, const int *cout_host,
                                 const float *eps_host, int L, const float *dout, float *dpoints1, float *dpoints2, float *const *grads_host,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    const int n_clouds = c.n_clouds, n = c.n, s = c.s;
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(points2 && idx && dist2 && params_host && cout_host && eps_host && dout && dpoints2 && grads_host, "%s: null pointer", what);
    AMPNET_REQUIRE(s >= 1, "%s: bad shape s=%d", what, s);
    AMPNET_REQUIRE(k >= 1 && k <= 3 && k <= s, "%s: k=%d must be 1, 2 or 3 and <= s=%d", what, k, s);
    AMPNET_REQUIRE(D1 >= 0 && (D1 == 0) == (points1 == nullptr), "%s: points1 must be NULL exactly when D1 = 0 (D1=%d)", what, D1);
    AMPNET_REQUIRE((D1 == 0) == (dpoints1 == nullptr), "%s: dpoints1 must be NULL exactly when D1 = 0 (D1=%d)", what, D1);
    FpBwdShape sh;
    size_t off_coef, floats;
    int rc = fpt_bwd_shape(what, D1, D2, n_clouds, n, cout_host, L, sh, off_coef, floats);
    if (rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE((long long)n_clouds * s <= 0x7fffffffLL, "%s: n_clouds * s = %lld coarse points exceed 2^31 - 1", what, (long long)n_clouds * s);
    for (int q = 0; q < 4 * L; ++q) AMPNET_REQUIRE(grads_host[q], "%s: null gradient pointer %d of layer %d", what, q % 4, q / 4);
    AMPNET_REQUIRE(workspace && workspace_bytes >= floats * sizeof(float), "%s: workspace of %zu bytes, need %zu", what, workspace_bytes,
                   floats * sizeof(float));
    MlpPlan p;
    MlpFold f;
    if (!mlp_plan_build(what, D1 + D2, 32, params_host, cout_host, eps_host, L, p, f)) return AMPNET_E_ARG;
    mlp_plan_unstaged(p);
    float *ws = static_cast<float *>(workspace);
    BntBwd b;
    const size_t lds = bnt_bwd_plan(p, f, sh, ws, off_coef, b);
    static bool attr_set = false;
    rc = mlp_allow_full_lds(what, reinterpret_cast<const void *>(fpt_bwd_phase_kernel), attr_set);
    if (rc != AMPNET_OK) return rc;
    rc = fpt_fold_launch(p, f, ws, st);
    if (rc != AMPNET_OK) return rc;
    for (int l = L - 1; l >= -1; --l) {
        hipLaunchKernelGGL(fpt_bwd_phase_kernel, dim3(sh.grid), dim3(64), lds, st, p, b, l, points1, D1, points2, D2, n, s, idx, dist2, k, ws, dout,
                           sh.tiles_per_cloud, sh.n_tiles, dpoints1);
        rc = check_launch("fpt_bwd_phase_kernel");
        if (rc != AMPNET_OK) return rc;
        if (l < 0) break;
        rc = fpt_bwd_finalize_launch(p.cout[l], b.parts, sh.grid, sh.M, f.mean[l], f.var[l], grads_host[4 * l + 1], grads_host[4 * l + 2],
                                     grads_host[4 * l + 3], b.coef + p.fold_off[l], st);
        if (rc != AMPNET_OK) return rc;
    }
    float *wpart = ws + sh.off_wpart;
    for (int l = 0; l < L; ++l) {
        rc = fpb_wgrad_launch(b.dz[l], p.cout[l], b.xs[l], p.cin[l], sh.ldxs[l], sh.M, sh.chunk_rows, sh.chunks, wpart, grads_host[4 * l], st);
        if (rc != AMPNET_OK) return rc;
    }
    return fp_gather_launch(b.dx0, D2, c, idx, dist2, k, dpoints2, st);
}

}  // namespace ampnet

extern "C" int ampnet_fp_train_backward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s,
                                            const int32_t *idx, const float *dist2, int k, const float *const *params_host,
                                            const int *cout_host, const float *eps_host, int L, const float *dout, float *dpoints1,
                                            float *dpoints2, float *const *grads_host, void *workspace, size_t workspace_bytes, void *stream)
{
    const ampnet::BwdClouds c = {n_clouds, n, s, nullptr, 0, 0};
    return ampnet::fp_train_backward_run("ampnet_fp_train_backward_f32", points1, D1, points2, D2, c, idx, dist2, k, params_host, cout_host,
                                         eps_host, L, dout, dpoints1, dpoints2, grads_host, workspace, workspace_bytes, stream);
}

extern "C" int ampnet_fp_train_backward_ragged_f32(const float *points1, int D1, const float *points2, int D2, const int32_t *cloud_off,
                                                   int n_clouds, int total, int s, const int32_t *idx, const float *dist2, int k,
                                                   const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                                                   const float *dout, float *dpoints1, float *dpoints2, float *const *grads_host,
                                                   void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "ampnet_fp_train_backward_ragged_f32";
    ampnet::BwdClouds c;
    int rc = ampnet::bwd_clouds_ragged(what, cloud_off, n_clouds, total, s, c);
    if (rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE(k <= s, "%s: k=%d must be <= s=%d, the coarse points of ONE cloud", what, k, s);
    return ampnet::fp_train_backward_run(what, points1, D1, points2, D2, c, idx, dist2, k, params_host, cout_host, eps_host, L, dout, dpoints1,
                                         dpoints2, grads_host, workspace, workspace_bytes, stream);
}
