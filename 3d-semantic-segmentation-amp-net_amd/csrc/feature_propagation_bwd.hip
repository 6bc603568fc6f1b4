// feature_propagation_bwd.hip -- the backward of one fused feature-propagation layer with BatchNorm's running statistics frozen (C ABI:
// ampnet_fp_backward_f32, ampnet_fp_backward_workspace_bytes).  Per layer, with a = W x the raw accumulator, scale = gamma / sqrt(var + eps)
// and y = fma(a, scale, shift) as in the forward:
//     dy = dx_l [y > 0],  dbeta = sum_rows dy,  G = sum_rows dy a,  dgamma = (G + (b - mean) dbeta) / sqrt(var + eps),
//     dz = dy scale,  dbias = scale dbeta,  dW = dz^T x_{l-1},  dx_{l-1} = dz W.
// The forward keeps nothing, so everything is recomputed.  Five kernels on the caller's stream:
//
//   fold (sa_fold_kernel)   scale and shift, as in the forward.
//   fp_backward_kernel      A workgroup is ONE wave and a wave owns 32 consecutive fine points of one cloud, as in the forward.  It rebuilds
//       their rows with the forward's row builder (fp_rows.h) into tile X_0, runs layers 0 .. L-2 forward with the forward's own code
//       (mlp_dispatch<K_QUADS>, weights read through L2) into tiles X_1 .. X_{L-1}, and keeps ALL of them: a tile per layer input instead
//       of the forward's ping-pong.  Then it walks the layers backward.  Layer l: the accumulators a of the layer are computed AGAIN from
//       X_l in the forward's contraction order (K_QUADS: the same bits, so the same ReLU mask), dx_l -- `dout` from global memory for the
//       last layer, tile X_{l+1} otherwise -- becomes dz in place in X_{l+1} (the same element, the same lane), and dx_{l-1} = dz W
//       overwrites X_l, whose activations nobody needs any more.  So L + 1 tiles of widths kp_0, cout_0 .. cout_{L-1}: 115 KB for
//       fp3 of pointnet_2 (384 -> 256 -> 256).  The one shape family of the forward's limits that this exceeds (cin_0 > 504 with three
//       layers of 256) builds X_0 in the space of X_2 and X_3 and REBUILDS it there before layer 0's backward.
//       Why the layer's GEMM is run a second time instead of keeping a: a tile of a per layer would double the LDS, and a cannot be had
//       back from y when scale = 0.  Why mlp_tiles is not reused for it: its epilogue is handed relu(y) only; its K loop is fused_mlp.h's
//       mlp_accumulate, whose raw accumulator goes to the backward's epilogue (fpb_recompute).
//       dx = dz W is the forward's lane map with cin and cout exchanged: lane (r, h) supplies row r of dz and COLUMN c0 + r of W, read along
//       W's rows through L2 (128 contiguous bytes per half wave and k); the contraction runs over o ascending in blocks of 8, k-step
//       i < 4 of lane half h taking o = o0 + 2 i + h, one fmaf chain per output element.
//       dx_0's columns [0, D1) are stored straight to dpoints1, columns [D1, cin_0) to the workspace for the scatter below.
//       The wave also stores x_l and dz_l of its rows to the workspace (dW below) and adds its tiles' per-channel sums of dy and dy a
//       (rows in the accumulator's order, lane half 0 before half 1, tiles in ascending order) into ITS OWN row of a partials array in
//       global memory: every element is read and written by the same lane only.
//   fp_wgrad_kernel, fp_wgrad_reduce_kernel   dW_l = dz_l^T x_l as a split-K MFMA GEMM over the rows (mlp_bwd.hip, shared with the
//       set-abstraction backward): the chunks' partials are added in ascending chunk order.
//   fp_scatter_kernel       dpoints2 as a GATHER: one wave per coarse point j scans its cloud's n k neighbour entries in ascending order, 64
//       at a time, takes the entries equal to j by ballot and adds w_k dx_0[i, D1:] in ascending (i, k) order, a lane per column.  The
//       weights are the forward's (fp_interp_weights).  No float atomics; a coarse point nobody picked gets zeros.
//   fp_bwd_finalize_kernel  adds the workgroups' partials in a fixed order (a wave per channel) and derives dbeta, dgamma and dbias
//       (mlp_bwd.hip).
//
// Every order above is a function of the shape alone: two runs give the same bits.  Exact fp32 MFMA whatever the matrix precision is.
#include "fp_bwd_tiles.h"

namespace ampnet {

struct FpBwdPlan {
    int off_x[MLP_MAX_LAYERS + 1], ld_x[MLP_MAX_LAYERS + 1];   // tile X_l: float offset in LDS, odd row stride
    int rebuild;                                               // X_0 shares the space of X_2, X_3 and is built twice
    int ldxs[MLP_MAX_LAYERS];                                  // row stride of x_l in the workspace: cin_l rounded up to 32 (zeros)
    int sum_c;                                                 // sum of cout_l; layer l's channels start at fold_off[l] / 2
    float *xs[MLP_MAX_LAYERS], *dz[MLP_MAX_LAYERS], *dx0, *parts;
};

__global__ __launch_bounds__(64) void fp_backward_kernel(MlpPlan p, FpBwdPlan b, const float *__restrict__ points1, int D1,
                                                        const float *__restrict__ points2, int D2, int n, int s,
                                                        const int32_t *__restrict__ idx, const float *__restrict__ dist2, int k,
                                                        const float *__restrict__ fold, const float *__restrict__ dout, int tiles_per_cloud,
                                                        int n_tiles, float *__restrict__ dpoints1)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int lane = threadIdx.x;
    const int L = p.L;
    float *part_b = b.parts + (size_t)blockIdx.x * 2 * b.sum_c, *part_g = part_b + b.sum_c;
    if (lane < 32)
        for (int c = lane; c < b.sum_c; c += 32) part_b[c] = part_g[c] = 0.0f;       // channel c belongs to lane c % 32, here and below
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int cloud_i = tile / tiles_per_cloud, row0 = (tile - cloud_i * tiles_per_cloud) * 32;
        const int rows = min(32, n - row0);
        const size_t grow = (size_t)cloud_i * n + row0;
        float *x0 = s_mem + b.off_x[0];
        fp_build_rows(x0, b.ld_x[0], p.kp[0], points1, D1, points2, D2, n, s, idx, dist2, k, cloud_i, row0, rows, lane);
        wave_lds_sync();
        fpb_store_rows(x0, b.ld_x[0], p.kp[0], b.xs[0] + grow * b.ldxs[0], b.ldxs[0], rows, lane);
        for (int l = 0; l + 1 < L; ++l) {
            float *y = s_mem + b.off_x[l + 1];
            mlp_dispatch<K_QUADS>(p, l, 32, s_mem, s_mem + b.off_x[l], b.ld_x[l], fold, MlpToTile{y, b.ld_x[l + 1]}, nullptr, lane);
            wave_lds_sync();
            fpb_store_rows(y, b.ld_x[l + 1], p.cout[l], b.xs[l + 1] + grow * b.ldxs[l + 1], b.ldxs[l + 1], rows, lane);
        }
        for (int l = L - 1; l >= 0; --l) {
            float *x = s_mem + b.off_x[l], *d = s_mem + b.off_x[l + 1];
            const int ldx = b.ld_x[l], ldd = b.ld_x[l + 1], cin = p.cin[l], cout = p.cout[l], ch = p.fold_off[l] / 2;
            if (l == 0 && b.rebuild) {
                wave_lds_sync();                  // the reads of X_2 (dx = dz W of layer 1) are done
                fp_build_rows(x, ldx, p.kp[0], points1, D1, points2, D2, n, s, idx, dist2, k, cloud_i, row0, rows, lane);
                wave_lds_sync();
            }
            const float *scale = fold + p.fold_off[l], *shift = scale + cout;
            const float *dsrc = l == L - 1 ? dout + grow * cout : nullptr;
            float *dz_ws = b.dz[l] + grow * cout;
            int n0 = 0;
            if (p.w_vec[l]) {
                for (; n0 + 128 <= cout; n0 += 128)
                    fpb_recompute<4, true>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, dsrc, rows, dz_ws, part_b + ch, part_g + ch, lane);
                for (; n0 < cout; n0 += 32)
                    fpb_recompute<1, true>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, dsrc, rows, dz_ws, part_b + ch, part_g + ch, lane);
            } else {
                for (; n0 + 128 <= cout; n0 += 128)
                    fpb_recompute<4, false>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, dsrc, rows, dz_ws, part_b + ch, part_g + ch, lane);
                for (; n0 < cout; n0 += 32)
                    fpb_recompute<1, false>(x, ldx, p.w[l], cin, p.kp[l], cout, n0, scale, shift, d, ldd, dsrc, rows, dz_ws, part_b + ch, part_g + ch, lane);
            }
            wave_lds_sync();
            float *xo = l ? x : nullptr;
            float *dp1 = dpoints1 ? dpoints1 + grow * D1 : nullptr, *dx0 = b.dx0 + grow * D2;
            int c0 = 0;
            for (; c0 + 128 <= cin; c0 += 128) mlp_dgrad<4>(d, ldd, p.w[l], cin, cout, c0, xo, ldx, dp1, D1, dx0, D2, rows, lane);
            for (; c0 < cin; c0 += 32) mlp_dgrad<1>(d, ldd, p.w[l], cin, cout, c0, xo, ldx, dp1, D1, dx0, D2, rows, lane);
            wave_lds_sync();
        }
    }
}

__global__ __launch_bounds__(64) void fp_scatter_kernel(const float *__restrict__ dx0, int D2, int n, int s, const int32_t *__restrict__ idx,
                                                       const float *__restrict__ dist2, int k, float *__restrict__ dpoints2)
{
    const int lane = threadIdx.x;
    const int cloud_i = blockIdx.x / s, j = blockIdx.x - cloud_i * s;
    const long long total = (long long)n * k;
    const int32_t *ic = idx + (size_t)cloud_i * total;
    const float *dc = dist2 + (size_t)cloud_i * total, *gx = dx0 + (size_t)cloud_i * n * D2;
    float acc[AMPNET_FP_MAX_CIN / 64];
#pragma unroll
    for (int u = 0; u < AMPNET_FP_MAX_CIN / 64; ++u) acc[u] = 0.0f;
    for (long long e0 = 0; e0 < total; e0 += 64) {
        const long long e = e0 + lane;
        const bool hit = e < total && min(max(ic[e], 0), s - 1) == j;
        int i = 0;
        float w = 0.0f;
        if (hit) {
            i = (int)(e / k);
            const int q = (int)(e - (long long)i * k);
            float wk[3];
            fp_interp_weights(dc + (size_t)i * k, k, wk);
            w = q == 0 ? wk[0] : q == 1 ? wk[1] : wk[2];
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {                            // wave-uniform: every lane walks the hits in ascending entry order
            const int src = __ffsll(mask) - 1;
            mask &= mask - 1;
            const int ib = __shfl(i, src);
            const float wb = __shfl(w, src);
            const float *row = gx + (size_t)ib * D2;
#pragma unroll
            for (int u = 0; u < AMPNET_FP_MAX_CIN / 64; ++u)
                if (lane + 64 * u < D2) acc[u] = fmaf(wb, row[lane + 64 * u], acc[u]);
        }
    }
    float *dst = dpoints2 + (size_t)blockIdx.x * D2;
#pragma unroll
    for (int u = 0; u < AMPNET_FP_MAX_CIN / 64; ++u)
        if (lane + 64 * u < D2) dst[lane + 64 * u] = acc[u];
}

int fp_scatter_launch(const float *dx0, int D2, int n_clouds, int n, int s, const int32_t *idx, const float *dist2, int k, float *dpoints2,
                      hipStream_t st)
{
    hipLaunchKernelGGL(fp_scatter_kernel, dim3(n_clouds * s), dim3(64), 0, st, dx0, D2, n, s, idx, dist2, k, dpoints2);
    return check_launch("fp_scatter_kernel");
}

// fp_scatter_kernel for fine clouds of UNEQUAL size packed back to back (ampnet_fp_backward_ragged_f32): one wave per coarse point; global
// coarse point j = blockIdx.x belongs to cloud b = j / s and scans the neighbour entries of that cloud's fine rows
// [cloud_off[b], cloud_off[b + 1]) alone, not those of the whole array.  idx holds GLOBAL coarse indices and is clamped into the cloud's own
// range [b s, (b + 1) s - 1]; dx0's rows and dist2 are addressed by the global fine row.  The hits are walked in ascending (i, k) order with
// fp_scatter_kernel's own statements, so cloud by cloud the result is what that kernel writes for the cloud alone, bit for bit (where a
// 64-entry step begins does not enter the order).  The table's rows are clamped into [0, total]: a wrong table cannot read past the arrays.
__global__ __launch_bounds__(64) void fp_scatter_ragged_kernel(const float *__restrict__ dx0, int D2, const int32_t *__restrict__ cloud_off,
                                                              int total, int s, const int32_t *__restrict__ idx,
                                                              const float *__restrict__ dist2, int k, float *__restrict__ dpoints2)
{
    const int lane = threadIdx.x;
    const int cloud_i = blockIdx.x / s, j = blockIdx.x;
    const int lo = cloud_i * s, hi = lo + s - 1;
    const int row0 = min(max(cloud_off[cloud_i], 0), total), row1 = min(max(cloud_off[cloud_i + 1], row0), total);
    const long long e_end = (long long)row1 * k;
    float acc[AMPNET_FP_MAX_CIN / 64];
#pragma unroll
    for (int u = 0; u < AMPNET_FP_MAX_CIN / 64; ++u) acc[u] = 0.0f;
    for (long long e0 = (long long)row0 * k; e0 < e_end; e0 += 64) {
        const long long e = e0 + lane;
        const bool hit = e < e_end && min(max(idx[e], lo), hi) == j;
        int i = 0;
        float w = 0.0f;
        if (hit) {
            i = (int)(e / k);
            const int q = (int)(e - (long long)i * k);
            float wk[3];
            fp_interp_weights(dist2 + (size_t)i * k, k, wk);
            w = q == 0 ? wk[0] : q == 1 ? wk[1] : wk[2];
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {                            // wave-uniform: every lane walks the hits in ascending entry order
            const int src = __ffsll(mask) - 1;
            mask &= mask - 1;
            const int ib = __shfl(i, src);
            const float wb = __shfl(w, src);
            const float *row = dx0 + (size_t)ib * D2;
#pragma unroll
            for (int u = 0; u < AMPNET_FP_MAX_CIN / 64; ++u)
                if (lane + 64 * u < D2) acc[u] = fmaf(wb, row[lane + 64 * u], acc[u]);
        }
    }
    float *dst = dpoints2 + (size_t)blockIdx.x * D2;
#pragma unroll
    for (int u = 0; u < AMPNET_FP_MAX_CIN / 64; ++u)
        if (lane + 64 * u < D2) dst[lane + 64 * u] = acc[u];
}

int fp_gather_launch(const float *dx0, int D2, const BwdClouds &c, const int32_t *idx, const float *dist2, int k, float *dpoints2, hipStream_t st)
{
    if (!c.cloud_off) return fp_scatter_launch(dx0, D2, c.n_clouds, c.n, c.s, idx, dist2, k, dpoints2, st);
    hipLaunchKernelGGL(fp_scatter_ragged_kernel, dim3(c.q * c.s_cloud), dim3(64), 0, st, dx0, D2, c.cloud_off, c.n, c.s_cloud, idx, dist2, k,
                       dpoints2);
    return check_launch("fp_scatter_ragged_kernel");
}

int fpb_shape(const char *what, int D1, int D2, int n_clouds, int n, const int *cout_host, int L, FpBwdShape &sh)
{
    AMPNET_REQUIRE(cout_host, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1, "%s: bad shape n_clouds=%d n=%d", what, n_clouds, n);
    AMPNET_REQUIRE(L >= 1 && L <= AMPNET_FP_MAX_LAYERS, "%s: L=%d layers, the kernel is built for 1 .. %d", what, L, AMPNET_FP_MAX_LAYERS);
    AMPNET_REQUIRE(D1 >= 0 && D2 >= 1 && D1 <= AMPNET_FP_MAX_CIN && D2 <= AMPNET_FP_MAX_CIN && D1 + D2 <= AMPNET_FP_MAX_CIN,
                   "%s: cin_0 = D1 + D2 = %d + %d must be in [1, %d] with D2 >= 1", what, D1, D2, AMPNET_FP_MAX_CIN);
    sh = {};
    sh.tiles_per_cloud = (int)(((long long)n + 31) / 32);
    AMPNET_REQUIRE((long long)n_clouds * sh.tiles_per_cloud <= 0x7fff0000LL, "%s: n_clouds * ceil(n / 32) = %lld tiles exceed %lld", what,
                   (long long)n_clouds * sh.tiles_per_cloud, 0x7fff0000LL);
    sh.M = (long long)n_clouds * n;
    sh.n_tiles = n_clouds * sh.tiles_per_cloud;
    sh.grid = sh.n_tiles < FPB_MAX_GRID ? sh.n_tiles : FPB_MAX_GRID;
    fpb_chunk_rule(sh.M, sh.chunk_rows, sh.chunks);
    return mlp_bwd_layout(what, align_up((size_t)AMPNET_FP_WORKSPACE_BYTES / sizeof(float), 64), D1 + D2, D2, sh.M, sh.grid, sh.chunks, cout_host, L,
                          sh);
}

}  // namespace ampnet

extern "C" size_t ampnet_fp_backward_workspace_bytes(int D1, int D2, int n_clouds, int n, const int *cout_host, int L)
{
    using namespace ampnet;
    FpBwdShape sh;
    if (fpb_shape("ampnet_fp_backward_workspace_bytes", D1, D2, n_clouds, n, cout_host, L, sh) != AMPNET_OK) return 0;
    return sh.floats * sizeof(float);
}

namespace ampnet {

// The body of ampnet_fp_backward_f32 and ampnet_fp_backward_ragged_f32: every phase runs on c's (n_clouds, n, s) -- the packed array as ONE
// cloud for the ragged entry point -- and the dpoints2 gather alone looks at c.cloud_off (fp_gather_launch).
static int fp_backward_run(const char *what, const float *points1, int D1, const float *points2, int D2, const BwdClouds &c, const int32_t *idx,
                           const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                           const float *dout, float *dpoints1, float *dpoints2, float *const *grads_host, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    const int n_clouds = c.n_clouds, n = c.n, s = c.s;
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(points2 && idx && dist2 && params_host && cout_host && eps_host && dout && dpoints2 && grads_host, "%s: null pointer", what);
    AMPNET_REQUIRE(s >= 1, "%s: bad shape s=%d", what, s);
    AMPNET_REQUIRE(k >= 1 && k <= 3 && k <= s, "%s: k=%d must be 1, 2 or 3 and <= s=%d", what, k, s);
    AMPNET_REQUIRE(D1 >= 0 && (D1 == 0) == (points1 == nullptr), "%s: points1 must be NULL exactly when D1 = 0 (D1=%d)", what, D1);
    AMPNET_REQUIRE((D1 == 0) == (dpoints1 == nullptr), "%s: dpoints1 must be NULL exactly when D1 = 0 (D1=%d)", what, D1);
    FpBwdShape sh;
    int rc = fpb_shape(what, D1, D2, n_clouds, n, cout_host, L, sh);
    if (rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE((long long)n_clouds * s <= 0x7fffffffLL, "%s: n_clouds * s = %lld coarse points exceed 2^31 - 1", what, (long long)n_clouds * s);
    for (int q = 0; q < 4 * L; ++q) AMPNET_REQUIRE(grads_host[q], "%s: null gradient pointer %d of layer %d", what, q % 4, q / 4);
    AMPNET_REQUIRE(workspace && workspace_bytes >= sh.floats * sizeof(float), "%s: workspace of %zu bytes, need %zu", what, workspace_bytes,
                   sh.floats * sizeof(float));
    MlpPlan p;
    MlpFold f;
    if (!mlp_plan_build(what, D1 + D2, 32, params_host, cout_host, eps_host, L, p, f)) return AMPNET_E_ARG;
    mlp_plan_unstaged(p);
    // the tiles X_0 .. X_L
    FpBwdPlan b = {};
    int floats = 0;
    for (int l = 0; l <= L; ++l) {
        b.ld_x[l] = (l ? p.cout[l - 1] : p.kp[0]) + 1;
        b.off_x[l] = floats;
        floats += 32 * b.ld_x[l];
    }
    if ((size_t)floats * sizeof(float) > (size_t)MLP_LDS_BYTES && L == 3 && b.ld_x[0] <= b.ld_x[2] + b.ld_x[3]) {
        b.rebuild = 1;
        floats -= 32 * b.ld_x[0];
        for (int l = 1; l <= L; ++l) b.off_x[l] -= 32 * b.ld_x[0];
        b.off_x[0] = b.off_x[2];
    }
    AMPNET_REQUIRE((size_t)floats * sizeof(float) <= (size_t)MLP_LDS_BYTES, "%s: a wave's tiles (%zu bytes) exceed the LDS", what,
                   (size_t)floats * sizeof(float));
    float *ws = static_cast<float *>(workspace);
    b.sum_c = sh.sum_c;
    b.parts = ws + sh.off_parts;
    b.dx0 = ws + sh.off_dx0;
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
    rc = mlp_allow_full_lds(what, reinterpret_cast<const void *>(fp_backward_kernel), attr_set);
    if (rc != AMPNET_OK) return rc;
    rc = mlp_fold_launch(p, f, ws, st);
    if (rc != AMPNET_OK) return rc;
    hipLaunchKernelGGL(fp_backward_kernel, dim3(sh.grid), dim3(64), floats * sizeof(float), st, p, b, points1, D1, points2, D2, n, s, idx, dist2,
                       k, ws, dout, sh.tiles_per_cloud, sh.n_tiles, dpoints1);
    rc = check_launch("fp_backward_kernel");
    if (rc != AMPNET_OK) return rc;
    float *wpart = ws + sh.off_wpart;
    for (int l = 0; l < L; ++l) {
        rc = fpb_wgrad_launch(b.dz[l], p.cout[l], b.xs[l], p.cin[l], sh.ldxs[l], sh.M, sh.chunk_rows, sh.chunks, wpart, grads_host[4 * l], st);
        if (rc != AMPNET_OK) return rc;
    }
    rc = fp_gather_launch(b.dx0, D2, c, idx, dist2, k, dpoints2, st);
    if (rc != AMPNET_OK) return rc;
    return fpb_finalize_launch(p, f, g, ws, b.parts, sh.grid, sh.sum_c, st);
}

}  // namespace ampnet

extern "C" int ampnet_fp_backward_f32(const float *points1, int D1, const float *points2, int D2, int n_clouds, int n, int s, const int32_t *idx,
                                      const float *dist2, int k, const float *const *params_host, const int *cout_host, const float *eps_host,
                                      int L, const float *dout, float *dpoints1, float *dpoints2, float *const *grads_host, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    const ampnet::BwdClouds c = {n_clouds, n, s, nullptr, 0, 0};
    return ampnet::fp_backward_run("ampnet_fp_backward_f32", points1, D1, points2, D2, c, idx, dist2, k, params_host, cout_host, eps_host, L, dout,
                                   dpoints1, dpoints2, grads_host, workspace, workspace_bytes, stream);
}

extern "C" int ampnet_fp_backward_ragged_f32(const float *points1, int D1, const float *points2, int D2, const int32_t *cloud_off, int n_clouds,
                                             int total, int s, const int32_t *idx, const float *dist2, int k, const float *const *params_host,
                                             const int *cout_host, const float *eps_host, int L, const float *dout, float *dpoints1,
                                             float *dpoints2, float *const *grads_host, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "ampnet_fp_backward_ragged_f32";
    ampnet::BwdClouds c;
    int rc = ampnet::bwd_clouds_ragged(what, cloud_off, n_clouds, total, s, c);
    if (rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE(k <= s, "%s: k=%d must be <= s=%d, the coarse points of ONE cloud", what, k, s);
    return ampnet::fp_backward_run(what, points1, D1, points2, D2, c, idx, dist2, k, params_host, cout_host, eps_host, L, dout, dpoints1, dpoints2,
                                   grads_host, workspace, workspace_bytes, stream);
}
