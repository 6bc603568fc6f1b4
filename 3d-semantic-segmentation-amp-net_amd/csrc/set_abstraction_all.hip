// set_abstraction_all.hip -- set abstraction with ONE group of all n points per cloud (the usual implementation's group_all=True,
// sample_and_group_all), eval mode, and its backward with the running statistics frozen (C ABI: ampnet_sa_all_forward_f32,
// ampnet_sa_all_backward_f32 and their *_workspace_bytes).  Row j of cloud b is [xyz[b, j, 0:3], feats[b, j, :]]: the coordinates as they
// are, no centre.  out[b, c] = max_j relu(bn_eval(...)) over the layers, arg[b, c] = the LOWEST j that attains it.
//
// Forward, kernels on the caller's stream:
//   fold (sa_fold_kernel)      scale and shift, as in ampnet_sa_forward_f32.
//   sa_all_forward_kernel      A wave owns a TILE of 32 consecutive rows of one cloud: it loads them straight into its LDS tile (rows past n
//       repeat the tile's first row, which can neither change a max nor win an argmax), runs layers 0 .. L-2 with the forward's own code
//       (mlp_dispatch<K_PAIRS>) and the last layer's raw accumulator with mlp_accumulate, the loop every backward uses to find the
//       forward's bits again: the epilogue of mlp_run carries ONE float per column, and this one needs the maximum and its row, a
//       SaArgMax per column (sa_tiles.h: the walk within a tile, and the rule that the LOWEST row wins a tie).
//       A cloud's cdiv(n, 32) tiles are dealt to at most SAA_MAX_RUNS RUNS of consecutive tiles; a wave walks the tiles of a run in
//       ascending order and keeps the run's (max, row) per column in ITS row of the workspace, every word read and written by one lane only,
//       again with a strict >.
//   sa_all_reduce_kernel       a thread per (cloud, column) combines the cloud's runs in ascending order with a strict >: the lowest row wins.
// The row results do not depend on a row's place in a tile (each MFMA row is its own fmaf chain, k ascending in the K_PAIRS order), so the
// output is bit for bit what ampnet_sa_forward_f32 gives on the same rows with a centre at the origin, whatever the tiling.  No atomics:
// every order is a function of the shape alone.
//
// Backward.  BatchNorm is a per-row affine map in eval mode, so only the rows that won some column carry any gradient: at most cout_last
// <= 256 distinct rows per cloud, whatever n is.
//   sa_all_compact_kernel      a workgroup per cloud sorts the distinct values of arg[b, :] (clamped to [0, n)) into ascending order and builds a
//       MINI-CLOUD of cout_last + 1 points: the winners' [xyz, feats] rows in that order, zero rows behind them, and one all-zero row LAST,
//       used as the centre of every group (x - 0 is exact).  The winners form K = cout_last / 32 chunks of 32: group_idx'[b, k, t] = 32 k + t
//       while that is a winner, else the chunk's first member (an empty chunk: winner 0).  dout'[b, k, c] = dout[b, c] where arg[b, c]'s
//       winner lies in chunk k, 0 elsewhere.
//   ampnet_sa_backward_f32     on the mini-cloud, unchanged: n_clouds x K groups of nsample = 32.  Inside a chunk the recomputed max of a
//       column whose winner is there is that winner again: its value is the cloud's maximum, the rows are in ascending order of j, so it
//       is the lowest row of the chunk attaining it, and the padding slots repeat an earlier row and lose the tie.  Every other column of
//       the chunk meets dout' = 0.  Padding rows get dz = 0 in every layer and contribute exact zeros to every sum.
//   sa_all_scatter_kernel      dfeats (zero-filled by a memset) [b, winner_i, :] = dfeats'[b, i, :]: the winners are distinct, plain stores.
// After the pass of sa_all_compact_kernel over arg nothing depends on n but the memset of dfeats.
#include "sa_tiles.h"

namespace ampnet {

constexpr int SAA_MAX_RUNS = 256;         // runs of consecutive tiles per cloud (= partial rows per cloud in the workspace)
constexpr int SAA_CHUNK = 32;             // winners per chunk of the backward = nsample of the inner ampnet_sa_backward_f32

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
struct SaAllShape {
    int tiles, runs, items;               // per cloud: 32-row tiles, runs of tiles; items = n_clouds * runs
    size_t off_pmax, off_parg, floats;    // float offsets in the workspace (the fold comes first)
};

// the limits both directions share (`what` opens every message)
static int saa_check(const char *what, int D, int n_clouds, int n, const int *cout_host, int L)
{
    AMPNET_REQUIRE(cout_host, "%s: null pointer", what);
    AMPNET_REQUIRE(n_clouds >= 1 && n >= 1, "%s: bad shape n_clouds=%d n=%d (both must be >= 1)", what, n_clouds, n);
    AMPNET_TRY(sa_check_limits(what, D, n_clouds, n, 0, L, true));
    for (int l = 0; l < L; ++l)
        AMPNET_REQUIRE(cout_host[l] >= 32 && cout_host[l] <= AMPNET_SA_MAX_COUT && cout_host[l] % 32 == 0,
                       "%s: layer %d has cout=%d, must be a multiple of 32 in [32, %d]", what, l, cout_host[l], AMPNET_SA_MAX_COUT);
    return AMPNET_OK;
}

static int saa_shape(const char *what, int D, int n_clouds, int n, const int *cout_host, int L, SaAllShape &sh)
{
    AMPNET_TRY(saa_check(what, D, n_clouds, n, cout_host, L));
    sh = {};
    sh.tiles = cdiv(n, 32);
    sh.runs = sh.tiles < SAA_MAX_RUNS ? sh.tiles : SAA_MAX_RUNS;
    sh.items = n_clouds * sh.runs;                              // <= n_clouds * n
    const size_t part = (size_t)sh.items * cout_host[L - 1];
    sh.off_pmax = align_up((size_t)AMPNET_SA_WORKSPACE_BYTES / sizeof(float), 64);
    sh.off_parg = sh.off_pmax + align_up(part, 64);
    sh.floats = sh.off_parg + align_up(part, 64);
    return AMPNET_OK;
}

// Rows j0 .. j0 + 31 of a cloud into `tile` [32][ldt], kp0 columns each (zeros past cin0); the rows past `rows` repeat row j0.  Element
// e = (row, column) with the columns fastest, so a row's coordinates and features load contiguously.
__device__ __forceinline__ void saa_gather_tile(float *tile, int ldt, int kp0, int cin0, const float *__restrict__ cloud, int ld,
                                                const float *__restrict__ fcloud, int D, int j0, int rows, int lane)
{
    for (int e = lane; e < 32 * kp0; e += 64) {                // (32 kp0 is a multiple of 64: every lane makes the same trips)
        const int t = e / kp0, c = e - t * kp0;
        const int j = j0 + (t < rows ? t : 0);
        float v = 0.0f;
        if (c < 3) v = cloud[(size_t)j * ld + c];
        else if (c < cin0) v = fcloud[(size_t)j * D + (c - 3)];
        tile[t * ldt + c] = v;
    }
}

// The last layer on one 32-row tile: per column the largest relu(y) and the LOWEST row of the tile that attains it, merged into the
// run's partial (pm, pa) -- `first`: this is the run's first tile and the partial is written, not read.  j0: the cloud row of tile row 0.
template <int NT>
__device__ __forceinline__ void saa_last(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int n0,
                                         const float *__restrict__ scale, const float *__restrict__ shift, int j0, bool first, float *pm,
                                         int32_t *pa, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    mlp_accumulate<NT, K_PAIRS, false>(acc, mlp_operand<K_PAIRS>(x, ldx, r, h), w, ldw, k_valid, kp, n0, r, h);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        const float sc = scale[col], sh = shift[col];
        SaArgMax am;
        am.init();
#pragma unroll
        for (int i = 0; i < 16; ++i)                                           // (the rows ascend with i, as SaArgMax asks)
            am.put(acc[t][i], fmaxf(fmaf(acc[t][i], sc, sh), 0.0f), mlp_acc_row(i, h));
        am.merge_halves();
        // rows past n repeat tile row 0 and lose the tie to it; an earlier tile of the run keeps a tie too
        if (h == 0 && (first || am.best > pm[col])) {
            pm[col] = am.best;
            pa[col] = j0 + am.row;
        }
    }
}

// the last layer's cout / 32 column tiles, four at a time, then two, then one (mlp_layer's walk)
__device__ __forceinline__ void saa_last_layer(const float *x, int ldx, const float *w, int ldw, int k_valid, int kp, int cout,
                                               const float *__restrict__ scale, const float *__restrict__ shift, int j0, bool first, float *pm,
                                               int32_t *pa, int lane)
{
    int n0 = 0;
    for (; n0 + 128 <= cout; n0 += 128) saa_last<4>(x, ldx, w, ldw, k_valid, kp, n0, scale, shift, j0, first, pm, pa, lane);
    if (n0 + 64 <= cout) {
        saa_last<2>(x, ldx, w, ldw, k_valid, kp, n0, scale, shift, j0, first, pm, pa, lane);
        n0 += 64;
    }
    if (n0 + 32 <= cout) saa_last<1>(x, ldx, w, ldw, k_valid, kp, n0, scale, shift, j0, first, pm, pa, lane);
}

__global__ __launch_bounds__(256) void sa_all_forward_kernel(MlpPlan p, const float *__restrict__ xyz, int n, int ld,
                                                            const float *__restrict__ feats, int D, const float *__restrict__ fold, int tiles,
                                                            int runs, int items, float *pmax, int32_t *parg)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MlpLds m = mlp_lds(p, 32, s_mem, wave);
    mlp_stage_weights(p, m.s_w, tid, 64 * p.nw);
    __syncthreads();
    const int L = p.L, cin0 = p.cin[0], kp0 = p.kp[0], cout_last = p.cout[L - 1], last = L - 1;
    const float *scale = fold + p.fold_off[last], *shift = scale + cout_last;
    const bool staged = p.w_off[last] >= 0;
    for (int item = blockIdx.x * p.nw + wave; item < items; item += gridDim.x * p.nw) {
        const int cloud_i = item / runs, q = item - cloud_i * runs;
        const int t0 = (int)((long long)q * tiles / runs), t1 = (int)((long long)(q + 1) * tiles / runs);
        const float *cloud = xyz + (size_t)cloud_i * n * ld;
        const float *fcloud = feats ? feats + (size_t)cloud_i * n * D : nullptr;
        float *pm = pmax + (size_t)item * cout_last;
        int32_t *pa = parg + (size_t)item * cout_last;
        for (int t = t0; t < t1; ++t) {
            const int j0 = 32 * t, rows = n - j0 < 32 ? n - j0 : 32;
            saa_gather_tile(m.tile_a, p.ld_a, kp0, cin0, cloud, ld, fcloud, D, j0, rows, lane);
            wave_lds_sync();
            float *x = m.tile_a, *y = m.tile_b;
            int ldx = p.ld_a, ldy = p.ld_b;
            for (int l = 0; l < last; ++l) {
                mlp_dispatch<K_PAIRS>(p, l, 32, m.s_w, x, ldx, fold, MlpToTile{y, ldy}, nullptr, lane);
                wave_lds_sync();
                float *nx = y;
                y = x;
                x = nx;
                const int ldt = ldx;
                ldx = ldy;
                ldy = ldt;
            }
            if (staged)                                        // (two calls: each keeps its weights' address space)
                saa_last_layer(x, ldx, m.s_w + p.w_off[last], p.kp[last] + 1, p.kp[last], p.kp[last], cout_last, scale, shift, j0, t == t0, pm, pa, lane);
            else
                saa_last_layer(x, ldx, p.w[last], p.cin[last], p.cin[last], p.kp[last], cout_last, scale, shift, j0, t == t0, pm, pa, lane);
            // the next tile's gather overwrites tile A: every read of this tile is done (the last layer's results are in registers)
            wave_lds_sync();
        }
    }
}

// a thread per (cloud, column): the cloud's runs in ascending order, strict >
__global__ __launch_bounds__(256) void sa_all_reduce_kernel(const float *__restrict__ pmax, const int32_t *__restrict__ parg, int runs,
                                                           int cout_last, int total, float *__restrict__ out, int32_t *__restrict__ arg_out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int cloud_i = e / cout_last, c = e - cloud_i * cout_last;
    const size_t base = (size_t)cloud_i * runs * cout_last + c;
    float best = pmax[base];
    int32_t brow = parg[base];
    for (int q = 1; q < runs; ++q) {
        const float v = pmax[base + (size_t)q * cout_last];
        if (v > best) {
            best = v;
            brow = parg[base + (size_t)q * cout_last];
        }
    }
    out[e] = best;
    if (arg_out) arg_out[e] = brow;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
struct SaAllBwdShape {
    int C, K, n_mini;                     // cout_last, chunks per cloud, points of a mini-cloud (C + 1: the zero row is last)
    size_t off_wrow, off_xyz, off_feats, off_centres, off_gidx, off_dout, off_dfeats, off_inner, inner_bytes, floats;
};

static int saa_bwd_shape(const char *what, int D, int n_clouds, int n, const int *cout_host, int L, SaAllBwdShape &sh)
{
    AMPNET_TRY(saa_check(what, D, n_clouds, n, cout_host, L));
    sh = {};
    sh.C = cout_host[L - 1];
    sh.K = sh.C / SAA_CHUNK;
    sh.n_mini = sh.C + 1;
    AMPNET_REQUIRE((long long)n_clouds * sh.n_mini <= 0x7fffffffLL, "%s: n_clouds * (cout_last + 1) = %lld mini-cloud rows exceed 2^31 - 1", what,
                   (long long)n_clouds * sh.n_mini);
    sh.inner_bytes = ampnet_sa_backward_workspace_bytes(D, n_clouds, sh.K, SAA_CHUNK, cout_host, L);
    if (!sh.inner_bytes) return AMPNET_E_ARG;                  // (ampnet_last_error is the inner entry point's)
    size_t off = 0;
    auto take = [&off](size_t floats) {
        const size_t at = off;
        off += align_up(floats, 64);
        return at;
    };
    sh.off_wrow = take((size_t)n_clouds * sh.C);
    sh.off_xyz = take((size_t)n_clouds * sh.n_mini * 3);
    sh.off_feats = take((size_t)n_clouds * sh.n_mini * D);
    sh.off_centres = take((size_t)n_clouds * sh.K);
    sh.off_gidx = take((size_t)n_clouds * sh.K * SAA_CHUNK);
    sh.off_dout = take((size_t)n_clouds * sh.K * sh.C);
    sh.off_dfeats = take((size_t)n_clouds * sh.n_mini * D);
    sh.off_inner = off;
    sh.floats = off + align_up(sh.inner_bytes, 256) / sizeof(float);
    return AMPNET_OK;
}

// A workgroup per cloud (256 threads, thread c owns column c < C <= 256): see the file header.
__global__ __launch_bounds__(256) void sa_all_compact_kernel(const float *__restrict__ xyz, int n, int ld, const float *__restrict__ feats, int D,
                                                            const int32_t *__restrict__ arg, const float *__restrict__ dout, int C,
                                                            int32_t *__restrict__ wrow, float *__restrict__ mxyz, float *__restrict__ mfeats,
                                                            int32_t *__restrict__ centres, int32_t *__restrict__ gidx,
                                                            float *__restrict__ dout_k)
{
    __shared__ int s_val[AMPNET_SA_MAX_COUT], s_first[AMPNET_SA_MAX_COUT], s_sorted[AMPNET_SA_MAX_COUT];
    const int b = blockIdx.x, c = threadIdx.x, K = C / SAA_CHUNK, n_mini = C + 1;
    if (c < C) s_val[c] = min(max(arg[(size_t)b * C + c], 0), n - 1);
    __syncthreads();
    if (c < C) {
        int first = 1;
        for (int o = 0; o < c; ++o) first &= s_val[o] != s_val[c];
        s_first[c] = first;
    }
    __syncthreads();
    int rank = 0, nw = 0;                 // rank: distinct winners below mine; nw: distinct winners of the cloud (>= 1)
    for (int o = 0; o < C; ++o) {
        nw += s_first[o];
        if (c < C) rank += s_first[o] && s_val[o] < s_val[c];
    }
    if (c < C && s_first[c]) s_sorted[rank] = s_val[c];
    __syncthreads();
    if (c < C) wrow[(size_t)b * C + c] = c < nw ? s_sorted[c] : -1;
    const float *cloud = xyz + (size_t)b * n * ld;
    float *mx = mxyz + (size_t)b * n_mini * 3;
    for (int e = c; e < n_mini * 3; e += 256) {
        const int i = e / 3, col = e - 3 * i;
        mx[e] = i < nw ? cloud[(size_t)s_sorted[i] * ld + col] : 0.0f;
    }
    if (D) {
        const float *fcloud = feats + (size_t)b * n * D;
        float *mf = mfeats + (size_t)b * n_mini * D;
        for (int e = c; e < n_mini * D; e += 256) {
            const int i = e / D, col = e - D * i;
            mf[e] = i < nw ? fcloud[(size_t)s_sorted[i] * D + col] : 0.0f;
        }
    }
    if (c < K) centres[(size_t)b * K + c] = C;                 // the all-zero row
    for (int e = c; e < K * SAA_CHUNK; e += 256) {
        const int head = e / SAA_CHUNK * SAA_CHUNK;            // the chunk's first member; an empty chunk repeats winner 0
        gidx[(size_t)b * K * SAA_CHUNK + e] = e < nw ? e : head < nw ? head : 0;
    }
    if (c < C) {
        const float g = dout[(size_t)b * C + c];
        for (int k = 0; k < K; ++k) dout_k[((size_t)b * K + k) * C + c] = rank / SAA_CHUNK == k ? g : 0.0f;
    }
}

// a wave per (cloud, winner slot): dfeats[b, winner, :] = dfeats'[b, slot, :]
__global__ __launch_bounds__(64) void sa_all_scatter_kernel(const float *__restrict__ dfeats_mini, const int32_t *__restrict__ wrow, int C, int n,
                                                           int D, float *__restrict__ dfeats)
{
    const int b = blockIdx.x / C, i = blockIdx.x - b * C;
    const int j = wrow[blockIdx.x];
    if (j < 0) return;
    const float *src = dfeats_mini + ((size_t)b * (C + 1) + i) * D;
    float *dst = dfeats + ((size_t)b * n + j) * D;
    for (int col = threadIdx.x; col < D; col += 64) dst[col] = src[col];
}

}  // namespace ampnet

extern "C" size_t ampnet_sa_all_forward_workspace_bytes(int D, int n_clouds, int n, const int *cout_host, int L)
{
    using namespace ampnet;
    SaAllShape sh;
    if (saa_shape("ampnet_sa_all_forward_workspace_bytes", D, n_clouds, n, cout_host, L, sh) != AMPNET_OK) return 0;
    return sh.floats * sizeof(float);
}

extern "C" int ampnet_sa_all_forward_f32(const float *xyz, int n_clouds, int n, int ld, const float *feats, int D,
                                         const float *const *params_host, const int *cout_host, const float *eps_host, int L, float *out,
                                         int32_t *arg_out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_sa_all_forward_f32";
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(xyz && params_host && cout_host && eps_host && out, "%s: null pointer", what);
    AMPNET_REQUIRE(ld >= 3, "%s: bad shape ld=%d (must be >= 3)", what, ld);
    SaAllShape sh;
    AMPNET_TRY(sa_check_feats(what, feats, D, nullptr));
    AMPNET_TRY(saa_shape(what, D, n_clouds, n, cout_host, L, sh));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.floats * sizeof(float)));
    MlpPlan p;
    MlpFold f;
    const int lds = mlp_plan_build(what, 3 + D, 32, params_host, cout_host, eps_host, L, p, f);
    if (!lds) return AMPNET_E_ARG;
    float *ws = static_cast<float *>(workspace);
    float *pmax = ws + sh.off_pmax;
    int32_t *parg = reinterpret_cast<int32_t *>(ws + sh.off_parg);
    static bool attr_set = false;
    AMPNET_TRY(mlp_allow_full_lds(what, reinterpret_cast<const void *>(sa_all_forward_kernel), attr_set));
    AMPNET_TRY(mlp_fold_launch(p, f, ws, st));
    hipLaunchKernelGGL(sa_all_forward_kernel, dim3(mlp_grid(sh.items, p.nw)), dim3(64 * p.nw), lds, st, p, xyz, n, ld, feats, D, ws, sh.tiles,
                       sh.runs, sh.items, pmax, parg);
    AMPNET_TRY(check_launch("sa_all_forward_kernel"));
    const int total = n_clouds * p.cout[L - 1];
    hipLaunchKernelGGL(sa_all_reduce_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, pmax, parg, sh.runs, p.cout[L - 1], total, out, arg_out);
    return check_launch("sa_all_reduce_kernel");
}

extern "C" size_t ampnet_sa_all_backward_workspace_bytes(int D, int n_clouds, int n, const int *cout_host, int L)
{
    using namespace ampnet;
    SaAllBwdShape sh;
    if (saa_bwd_shape("ampnet_sa_all_backward_workspace_bytes", D, n_clouds, n, cout_host, L, sh) != AMPNET_OK) return 0;
    return sh.floats * sizeof(float);
}

extern "C" int ampnet_sa_all_backward_f32(const float *xyz, int n_clouds, int n, int ld, const float *feats, int D,
                                          const float *const *params_host, const int *cout_host, const float *eps_host, int L,
                                          const int32_t *arg, const float *dout, float *dfeats, float *const *grads_host, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_sa_all_backward_f32";
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(xyz && params_host && cout_host && eps_host && arg && dout && grads_host, "%s: null pointer", what);
    AMPNET_REQUIRE(ld >= 3, "%s: bad shape ld=%d (must be >= 3)", what, ld);
    SaAllBwdShape sh;
    AMPNET_TRY(sa_check_feats(what, feats, D, dfeats));
    AMPNET_TRY(saa_bwd_shape(what, D, n_clouds, n, cout_host, L, sh));
    AMPNET_TRY(sa_check_tables(what, params_host, grads_host, L));
    AMPNET_TRY(sa_check_workspace(what, workspace, workspace_bytes, sh.floats * sizeof(float)));
    float *ws = static_cast<float *>(workspace);
    int32_t *wrow = reinterpret_cast<int32_t *>(ws + sh.off_wrow), *centres = reinterpret_cast<int32_t *>(ws + sh.off_centres);
    int32_t *gidx = reinterpret_cast<int32_t *>(ws + sh.off_gidx);
    float *mxyz = ws + sh.off_xyz, *mfeats = D ? ws + sh.off_feats : nullptr, *dout_k = ws + sh.off_dout;
    float *dfeats_mini = dfeats ? ws + sh.off_dfeats : nullptr;
    hipLaunchKernelGGL(sa_all_compact_kernel, dim3(n_clouds), dim3(256), 0, st, xyz, n, ld, feats, D, arg, dout, sh.C, wrow, mxyz, mfeats, centres,
                       gidx, dout_k);
    AMPNET_TRY(check_launch("sa_all_compact_kernel"));
    const int rc = ampnet_sa_backward_f32(mxyz, n_clouds, sh.n_mini, 3, centres, sh.K, gidx, SAA_CHUNK, mfeats, D, params_host, cout_host, eps_host, L, dout_k,
                                          dfeats_mini, grads_host, nullptr, ws + sh.off_inner, sh.inner_bytes, stream);
    if (rc != AMPNET_OK || !dfeats) return rc;
    if (hipMemsetAsync(dfeats, 0, (size_t)n_clouds * n * D * sizeof(float), st) != hipSuccess)
        return fail(AMPNET_E_LAUNCH, "%s: memset of dfeats failed", what);
    hipLaunchKernelGGL(sa_all_scatter_kernel, dim3(n_clouds * sh.C), dim3(64), 0, st, dfeats_mini, wrow, sh.C, n, D, dfeats);
    return check_launch("sa_all_scatter_kernel");
}
