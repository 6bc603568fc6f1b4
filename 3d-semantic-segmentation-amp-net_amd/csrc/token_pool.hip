// token_pool.hip -- the window token of pointnet_2: one linear layer and a segmented max over clouds of unequal size, fused, and its
// backward (C ABI: ampnet_token_pool_forward_f32, ampnet_token_pool_backward_f32 and their *_workspace_bytes).
//   out[q, c] = max_r (W[c, :] . rows[r, :] + bias[c])  over the rows r of cloud q = rows cloud_off[q] .. cloud_off[q + 1] of `rows`,
//   arg[q, c] = the LOWEST row, counted inside cloud q, whose float32 value attains it (the rule of ampnet_sa_all_forward_f32).
// No BatchNorm, no ReLU: a maximum below zero stays below zero.  Exact fp32 (v_mfma_f32_32x32x2_f32): the matrix-precision scope is never
// consulted.  Non-finite inputs are out of contract.
//
// THE VALUE OF A ROW.  y[r, c] = acc + bias[c] (one float32 add), acc the MFMA accumulator chain of fused_mlp.h in the K_QUADS order:
// acc starts at 0 and takes the products x[k] * W[c, k] one fmaf-like MFMA step at a time with k in the order, per block of 8 from k0 = 0
// upwards, k0 + 0, k0 + 4, k0 + 1, k0 + 5, k0 + 2, k0 + 6, k0 + 3, k0 + 7 (k-step i of lane half h takes k = k0 + 4 h + i; the hardware
// adds the two halves of a step in the order h = 0, 1).  It is a function of the row's cin numbers and the weights alone: every MFMA row
// is its own chain, so the value does not depend on the row's place in its tile, on its cloud, on the launch, or on whether the weights
// were staged in LDS.  The tie rule and the ragged contract rest on this.
//
// Forward, kernels on the caller's stream:
//   tp_tile_scan_kernel   tile_off[q] = sum over p < q of cdiv(n_p, 32): a cloud of n rows owns cdiv(n, 32) TILES of 32 consecutive rows of
//       its own -- a tile never mixes two clouds -- and T = tile_off[Q] tiles exist in all.  One workgroup.
//   tp_forward_kernel     The tiles, in their global order, are cut into ITEMS of G consecutive tiles (G a function of Q and total alone,
//       tp_shape).  A wave takes an item, finds the cloud of its first tile by a wave-uniform bisection of tile_off (cloud_input_kernel's
//       search) and walks the item's tiles in ascending order, cloud after cloud.  A tile goes through a lane's registers into the wave's LDS
//       tile -- the NEXT tile's loads are issued before this tile's MFMAs and fly during them -- (rows past n
//       repeat the tile's first row: they can neither change a max nor win an argmax), is multiplied by the weights -- staged in LDS once per
//       workgroup when they fit beside the waves' tiles, else read through L2 with one 16-byte load per lane and block -- and its (max,
//       row) per column is merged with a strict > into the partial of the RUN, the item's tiles of one cloud.  A run that is the whole
//       cloud writes out and arg_out itself.  Any other run keeps its partial in the workspace; an item holds at most two of those, its
//       first run (the cloud began in an earlier item: slot 2 item) and its last (the cloud goes on in the next item: slot 2 item + 1).
//       Every word of a partial is read and written by one lane only.
//   tp_reduce_kernel      a thread per (cloud, column) of the clouds that span several items: the cloud's runs in ascending order with a
//       strict >, so the lowest row wins.
// Many clouds of few rows fill the items with whole clouds, a few clouds of many rows are cut into many runs: the waves stay busy either
// way.  No atomics; every order is a function of the shape alone, so two calls return the same bits.
//
// Backward, given arg (clamped into its cloud).  fp32 accumulators, fmaf chains from 0 in the stated orders; no atomics.
//   dx        a memset, then tp_dx_kernel: a workgroup per cloud, thread k owns column k.  For every distinct winner r of the cloud,
//             dx[r, k] = sum over the channels c with arg[q, c] = r, ascending c, of dout[q, c] * W[c, k].
//   dW, db    tp_dw_kernel: a thread per (c, k): dW[c, k] = sum over q ascending of dout[q, c] * rows[cloud q's row arg[q, c], k];
//             the thread of k = 0 also sums db[c] = sum over q ascending of dout[q, c] (plain adds).
// Apart from the memset the work is O(Q cout cin) whatever `total` is.
#include "fused_mlp.h"

namespace ampnet {

constexpr int TP_MIN = 32, TP_MAX = 256;      // cin and cout: multiples of 32 in this range
constexpr int TP_WAVES = 4;                   // waves per workgroup of the forward
constexpr int TP_ITEMS = 4096;                // the items the tiles are cut into, about: 4 per wave of a full grid
constexpr int TP_SCAN_THREADS = 1024;

struct TpShape {
    int G, items;                             // tiles per item; items (an upper bound: the device knows T)
    int staged, lds;                          // weights in LDS; dynamic LDS bytes
    int grid;                                 // workgroups of the forward
    size_t off_pmax, off_parg, off_arg, words;  // 4-byte word offsets in the workspace (tile_off [Q + 1] comes first)
};

static int tp_check(const char *what, int cin, int cout, int Q, long long total)
{
    AMPNET_REQUIRE(cin >= TP_MIN && cin <= TP_MAX && cin % 32 == 0, "%s: cin=%d, must be a multiple of 32 in [%d, %d]", what, cin, TP_MIN, TP_MAX);
    AMPNET_REQUIRE(cout >= TP_MIN && cout <= TP_MAX && cout % 32 == 0, "%s: cout=%d, must be a multiple of 32 in [%d, %d]", what, cout, TP_MIN,
                   TP_MAX);
    AMPNET_REQUIRE(Q >= 1 && total >= Q && total <= 0x7fffffffLL, "%s: bad shape Q=%d clouds, total=%lld rows (every cloud holds a row, total < 2^31)",
                   what, Q, total);
    AMPNET_REQUIRE((long long)Q * cout <= 0x7fffffffLL, "%s: Q * cout = %lld outputs exceed 2^31 - 1", what, (long long)Q * cout);
    return AMPNET_OK;
}

static int tp_shape(const char *what, int cin, int cout, int Q, long long total, TpShape &sh)
{
    AMPNET_TRY(tp_check(what, cin, cout, Q, total));
    sh = {};
    const long long t_max = (total + 31LL * Q) / 32;                         // >= T = sum of cdiv(n_q, 32)
    sh.G = (int)((t_max + TP_ITEMS - 1) / TP_ITEMS);
    sh.items = (int)((t_max + sh.G - 1) / sh.G);
    const int ld = cin + 1;
    const size_t tiles = (size_t)TP_WAVES * 32 * ld * sizeof(float), weights = (size_t)cout * ld * sizeof(float);
    sh.staged = tiles + weights <= (size_t)MLP_LDS_BYTES;
    sh.lds = (int)(tiles + (sh.staged ? weights : 0));
    const size_t part = (size_t)2 * sh.items * cout;
    sh.off_pmax = align_up((size_t)Q + 1, 64);
    sh.off_parg = sh.off_pmax + align_up(part, 64);
    sh.off_arg = sh.off_parg + align_up(part, 64);                           // the whole clouds' rows when the caller wants no arg_out
    sh.words = sh.off_arg + align_up((size_t)Q * cout, 64);
    // every workgroup stages the weights once: as many workgroups as 256 CUs hold at this LDS size, each wave walking several items
    const int resident = 256 * (MLP_LDS_BYTES / sh.lds > 4 ? 4 : MLP_LDS_BYTES / sh.lds);
    sh.grid = cdiv(sh.items, TP_WAVES) < resident ? cdiv(sh.items, TP_WAVES) : resident;
    return AMPNET_OK;
}

// tile_off[q] = tiles of the clouds before q, q <= Q.  One workgroup: a thread sums a stretch of clouds, the stretches are scanned in LDS.
__global__ __launch_bounds__(TP_SCAN_THREADS) void tp_tile_scan_kernel(const int32_t *__restrict__ cloud_off, int Q, int32_t *__restrict__ tile_off)
{
    __shared__ int s_sum[TP_SCAN_THREADS];
    const int tid = threadIdx.x, per = (Q + TP_SCAN_THREADS - 1) / TP_SCAN_THREADS;
    const int q0 = min((long long)tid * per, (long long)Q), q1 = min((long long)q0 + per, (long long)Q);
    int sum = 0;
    for (int q = q0; q < q1; ++q) sum += (cloud_off[q + 1] - cloud_off[q] + 31) >> 5;
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < TP_SCAN_THREADS; ++i) {
            const int v = s_sum[i];
            s_sum[i] = run;
            run += v;
        }
    }
    __syncthreads();
    int at = s_sum[tid];
    for (int q = q0; q < q1; ++q) {
        tile_off[q] = at;
        at += (cloud_off[q + 1] - cloud_off[q] + 31) >> 5;
    }
    if (q1 == Q && (q0 < q1 || tid == 0)) tile_off[Q] = at;             // (every such thread holds the same total)
}

// A tile's 32 consecutive rows from `src` (cin = 8 P floats each, 16-byte aligned) into a lane's P float4 registers, and from there into
// `tile` [32][ld]; the rows past `live` repeat row 0.  Two steps, so that the loads of the NEXT tile fly while this one is multiplied.
template <int P>
__device__ __forceinline__ void tp_fetch_tile(float4 (&pre)[P], const float *__restrict__ src, int live, int lane)
{
    constexpr int C4N = 2 * P, CIN = 8 * P;                       // float4 per row: 8 .. 64
#pragma unroll
    for (int i = 0; i < P; ++i) {                               // (32 C4N = 64 P elements: every lane makes the same P trips)
        const int e = lane + 64 * i, t = e / C4N, c4 = e - t * C4N;
        pre[i] = *reinterpret_cast<const float4 *>(src + (size_t)(t < live ? t : 0) * CIN + 4 * c4);
    }
}

template <int P>
__device__ __forceinline__ void tp_store_tile(float *tile, int ld, const float4 (&pre)[P], int lane)
{
    constexpr int C4N = 2 * P;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int e = lane + 64 * i, t = e / C4N, c4 = e - t * C4N;
        float *d = tile + t * ld + 4 * c4;
        d[0] = pre[i].x;
        d[1] = pre[i].y;
        d[2] = pre[i].z;
        d[3] = pre[i].w;
    }
}

// NT column tiles from n0 of one 32-row tile: per column the largest y and the LOWEST row of the tile attaining it, merged with a strict >
// into (pm, pa) -- `first`: the run's first tile, the partial is written and not read.  j0: the cloud row of tile row 0.
template <int NT, bool VEC>
__device__ __forceinline__ void tp_tile_cols(const float *x, int ldx, const float *w, int ldw, int cin, int n0, const float *__restrict__ bias,
                                             int j0, bool first, float *pm, int32_t *pa, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    mlp_accumulate<NT, K_QUADS, VEC>(acc, mlp_operand<K_QUADS>(x, ldx, r, h), w, ldw, cin, cin, n0, r, h);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + 32 * t + r;
        const float b = bias[col];
        float best = acc[t][0] + b;
        int row = mlp_acc_row(0, h);
#pragma unroll
        for (int i = 1; i < 16; ++i) {                                             // (the rows ascend with i)
            const float y = acc[t][i] + b;
            if (y > best) {
                best = y;
                row = mlp_acc_row(i, h);
            }
        }
        const float ob = __shfl_xor(best, 32);
        const int orow = __shfl_xor(row, 32);
        if (ob > best || (ob == best && orow < row)) {
            best = ob;
            row = orow;
        }
        // rows past n repeat tile row 0 and lose the tie to it; an earlier tile of the run keeps a tie too
        if (h == 0 && (first || best > pm[col])) {
            pm[col] = best;
            pa[col] = j0 + row;
        }
    }
}

// the cout / 32 column tiles, four at a time, then two, then one (mlp_layer's walk)
template <bool VEC>
__device__ __forceinline__ void tp_tile(const float *x, int ldx, const float *w, int ldw, int cin, int cout, const float *__restrict__ bias, int j0,
                                        bool first, float *pm, int32_t *pa, int lane)
{
    int n0 = 0;
    for (; n0 + 128 <= cout; n0 += 128) tp_tile_cols<4, VEC>(x, ldx, w, ldw, cin, n0, bias, j0, first, pm, pa, lane);
    if (n0 + 64 <= cout) {
        tp_tile_cols<2, VEC>(x, ldx, w, ldw, cin, n0, bias, j0, first, pm, pa, lane);
        n0 += 64;
    }
    if (n0 + 32 <= cout) tp_tile_cols<1, VEC>(x, ldx, w, ldw, cin, n0, bias, j0, first, pm, pa, lane);
}

// the cloud a wave is in: its rows and its tiles
struct TpCloud {
    int q, c0, n, tq0, tq1;
    __device__ __forceinline__ void load(const int32_t *__restrict__ cloud_off, const int32_t *__restrict__ tile_off, int q_)
    {
        q = q_;
        c0 = cloud_off[q];
        n = cloud_off[q + 1] - c0;
        tq0 = tile_off[q];
        tq1 = tile_off[q + 1];
    }
    __device__ __forceinline__ int live(int t) const { return n - 32 * (t - tq0) < 32 ? n - 32 * (t - tq0) : 32; }
};

template <int P>                                                         // cin = 8 P
__global__ __launch_bounds__(64 * TP_WAVES) void tp_forward_kernel(const float *__restrict__ rows, const int32_t *__restrict__ cloud_off,
                                                                   const int32_t *__restrict__ tile_off, int Q, const float *__restrict__ W,
                                                                   const float *__restrict__ bias, int cout, int G, int items_max, int staged,
                                                                   float *pmax, int32_t *parg, float *out, int32_t *arg_scratch)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    constexpr int cin = 8 * P, ld = cin + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *tile = s_mem + wave * 32 * ld, *s_w = s_mem + TP_WAVES * 32 * ld;
    if (staged) {
        for (int e = tid; e < cout * cin; e += 64 * TP_WAVES) {
            const int o = e / cin, k = e - o * cin;
            s_w[o * ld + k] = W[e];
        }
    }
    __syncthreads();
    // (items_max: what the workspace was sized for; a table that keeps the header's promises never exceeds it)
    const int T = tile_off[Q], items = min((T + G - 1) / G, items_max);
    float4 pre[P];
    for (int item = blockIdx.x * TP_WAVES + wave; item < items; item += gridDim.x * TP_WAVES) {
        const int t_begin = item * G, t_end = min(T, t_begin + G);       // (item * G < T + G: no overflow)
        int lo = 0, hi = Q - 1;                                          // the cloud of tile t_begin: the last q with tile_off[q] <= t_begin
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tile_off[mid] <= t_begin) lo = mid; else hi = mid - 1;
        }
        TpCloud cl;
        cl.load(cloud_off, tile_off, lo);
        if (t_begin < t_end) tp_fetch_tile<P>(pre, rows + (size_t)(cl.c0 + 32 * (t_begin - cl.tq0)) * cin, cl.live(t_begin), lane);
        for (int t = t_begin; t < t_end; ++t) {
            // the RUN of this tile: the item's tiles of cloud cl.  A run that is the whole cloud goes to the cloud's row of out / arg; else
            // to the item's slot 1 when the cloud goes on in the next item, slot 0 when it ends here (it began in an earlier one)
            const bool whole = cl.tq0 >= t_begin && cl.tq1 <= t_end, first = t == t_begin || t == cl.tq0;
            const size_t at = whole ? (size_t)cl.q * cout : ((size_t)2 * item + (cl.tq1 > t_end ? 1 : 0)) * cout;
            float *pm = (whole ? out : pmax) + at;
            int32_t *pa = (whole ? arg_scratch : parg) + at;
            const int j0 = 32 * (t - cl.tq0);
            tp_store_tile<P>(tile, ld, pre, lane);
            wave_lds_sync();
            // the next tile of the item: this cloud's, or the first of the next cloud (every cloud owns a tile); its loads fly during the MFMAs
            TpCloud nx = cl;
            if (t + 1 < t_end) {
                if (t + 1 >= cl.tq1 && cl.q + 1 < Q) nx.load(cloud_off, tile_off, cl.q + 1);
                tp_fetch_tile<P>(pre, rows + (size_t)(nx.c0 + 32 * (t + 1 - nx.tq0)) * cin, nx.live(t + 1), lane);
            }
            if (staged)                                                  // (two calls: each keeps its weights' address space)
                tp_tile<false>(tile, ld, s_w, ld, cin, cout, bias, j0, first, pm, pa, lane);
            else
                tp_tile<true>(tile, ld, W, cin, cin, cout, bias, j0, first, pm, pa, lane);
            wave_lds_sync();                                             // the next store overwrites the tile: every read of it is done
            cl = nx;
        }
    }
}

// a thread per (cloud, column): a cloud that spans several items combines its runs in ascending order, strict >; every other cloud was
// written by the forward kernel.  arg_scratch: where the forward kernel put the whole clouds' rows (arg_out, or a workspace array)
__global__ __launch_bounds__(256) void tp_reduce_kernel(const float *__restrict__ pmax, const int32_t *__restrict__ parg,
                                                       const int32_t *__restrict__ tile_off, int G, int cout, int n_out, float *__restrict__ out,
                                                       int32_t *__restrict__ arg_out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out) return;
    const int q = e / cout, c = e - q * cout;
    const int g0 = tile_off[q] / G, g1 = (tile_off[q + 1] - 1) / G;
    if (g0 == g1) return;
    float best = pmax[((size_t)2 * g0 + 1) * cout + c];
    int32_t brow = parg[((size_t)2 * g0 + 1) * cout + c];
    for (int g = g0 + 1; g <= g1; ++g) {
        const size_t at = ((size_t)2 * g + (g < g1 ? 1 : 0)) * cout + c;
        const float v = pmax[at];
        if (v > best) {
            best = v;
            brow = parg[at];
        }
    }
    out[e] = best;
    if (arg_out) arg_out[e] = brow;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// A workgroup per cloud, 256 threads: thread c < cout owns arg[q, c], thread k < cin column k of dx.  The channels are sorted by
// (winner row, channel) -- a rank by counting -- so that a winner's channels stand together in ascending order: one pass over the sorted
// list then forms every winner's row of dx, O(cout) steps per column.
__global__ __launch_bounds__(256) void tp_dx_kernel(const int32_t *__restrict__ cloud_off, const float *__restrict__ W, const int32_t *__restrict__ arg,
                                                   const float *__restrict__ dout, int cin, int cout, float *__restrict__ dx)
{
    __shared__ int s_val[TP_MAX], s_order[TP_MAX];
    __shared__ float s_g[TP_MAX];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int c0 = cloud_off[q], n = cloud_off[q + 1] - c0;
    if (n < 1) return;                                                   // (uniform; a table that keeps the header's promises has none)
    if (tid < cout) {
        s_val[tid] = min(max(arg[(size_t)q * cout + tid], 0), n - 1);
        s_g[tid] = dout[(size_t)q * cout + tid];
    }
    __syncthreads();
    if (tid < cout) {
        const int v = s_val[tid];
        int rank = 0;
        for (int o = 0; o < cout; ++o) rank += s_val[o] < v || (s_val[o] == v && o < tid);
        s_order[rank] = tid;
    }
    __syncthreads();
    if (tid >= cin) return;
    float acc = 0.0f;
    int r = s_val[s_order[0]];
    for (int i = 0; i < cout; ++i) {
        const int c = s_order[i], rc = s_val[c];
        if (rc != r) {                                                   // (uniform) the winner before is complete
            dx[(size_t)(c0 + r) * cin + tid] = acc;
            acc = 0.0f;
            r = rc;
        }
        acc = fmaf(s_g[c], W[(size_t)c * cin + tid], acc);
    }
    dx[(size_t)(c0 + r) * cin + tid] = acc;
}

// a thread per (c, k), k fastest
__global__ __launch_bounds__(256) void tp_dw_kernel(const float *__restrict__ rows, const int32_t *__restrict__ cloud_off,
                                                   const int32_t *__restrict__ arg, const float *__restrict__ dout, int Q, int cin, int cout,
                                                   float *__restrict__ dW, float *__restrict__ db)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= cout * cin) return;
    const int c = e / cin, k = e - c * cin;
    float acc = 0.0f, accb = 0.0f;
#pragma unroll 4
    for (int q = 0; q < Q; ++q) {
        const int c0 = cloud_off[q], n = cloud_off[q + 1] - c0;
        const int r = max(min(arg[(size_t)q * cout + c], n - 1), 0);
        const float g = dout[(size_t)q * cout + c];
        acc = fmaf(g, rows[(size_t)(c0 + r) * cin + k], acc);
        accb += g;
    }
    if (dW) dW[e] = acc;
    if (db && k == 0) db[c] = accb;
}

}  // namespace ampnet

extern "C" size_t ampnet_token_pool_forward_workspace_bytes(int cin, int cout, int Q, long long total)
{
    using namespace ampnet;
    TpShape sh;
    if (tp_shape("ampnet_token_pool_forward_workspace_bytes", cin, cout, Q, total, sh) != AMPNET_OK) return 0;
    return sh.words * 4;
}

extern "C" int ampnet_token_pool_forward_f32(const float *rows, const int32_t *cloud_off, int Q, long long total, const float *W, const float *bias,
                                             int cin, int cout, float *out, int32_t *arg_out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_token_pool_forward_f32";
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(rows && cloud_off && W && bias && out, "%s: null pointer", what);
    TpShape sh;
    AMPNET_TRY(tp_shape(what, cin, cout, Q, total, sh));
    AMPNET_REQUIRE(((uintptr_t)rows | (uintptr_t)W) % 16 == 0, "%s: rows and W must be 16-byte aligned", what);
    AMPNET_REQUIRE(workspace && workspace_bytes >= sh.words * 4, "%s: workspace of %zu bytes, %zu are needed (ampnet_token_pool_forward_workspace_bytes)",
                   what, workspace ? workspace_bytes : (size_t)0, sh.words * 4);
    AMPNET_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", what);
    int32_t *ws = static_cast<int32_t *>(workspace);
    int32_t *tile_off = ws, *parg = ws + sh.off_parg;
    float *pmax = reinterpret_cast<float *>(ws + sh.off_pmax);
    hipLaunchKernelGGL(tp_tile_scan_kernel, dim3(1), dim3(TP_SCAN_THREADS), 0, st, cloud_off, Q, tile_off);
    AMPNET_TRY(check_launch("tp_tile_scan_kernel"));
    int32_t *arg_scratch = arg_out ? arg_out : ws + sh.off_arg;
#define TP_LAUNCH(P)                                                                                                                      \
    case P: {                                                                                                                             \
        AMPNET_TRY(allow_dynamic_lds<tp_forward_kernel<P>>(MLP_LDS_BYTES, what));                                                          \
        hipLaunchKernelGGL(tp_forward_kernel<P>, dim3(sh.grid), dim3(64 * TP_WAVES), sh.lds, st, rows, cloud_off, tile_off, Q, W, bias, cout, \
                           sh.G, sh.items, sh.staged, pmax, parg, out, arg_scratch);                                                      \
        break;                                                                                                                            \
    }
    switch (cin / 8) {                                                   // (one instantiation per cin: the prefetch lives in registers)
        TP_LAUNCH(4) TP_LAUNCH(8) TP_LAUNCH(12) TP_LAUNCH(16) TP_LAUNCH(20) TP_LAUNCH(24) TP_LAUNCH(28) TP_LAUNCH(32)
    }
#undef TP_LAUNCH
    AMPNET_TRY(check_launch("tp_forward_kernel"));
    const long long n_out = (long long)Q * cout;
    hipLaunchKernelGGL(tp_reduce_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, pmax, parg, tile_off, sh.G, cout, (int)n_out, out,
                       arg_out);
    return check_launch("tp_reduce_kernel");
}

extern "C" size_t ampnet_token_pool_backward_workspace_bytes(int cin, int cout, int Q, long long total)
{
    using namespace ampnet;
    if (tp_check("ampnet_token_pool_backward_workspace_bytes", cin, cout, Q, total) != AMPNET_OK) return 0;
    return 256;                                                              // (nothing is kept there today; a non-zero size means accepted)
}

extern "C" int ampnet_token_pool_backward_f32(const float *rows, const int32_t *cloud_off, int Q, long long total, const float *W, int cin, int cout,
                                              const int32_t *arg, const float *dout, float *dx, float *dW, float *db, void *workspace,
                                              size_t workspace_bytes, void *stream)
{
    using namespace ampnet;
    const char *what = "ampnet_token_pool_backward_f32";
    hipStream_t st = (hipStream_t)stream;
    AMPNET_REQUIRE(rows && cloud_off && W && arg && dout, "%s: null pointer", what);
    AMPNET_TRY(tp_check(what, cin, cout, Q, total));
    (void)workspace;
    (void)workspace_bytes;
    if (dx) {
        if (hipMemsetAsync(dx, 0, (size_t)total * cin * sizeof(float), st) != hipSuccess) return fail(AMPNET_E_LAUNCH, "%s: memset of dx failed", what);
        hipLaunchKernelGGL(tp_dx_kernel, dim3(Q), dim3(256), 0, st, cloud_off, W, arg, dout, cin, cout, dx);
        AMPNET_TRY(check_launch("tp_dx_kernel"));
    }
    if (dW || db) {
        hipLaunchKernelGGL(tp_dw_kernel, dim3(cdiv(cout * cin, 256)), dim3(256), 0, st, rows, cloud_off, arg, dout, Q, cin, cout, dW, db);
        AMPNET_TRY(check_launch("tp_dw_kernel"));
    }
    return AMPNET_OK;
}
