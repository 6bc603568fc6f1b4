// layer_probe.hip -- test hooks (include/ampnet_hip.h, "test hooks"): one launch of pw_gemm / pw_bwd_fused on buffers the caller
// chooses, for the layer-local float64 parity tests (tests/test_pw_layers_gpu.py).  No product path calls these.
//
// The probes exist for shared GPUs: before anything is launched every extent is checked on the host against what the kernel will
// touch (rows from win_off / uniform_rows, partial slots from the statistics plan, ld x rows), so that a wrong test gets
// AMPNET_E_ARG instead of an out-of-bounds access.  win_off is copied to the host once per call for that.
#include <vector>
#include "kernels.h"
#include "encoder.h"

namespace ampnet {
namespace {

// the window offsets on the host: Q + 1 ascending values from 0 up; total rows and the largest window
int read_win_off(const int32_t *win_off, int64_t n, int Q, hipStream_t st, int64_t &rows, int &max_rows)
{
    AMPNET_REQUIRE(win_off && n >= (int64_t)Q + 1, "probe: win_off needs Q + 1 = %d entries (has %lld)", Q + 1, (long long)n);
    std::vector<int32_t> h((size_t)Q + 1);
    if (hipMemcpyAsync(h.data(), win_off, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(AMPNET_E_LAUNCH, "probe: copying win_off failed");
    AMPNET_REQUIRE(h[0] >= 0, "probe: win_off[0] = %d < 0", h[0]);
    max_rows = 0;
    for (int q = 0; q < Q; ++q) {
        AMPNET_REQUIRE(h[q + 1] >= h[q], "probe: win_off not ascending at %d (%d > %d)", q, h[q], h[q + 1]);
        if (h[q + 1] - h[q] > max_rows) max_rows = h[q + 1] - h[q];
    }
    rows = h[Q];
    return AMPNET_OK;
}

// [rows, ld] with `cols` used columns
bool covers(int64_t n, int64_t rows, int64_t ld, int64_t cols) { return rows <= 0 || (ld >= cols && n >= (rows - 1) * ld + cols); }

}  // namespace
}  // namespace ampnet

extern "C" int ampnet_probe_pw_gemm_f32(const AmpnetPwGemmProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_pw_gemm: null descriptor");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AMPNET_REQUIRE(d->Q >= 1 && d->chunks >= 1 && d->chunk_rows >= 1 && d->n_slots >= 1 && d->cout >= 1 && d->cin >= 1,
                   "probe_pw_gemm: bad sizes");
    int64_t rows = 0;
    int max_rows = 0;
    if (d->uniform_rows > 0) {
        rows = (int64_t)d->Q * d->uniform_rows;
        max_rows = d->uniform_rows;
    } else if (int rc = read_win_off(d->win_off, d->win_off_n, d->Q, st, rows, max_rows); rc != AMPNET_OK) {
        return rc;
    }
    AMPNET_REQUIRE((int64_t)d->chunks * d->chunk_rows >= max_rows, "probe_pw_gemm: %d chunks of %d rows do not cover a window of %d rows",
                   d->chunks, d->chunk_rows, max_rows);
    const int64_t Q = d->Q, cin = d->cin, cout = d->cout, S = d->n_slots;
    AMPNET_REQUIRE(d->A && covers(d->A_n, rows, d->lda, cin), "probe_pw_gemm: A [%lld, %d] short", (long long)rows, d->lda);
    if (d->w_win_stride) {
        const int64_t pmax = Q - 1;   // pidx < Q, slot-major or not
        AMPNET_REQUIRE(d->W && d->w_win_stride >= cin * cout && d->W_n >= pmax * d->w_win_stride + cin * cout, "probe_pw_gemm: per-window W short");
    } else {
        AMPNET_REQUIRE(d->W && covers(d->W_n, cout, d->ldw, cin), "probe_pw_gemm: W [%d, %d] short", d->cout, d->ldw);
    }
    if (d->bias) {
        const int64_t need = d->bias_win_stride ? (Q - 1) * d->bias_win_stride + cout : cout;
        AMPNET_REQUIRE(d->bias_n >= need, "probe_pw_gemm: bias short");
    }
    AMPNET_REQUIRE((d->pro_scale == nullptr) == (d->pro_shift == nullptr) && (!d->pro_scale || d->pro_n >= S * cin), "probe_pw_gemm: prologue constants short");
    AMPNET_REQUIRE(!d->Z || covers(d->Z_n, rows, d->ldz, cout), "probe_pw_gemm: Z short");
    if (d->part_rows) {
        AMPNET_REQUIRE(d->stat_lanes >= d->n_slots && d->stat_lanes <= 2048, "probe_pw_gemm: stat_lanes %d", d->stat_lanes);
        const int64_t parts = (int64_t)cdiv(d->stat_lanes, d->n_slots) * S;
        AMPNET_REQUIRE(d->part_sum && d->part_sq && d->part_n >= parts * cout && d->part_rows_n >= parts, "probe_pw_gemm: per-workgroup partials short");
    } else if (d->part_sum || d->part_sq) {
        AMPNET_REQUIRE(d->part_sum && d->part_sq && d->part_n >= Q * d->chunks * cout, "probe_pw_gemm: per-chunk partials short");
    }
    AMPNET_REQUIRE(!d->part_max || d->pool_n >= Q * d->chunks * cout, "probe_pw_gemm: pool partials short");
    AMPNET_REQUIRE(!d->pool_gamma || d->pool_gamma_n >= cout, "probe_pw_gemm: pool_gamma short");
    if (d->fin_scale) {
        AMPNET_REQUIRE(d->fin_gamma && d->fin_beta && d->fin_in_n >= cout && d->fin_shift && d->fin_out_n >= S * cout, "probe_pw_gemm: fin_* short");
    }
    if (d->pfin_sum) {
        AMPNET_REQUIRE(d->pfin_sq && d->pfin_rows && d->pfin_parts >= 1 && d->pfin_n >= (int64_t)d->pfin_parts * cin &&
                           d->pfin_rows_n >= d->pfin_parts && d->pfin_gamma && d->pfin_beta &&
                           d->pfin_in_n >= cin && d->pfin_out_n >= S * cin,
                       "probe_pw_gemm: pfin_* short");
    }
    PwGemm g;
    g.A = d->A; g.lda = d->lda; g.cin = d->cin;
    g.W = d->W; g.ldw = d->ldw; g.w_win_stride = d->w_win_stride; g.perwin_slot_major = d->perwin_slot_major;
    g.bias = d->bias; g.bias_win_stride = d->bias_win_stride;
    g.pro_scale = d->pro_scale; g.pro_shift = d->pro_shift;
    g.n_slots = d->n_slots; g.drop_p = d->drop_p; g.drop_seed = d->drop_seed;
    g.Z = d->Z; g.ldz = d->ldz; g.cout = d->cout;
    g.part_sum = d->part_sum; g.part_sq = d->part_sq; g.part_rows = d->part_rows; g.stat_lanes = d->stat_lanes;
    g.part_max = d->part_max; g.part_amax = d->part_amax; g.pool_gamma = d->pool_gamma;
    g.win_off = d->uniform_rows > 0 ? nullptr : d->win_off;
    g.Q = d->Q; g.chunk_rows = d->chunk_rows; g.chunks = d->chunks; g.rows_hint = rows;
    g.uniform_rows = d->uniform_rows; g.identity_k = d->identity_k;
    g.fin_gamma = d->fin_gamma; g.fin_beta = d->fin_beta; g.fin_eps = d->fin_eps;
    g.fin_scale = d->fin_scale; g.fin_shift = d->fin_shift; g.fin_mean = d->fin_mean; g.fin_invstd = d->fin_invstd;
    g.fin_smean = d->fin_smean; g.fin_suvar = d->fin_suvar;
    g.pfin_sum = d->pfin_sum; g.pfin_sq = d->pfin_sq; g.pfin_rows = d->pfin_rows; g.pfin_parts = d->pfin_parts;
    g.pfin_gamma = d->pfin_gamma; g.pfin_beta = d->pfin_beta;
    g.pfin_scale = d->pfin_scale; g.pfin_shift = d->pfin_shift; g.pfin_mean = d->pfin_mean; g.pfin_invstd = d->pfin_invstd;
    g.pfin_smean = d->pfin_smean; g.pfin_suvar = d->pfin_suvar;
    return pw_gemm(g, st);
}

namespace ampnet {
namespace {
PwBwd bwd_record(const AmpnetPwBwdProbe *d)
{
    PwBwd p;
    p.g.dy = d->dy; p.g.z = d->gz; p.g.P1 = d->P1; p.g.P2 = d->P2; p.g.P3 = d->P3; p.g.act = d->act; p.g.C = d->CX; p.g.z_bf16 = d->g_z_bf16;
    p.prev.z = d->pz; p.prev.s = d->ps; p.prev.t = d->pt; p.prev.drop_p = d->drop_p; p.prev.drop_seed = d->drop_seed; p.prev.C = d->CY;
    p.prev.z_bf16 = d->prev_z_bf16;
    p.prev_mean = d->prev_mean; p.prev_invstd = d->prev_invstd;
    p.W = d->W; p.ldw = d->ldw; p.w_slot_stride = d->w_slot_stride; p.w_win_stride = d->w_win_stride; p.perwin_slot_major = d->perwin_slot_major;
    p.bias_slot = d->bias_slot; p.add = d->add; p.out = d->out;
    p.dWpart = d->dWpart; p.dbpart = d->dbpart; p.part_a = d->part_a; p.part_b = d->part_b;
    p.win_off = d->win_off; p.Q = d->Q; p.n_slots = d->n_slots; p.max_rows = d->max_rows;
    p.blocks_per_slot = d->blocks_per_slot; p.items_per_block = d->items_per_block;
    p.fin_part_a = d->fin_part_a; p.fin_part_b = d->fin_part_b; p.fin_parts = d->fin_parts; p.fin_rows = d->fin_rows;
    p.fin_gamma = d->fin_gamma; p.fin_mean = d->fin_mean; p.fin_invstd = d->fin_invstd;
    p.fin_P1 = d->fin_P1; p.fin_P2 = d->fin_P2; p.fin_P3 = d->fin_P3; p.fin_slot_ab = d->fin_slot_ab;
    p.dbg_row_wrap = 0;
    return p;
}
}  // namespace
}  // namespace ampnet

extern "C" int ampnet_probe_pw_bwd_f32(const AmpnetPwBwdProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_pw_bwd: null descriptor");
    AMPNET_REQUIRE(d->kind == 0, "probe_pw_bwd: kind %d not built (0 = pw_bwd_fused)", d->kind);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AMPNET_REQUIRE(d->Q >= 1 && d->n_slots >= 1 && d->max_rows >= 1 && pw_bwd_supported(d->CX, d->CY) && d->blocks_per_slot >= 1 &&
                       d->blocks_per_slot <= 4096 && d->items_per_block >= 0,
                   "probe_pw_bwd: bad sizes");
    int64_t rows = 0;
    int max_rows = 0;
    if (int rc = read_win_off(d->win_off, d->win_off_n, d->Q, st, rows, max_rows); rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE(max_rows <= d->max_rows, "probe_pw_bwd: a window has %d rows > max_rows %d", max_rows, d->max_rows);
    const int64_t CX = d->CX, CY = d->CY, S = d->n_slots, grid = (int64_t)d->blocks_per_slot * S;
    AMPNET_REQUIRE(d->gz && d->g_n >= rows * CX && (!d->dy || d->g_n >= rows * CX), "probe_pw_bwd: g tensors short");
    AMPNET_REQUIRE(d->pz && d->pz_n >= rows * CY, "probe_pw_bwd: prev z short");
    AMPNET_REQUIRE(d->P_n >= S * CX || !(d->P1 || d->P2 || d->P3), "probe_pw_bwd: P1..P3 short");
    AMPNET_REQUIRE(d->ps_n >= S * CY || !(d->ps || d->pt || d->prev_mean || d->prev_invstd), "probe_pw_bwd: prev constants short");
    // every fused kernel reads prev.t wherever prev.s is set (and the Gram / act form reads P2, P3): the pairs come together
    AMPNET_REQUIRE((d->ps == nullptr) == (d->pt == nullptr), "probe_pw_bwd: prev scale and shift must come together");
    AMPNET_REQUIRE((d->prev_mean == nullptr) == (d->prev_invstd == nullptr), "probe_pw_bwd: prev mean and invstd must come together");
    AMPNET_REQUIRE(d->P2 && d->P3 && (d->act || (d->dy && (d->P1 || d->fin_part_a))), "probe_pw_bwd: gradient source incomplete");
    AMPNET_REQUIRE(!d->act || d->gz == d->pz, "probe_pw_bwd: the Gram form reads one tensor as both operands");
    AMPNET_REQUIRE(!d->bias_slot || d->bias_slot_n >= S * CY, "probe_pw_bwd: bias_slot short");
    AMPNET_REQUIRE(!d->add || d->add_n >= rows * CY, "probe_pw_bwd: add short");
    AMPNET_REQUIRE(d->out && d->out_n >= rows * CY, "probe_pw_bwd: out short");
    if (d->w_win_stride) {
        const int item_rows = pw_bwd_item_rows();
        const int64_t cpw = (d->max_rows + item_rows - 1) / item_rows;
        AMPNET_REQUIRE(d->items_per_block > 0 && d->Q % d->n_slots == 0 && d->w_win_stride >= CX * CY && d->W &&
                           d->W_n >= (int64_t)(d->Q - 1) * d->w_win_stride + CX * CY,
                       "probe_pw_bwd: per-window W short");
        // a workgroup past the last item would still look up the weights of the window after the last
        AMPNET_REQUIRE((int64_t)d->blocks_per_slot * d->items_per_block <= (d->Q / d->n_slots) * cpw, "probe_pw_bwd: more workgroups than items");
    } else {
        AMPNET_REQUIRE(d->W && d->w_slot_stride >= 0 && covers(d->W_n - (S - 1) * d->w_slot_stride, CX, d->ldw, CY), "probe_pw_bwd: W short");
    }
    AMPNET_REQUIRE(d->dWpart && d->dW_n >= grid * CX * CY, "probe_pw_bwd: dWpart short (%lld workgroups)", (long long)grid);
    AMPNET_REQUIRE(!d->dbpart || d->db_n >= grid * CX, "probe_pw_bwd: dbpart short");
    AMPNET_REQUIRE((!d->part_a && !d->part_b) || (d->part_a && d->part_b && d->pab_n >= grid * CY), "probe_pw_bwd: part_a / part_b short");
    if (d->fin_part_a) {
        AMPNET_REQUIRE(d->fin_part_b && d->fin_parts >= 1 && d->fin_part_n >= (int64_t)d->fin_parts * CX && d->fin_in_n >= S * CX &&
                           d->fin_out_n >= 2 * S * CX,
                       "probe_pw_bwd: fin_* short");
    }
    return pw_bwd_fused(bwd_record(d), st);
}

extern "C" int ampnet_probe_pw_plan(int Q, int n_slots, int max_rows, int cin, int cout, int stat_chunks, const AmpnetPwBwdProbe *bwd, AmpnetPwPlan *o)
{
    using namespace ampnet;
    AMPNET_REQUIRE(o && Q >= 1 && n_slots >= 1 && max_rows >= 1 && stat_chunks >= 1, "probe_pw_plan: bad arguments");
    o->stat_lane_cap = pw_gemm_stat_lane_cap(cin, cout);
    const PwStatPlan p = pw_gemm_stat_plan(Q, stat_chunks, n_slots, o->stat_lane_cap);
    o->stat_lanes = p.lanes;
    o->stat_parts = p.parts;
    o->stat_direct = p.direct ? 1 : 0;
    const EncShape s = enc_shape(Q, n_slots, 0, max_rows, 1);
    o->chunk_rows = s.chunk_rows;
    o->chunks = s.chunks;
    o->x_chunk_rows = s.x_chunk_rows;
    o->x_chunks = s.x_chunks;
    o->fc_rows = s.fc_rows;
    o->fc_chunk_rows = s.fc_chunk_rows;
    o->fc_chunks = s.fc_chunks;
    o->bwd_blocks = pw_bwd_blocks(Q, n_slots, max_rows);
    o->bwd_item_rows = pw_bwd_item_rows();
    o->bwd_x3 = bwd ? (pw_bwd_x3_supported(bwd_record(bwd)) ? 1 : 0) : -1;
    return AMPNET_OK;
}
