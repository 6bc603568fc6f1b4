// layer_probe.hip -- test hooks (include/ampnet_hip.h, "test hooks"): one launch of pw_gemm / pw_bwd_fused / pw_dgrad / pw_wgrad, of a
// kernel of the max-pooled layers' backward or of the input layers' weight gradient on buffers the caller chooses, for the layer-local
// float64 parity tests (tests/test_pw_layers_gpu.py, tests/test_pooled_bwd_gpu.py), of the head's kernels (tests/test_head_layers_gpu.py) and of
// the BatchNorm / pooling glue kernels (tests/test_bn_glue_gpu.py), and of the GRU recurrence and the classification head's kernels
// (tests/test_gru_cls_layers_gpu.py).  No product path calls these.
//
// The probes exist for shared GPUs: before anything is launched every extent is checked on the host against what the kernel will
// touch (rows from win_off / uniform_rows, partial slots from the statistics plan, ld x rows), so that a wrong test gets
// AMPNET_E_ARG instead of an out-of-bounds access.  win_off is copied to the host once per call for that.
#include <vector>
#include "kernels.h"
#include "bwd_misc.h"
#include "encoder.h"
#include "head.h"
#include "baseline.h"

namespace ampnet {
namespace {

// the BatchNorm descriptors (bn_desc.h) are the workspaces' arrays, which are not const; a probe's read-only inputs enter them through here
float *ro(const float *p) { return const_cast<float *>(p); }

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
    AMPNET_REQUIRE(d->tail == 0 || d->tail == 1, "probe_pw_gemm: tail = %d is neither 0 (ends at pfin_out_n) nor 1 (a_bf16 / z_bf16 follow)", d->tail);
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
    // bf16 tensors: A_n / Z_n are in elements, the checks above hold; pw_gemm's own checks gate the rest.  tail == 0: a descriptor that
    // ends at pfin_out_n (callers from before the two flags) -- reading on would be reading past the caller's struct
    if (d->tail == 1) { g.a_bf16 = d->a_bf16; g.z_bf16 = d->z_bf16; }
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
    g.eps = d->fin_eps;
    g.fin = BnFin{{d->fin_gamma, d->fin_beta}, {d->fin_scale, d->fin_shift, d->fin_mean, d->fin_invstd, d->fin_smean, d->fin_suvar}};
    g.pfin = BnPfin{{d->pfin_sum, d->pfin_sq, d->pfin_rows, d->pfin_parts},
                    {d->pfin_gamma, d->pfin_beta},
                    {d->pfin_scale, d->pfin_shift, d->pfin_mean, d->pfin_invstd, d->pfin_smean, d->pfin_suvar}};
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
    p.fin = BnBwdFin{d->fin_part_a, d->fin_part_b, d->fin_parts, d->fin_rows, d->fin_gamma, d->fin_mean, d->fin_invstd,
                     {d->fin_P1, d->fin_P2, d->fin_P3, d->fin_slot_ab}};
    p.dbg_row_wrap = 0;
    return p;
}
}  // namespace
}  // namespace ampnet

namespace ampnet {
namespace {
// kinds 1 (pw_dgrad) and 2 (pw_wgrad): the unfused kernels, fp32 tensors, dense or act gradient source
int probe_unfused(const AmpnetPwBwdProbe *d, hipStream_t st)
{
    AMPNET_REQUIRE(d->Q >= 1 && d->n_slots >= 1 && d->chunks >= 1 && d->chunk_rows >= 1 && d->CX >= 1 && d->CY >= 1 && d->CX % 4 == 0 &&
                       d->CY % 4 == 0 && d->CX <= 256 && d->CY <= 256,
                   "probe_pw_bwd: bad sizes");
    AMPNET_REQUIRE(!d->g_z_bf16 && !d->prev_z_bf16, "probe_pw_bwd: kinds 1 and 2 read fp32 tensors only");
    AMPNET_REQUIRE(d->act ? (d->gz && d->P2 && d->P3 && !d->dy && !d->P1) : (d->dy != nullptr), "probe_pw_bwd: gradient source is neither dense nor act");
    AMPNET_REQUIRE(!d->P1 || (d->P2 && d->P3 && d->gz), "probe_pw_bwd: BatchNorm constants incomplete");
    AMPNET_REQUIRE((d->ps == nullptr) == (d->pt == nullptr), "probe_pw_bwd: prev scale and shift must come together");
    AMPNET_REQUIRE((d->prev_mean == nullptr) == (d->prev_invstd == nullptr), "probe_pw_bwd: prev mean and invstd must come together");
    AMPNET_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f && (d->drop_p == 0.f || d->ps), "probe_pw_bwd: dropout needs the activation");
    int64_t rows = 0;
    int max_rows = 0;
    if (int rc = read_win_off(d->win_off, d->win_off_n, d->Q, st, rows, max_rows); rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE((int64_t)d->chunks * d->chunk_rows >= max_rows, "probe_pw_bwd: %d chunks of %d rows do not cover a window of %d rows", d->chunks,
                   d->chunk_rows, max_rows);
    const int64_t CX = d->CX, CY = d->CY, S = d->n_slots, Q = d->Q, parts = Q * d->chunks;
    AMPNET_REQUIRE((!d->dy || d->g_n >= rows * CX) && (!d->gz || d->g_n >= rows * CX), "probe_pw_bwd: g tensors short");
    AMPNET_REQUIRE(d->P_n >= S * CX || !(d->P1 || d->P2 || d->P3), "probe_pw_bwd: P1..P3 short");
    AMPNET_REQUIRE(d->ps_n >= S * CY || !(d->ps || d->prev_mean), "probe_pw_bwd: prev constants short");
    if (d->kind == 1) {
        AMPNET_REQUIRE(d->CX == 64 || d->CX == 128 || d->CX == 256, "probe_pw_bwd: pw_dgrad K=%d not in {64, 128, 256}", d->CX);
        AMPNET_REQUIRE(d->cp == d->CY, "probe_pw_bwd: pw_dgrad writes cp = CY columns (cp %d, CY %d)", d->cp, d->CY);
        AMPNET_REQUIRE(!d->pz || d->pz_n >= rows * CY, "probe_pw_bwd: prev z short");
        AMPNET_REQUIRE(!d->ps || d->pz, "probe_pw_bwd: prev constants without prev z");
        AMPNET_REQUIRE(d->W && d->out && d->out_n >= rows * CY, "probe_pw_bwd: out short");
        if (d->w_win_stride) {
            AMPNET_REQUIRE(!d->w_slot_stride && (!d->perwin_slot_major || Q % S == 0) && d->w_win_stride >= CX * CY &&
                               d->W_n >= (Q - 1) * d->w_win_stride + CX * CY,
                           "probe_pw_bwd: per-window W short");
        } else {
            AMPNET_REQUIRE(d->ldw % 4 == 0 && d->w_slot_stride >= 0 && covers(d->W_n - (S - 1) * d->w_slot_stride, CX, d->ldw, CY), "probe_pw_bwd: W short");
        }
        AMPNET_REQUIRE(!d->bias_slot || d->bias_slot_n >= S * CY, "probe_pw_bwd: bias_slot short");
        AMPNET_REQUIRE(!d->add || d->add_n >= rows * CY, "probe_pw_bwd: add short");
        const int64_t pc = d->part_chunks ? d->part_chunks : d->chunks;
        AMPNET_REQUIRE(d->part_chunks == 0 || d->part_chunks >= d->chunks, "probe_pw_bwd: part_chunks %d < chunks %d", d->part_chunks, d->chunks);
        AMPNET_REQUIRE((d->part_a == nullptr) == (d->part_b == nullptr) && (!d->part_a || (d->pz && d->pab_n >= Q * pc * CY)),
                       "probe_pw_bwd: part_a / part_b short");
        PwDgrad g;
        g.g.dy = d->dy; g.g.z = d->gz; g.g.P1 = d->P1; g.g.P2 = d->P2; g.g.P3 = d->P3; g.g.act = d->act; g.g.C = d->CX;
        g.W = d->W; g.ldw = d->ldw; g.w_win_stride = d->w_win_stride; g.perwin_slot_major = d->perwin_slot_major; g.w_slot_stride = d->w_slot_stride;
        g.bias_slot = d->bias_slot; g.add = d->add;
        g.prev.z = d->pz; g.prev.s = d->ps; g.prev.t = d->pt; g.prev.drop_p = d->drop_p; g.prev.drop_seed = d->drop_seed; g.prev.C = d->CY;
        g.prev_mean = d->prev_mean; g.prev_invstd = d->prev_invstd;
        g.out = d->out; g.cp = d->cp; g.part_a = d->part_a; g.part_b = d->part_b; g.part_chunks = d->part_chunks;
        g.win_off = d->win_off; g.Q = d->Q; g.n_slots = d->n_slots; g.chunk_rows = d->chunk_rows; g.chunks = d->chunks; g.rows_hint = rows;
        return pw_dgrad(g, st);
    }
    AMPNET_REQUIRE(d->chunk_rows % 64 == 0, "probe_pw_bwd: pw_wgrad chunk_rows %d not a multiple of 64", d->chunk_rows);
    AMPNET_REQUIRE(d->pz && d->pz_n >= rows * CY, "probe_pw_bwd: y z short");
    AMPNET_REQUIRE(d->ldp >= d->CY && d->dWpart && d->dW_n >= parts * CX * d->ldp, "probe_pw_bwd: dWpart short (%lld partials)", (long long)parts);
    AMPNET_REQUIRE(!d->dbpart || d->db_n >= parts * CX, "probe_pw_bwd: dbpart short");
    PwWgrad w;
    w.x.dy = d->dy; w.x.z = d->gz; w.x.P1 = d->P1; w.x.P2 = d->P2; w.x.P3 = d->P3; w.x.act = d->act; w.x.C = d->CX;
    w.y.z = d->pz; w.y.s = d->ps; w.y.t = d->pt; w.y.drop_p = d->drop_p; w.y.drop_seed = d->drop_seed; w.y.C = d->CY;
    w.dWpart = d->dWpart; w.ldp = d->ldp; w.dbpart = d->dbpart;
    w.win_off = d->win_off; w.Q = d->Q; w.n_slots = d->n_slots; w.chunk_rows = d->chunk_rows; w.chunks = d->chunks; w.rows_hint = rows;
    return pw_wgrad(w, st);
}
}  // namespace
}  // namespace ampnet

extern "C" int ampnet_probe_pw_bwd_f32(const AmpnetPwBwdProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_pw_bwd: null descriptor");
    AMPNET_REQUIRE(d->kind >= 0 && d->kind <= 2, "probe_pw_bwd: kind %d not built (0 = pw_bwd_fused, 1 = pw_dgrad, 2 = pw_wgrad)", d->kind);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d->kind != 0) return probe_unfused(d, st);
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

namespace ampnet {
namespace {
template <typename T> int to_host(const T *src, int64_t n, std::vector<T> &h, hipStream_t st, const char *what)
{
    h.resize((size_t)n);
    if (n > 0 && (hipMemcpyAsync(h.data(), src, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
        return fail(AMPNET_E_LAUNCH, "probe: copying %s failed", what);
    return AMPNET_OK;
}

// every argmax entry is -1 or a row of its own window (the kernels gather z_prev[arg] and write out[arg])
int check_arg(const AmpnetPooledBwdProbe *d, const std::vector<int32_t> &wo, hipStream_t st)
{
    const int64_t n = (int64_t)d->Q * d->C;
    AMPNET_REQUIRE(d->arg && d->arg_n >= n, "probe_pooled_bwd: arg [Q, C] short");
    std::vector<int32_t> h;
    if (int rc = to_host(d->arg, n, h, st, "arg"); rc != AMPNET_OK) return rc;
    for (int q = 0; q < d->Q; ++q)
        for (int c = 0; c < d->C; ++c) {
            const int r = h[(size_t)q * d->C + c];
            AMPNET_REQUIRE(r == -1 || (r >= wo[q] && r < wo[q + 1]), "probe_pooled_bwd: arg[%d][%d] = %d outside window [%d, %d)", q, c, r, wo[q], wo[q + 1]);
        }
    return AMPNET_OK;
}
}  // namespace
}  // namespace ampnet

extern "C" int ampnet_probe_pooled_bwd_f32(const AmpnetPooledBwdProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_pooled_bwd: null descriptor");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AMPNET_REQUIRE(d->op >= 0 && d->op <= 7, "probe_pooled_bwd: op %d not built", d->op);
    AMPNET_REQUIRE(d->Q >= 1 && d->n_slots >= 1 && d->Q % d->n_slots == 0 && d->C >= 1 && d->C <= 256 && d->cp >= 1 && d->cp <= 128,
                   "probe_pooled_bwd: bad sizes (Q %d, n_slots %d, C %d, cp %d)", d->Q, d->n_slots, d->C, d->cp);
    const int64_t Q = d->Q, S = d->n_slots, C = d->C, cp = d->cp;
    if (d->op == 6 || d->op == 7) {
        AMPNET_REQUIRE(d->chunks >= 1 && d->red_n0 >= 1 && d->red_part0 && d->red_out0 && d->red_part0_n >= Q * d->chunks * d->red_n0 &&
                           d->red_out0_n >= S * d->red_n0,
                       "probe_pooled_bwd: reduce_slots pair 0 short");
        if (d->op == 6) return reduce_slots(d->red_part0, d->Q, d->chunks, d->n_slots, d->red_n0, d->red_out0, st);
        AMPNET_REQUIRE(d->red_n1 >= 1 && d->red_part1 && d->red_out1 && d->red_part1_n >= Q * d->chunks * d->red_n1 && d->red_out1_n >= S * d->red_n1,
                       "probe_pooled_bwd: reduce_slots pair 1 short");
        return reduce_slots2(d->red_part0, d->red_n0, d->red_out0, d->red_part1, d->red_n1, d->red_out1, d->Q, d->chunks, d->n_slots, st);
    }
    if (d->op == 1) {
        AMPNET_REQUIRE(d->W && d->W_n >= C * cp && d->P2 && d->P3 && d->P_n >= S * C && d->G && d->G_n >= S * cp * cp && d->c0 && d->c0_n >= S * cp,
                       "probe_pooled_bwd: slot_mats buffers short");
        return slot_mats(d->W, d->P2, d->P3, d->n_slots, d->C, d->cp, d->G, d->c0, st);
    }
    int64_t rows = 0;
    int max_rows = 0;
    if (int rc = read_win_off(d->win_off, d->win_off_n, d->Q, st, rows, max_rows); rc != AMPNET_OK) return rc;
    std::vector<int32_t> wo;
    if (int rc = to_host(d->win_off, Q + 1, wo, st, "win_off"); rc != AMPNET_OK) return rc;
    // what the sparse ops read per window: arg, dpm (row prow(q) < Q), P1 [S, C], W [C, cp]
    const bool zprev_op = d->op == 2 || d->op == 4 || d->op == 5;
    if (zprev_op) {
        AMPNET_REQUIRE(d->z_prev && d->z_prev_n >= rows * cp, "probe_pooled_bwd: z_prev [rows, cp] short");
        AMPNET_REQUIRE(d->s_prev && d->t_prev && d->prev_n >= S * cp, "probe_pooled_bwd: s_prev / t_prev short");
        AMPNET_REQUIRE(d->op == 5 || (d->mean_prev && d->invstd_prev), "probe_pooled_bwd: mean_prev / invstd_prev missing");
        AMPNET_REQUIRE(!d->z_bf16 || d->op != 4, "probe_pooled_bwd: sparse_fix reads fp32 z_prev only");
    }
    if (d->op == 2 || d->op == 4) {
        AMPNET_REQUIRE(d->out && d->out_n >= rows * cp, "probe_pooled_bwd: out [rows, cp] short");
        AMPNET_REQUIRE(d->part_chunks >= 1 && d->slot_idx >= 0 && d->slot_idx < d->part_chunks, "probe_pooled_bwd: slot_idx %d outside part_chunks %d",
                       d->slot_idx, d->part_chunks);
        AMPNET_REQUIRE(d->part_a && d->part_b && d->part_n >= Q * d->part_chunks * cp, "probe_pooled_bwd: part_a / part_b short");
    }
    if (d->op != 4) {
        if (int rc = check_arg(d, wo, st); rc != AMPNET_OK) return rc;
        AMPNET_REQUIRE(d->dpm && d->qc_n >= Q * C, "probe_pooled_bwd: dpm [Q, C] short");
    }
    if (d->op == 2 || d->op == 3 || d->op == 5) {
        AMPNET_REQUIRE(d->P1 && d->P_n >= S * C && d->W && d->W_n >= C * cp, "probe_pooled_bwd: P1 / W short");
    }
    switch (d->op) {
    case 0: {
        AMPNET_REQUIRE(d->zext && d->d_pooled && d->qc_n >= Q * C, "probe_pooled_bwd: zext / d_pooled short");
        AMPNET_REQUIRE(d->scale && d->shift && d->mean && d->invstd && d->bn_n >= S * C, "probe_pooled_bwd: BatchNorm constants short");
        AMPNET_REQUIRE(d->P1 && d->P2 && d->P3 && d->P_n >= S * C && d->slot_ab && d->slot_ab_n >= 2 * S * C, "probe_pooled_bwd: P1..P3 / slot_ab short");
        PoolBwd p;
        p.d_pooled = d->d_pooled; p.slot_major = d->slot_major; p.arg = d->arg; p.zext = d->zext;
        p.fwd.scale = ro(d->scale); p.fwd.shift = ro(d->shift); p.fwd.mean = ro(d->mean); p.fwd.invstd = ro(d->invstd);
        p.win_off = d->win_off; p.Q = d->Q; p.n_slots = d->n_slots; p.C = d->C;
        p.dpm = d->dpm; p.out = BnBwd{d->P1, d->P2, d->P3, d->slot_ab};
        return pool_bwd(p, st);
    }
    case 2: {
        SparseScatter a;
        a.z_bf16 = d->z_bf16 ? 1 : 0; a.arg = d->arg; a.dpm = d->dpm; a.slot_major = d->slot_major; a.P1 = d->P1; a.W = d->W;
        a.z_prev = d->z_prev; a.s_prev = d->s_prev; a.t_prev = d->t_prev; a.mean_prev = d->mean_prev; a.invstd_prev = d->invstd_prev;
        a.Q = d->Q; a.n_slots = d->n_slots; a.C = d->C; a.cp = d->cp; a.out = d->out;
        a.part_a = d->part_a; a.part_b = d->part_b; a.part_chunks = d->part_chunks; a.slot_idx = d->slot_idx;
        return sparse_scatter(a, st);
    }
    case 3: {
        AMPNET_REQUIRE(d->cp % 4 == 0 && 256 % (d->cp / 4) == 0, "probe_pooled_bwd: sparse_rows cp %d", d->cp);
        AMPNET_REQUIRE(d->srows && d->srows_n >= Q * C * cp && d->srow_row && d->srow_row_n >= Q * C && d->srow_cnt && d->srow_cnt_n >= Q,
                       "probe_pooled_bwd: srows / srow_row / srow_cnt short");
        SparseRows a;
        a.arg = d->arg; a.dpm = d->dpm; a.slot_major = d->slot_major; a.P1 = d->P1; a.W = d->W;
        a.Q = d->Q; a.n_slots = d->n_slots; a.C = d->C; a.cp = d->cp;
        a.srows = d->srows; a.srow_row = d->srow_row; a.srow_cnt = d->srow_cnt;
        return sparse_rows(a, st);
    }
    case 4: {
        AMPNET_REQUIRE(d->srows && d->srows_n >= Q * C * cp && d->srow_row && d->srow_row_n >= Q * C && d->srow_cnt && d->srow_cnt_n >= Q,
                       "probe_pooled_bwd: srows / srow_row / srow_cnt short");
        // the merged rows name rows of z_prev / out: each of the first srow_cnt[q] must lie in window q
        std::vector<int32_t> cnt, rr;
        if (int rc = to_host(d->srow_cnt, Q, cnt, st, "srow_cnt"); rc != AMPNET_OK) return rc;
        if (int rc = to_host(d->srow_row, Q * C, rr, st, "srow_row"); rc != AMPNET_OK) return rc;
        for (int q = 0; q < d->Q; ++q) {
            AMPNET_REQUIRE(cnt[q] >= 0 && cnt[q] <= d->C, "probe_pooled_bwd: srow_cnt[%d] = %d", q, cnt[q]);
            for (int i = 0; i < cnt[q]; ++i) {
                const int r = rr[(size_t)q * d->C + i];
                AMPNET_REQUIRE(r >= wo[q] && r < wo[q + 1], "probe_pooled_bwd: srow_row[%d][%d] = %d outside its window", q, i, r);
            }
        }
        SparseFix a;
        a.srows = d->srows; a.srow_row = d->srow_row; a.srow_cnt = d->srow_cnt; a.z_prev = d->z_prev;
        a.s_prev = d->s_prev; a.t_prev = d->t_prev; a.mean_prev = d->mean_prev; a.invstd_prev = d->invstd_prev;
        a.Q = d->Q; a.n_slots = d->n_slots; a.C = d->C; a.cp = d->cp; a.out = d->out;
        a.part_a = d->part_a; a.part_b = d->part_b; a.part_chunks = d->part_chunks; a.slot_idx = d->slot_idx;
        return sparse_fix(a, st);
    }
    default: {   // 5
        AMPNET_REQUIRE(d->P2 && d->P3, "probe_pooled_bwd: P2 / P3 missing");
        AMPNET_REQUIRE(d->gram && d->gram_n >= S * cp * cp && d->asum && d->asum_n >= S * cp, "probe_pooled_bwd: gram / asum short");
        AMPNET_REQUIRE(d->dW && d->dW_n >= C * cp, "probe_pooled_bwd: dW short");
        AMPNET_REQUIRE(((size_t)Q * 2 + (size_t)S * cp * 2) * sizeof(int) <= 60 * 1024, "probe_pooled_bwd: pooled_wgrad needs more than 60 KB of LDS");
        AMPNET_REQUIRE(!d->wgram || (d->n_slots <= 10 /* SG_MAX_PROBLEMS */ && d->wgram_n >= S * C * cp), "probe_pooled_bwd: wgram short");
        PooledWgrad a;
        a.z_bf16 = d->z_bf16 ? 1 : 0; a.W = d->W; a.P1 = d->P1; a.P2 = d->P2; a.P3 = d->P3; a.gram = d->gram; a.asum = d->asum;
        a.arg = d->arg; a.dpm = d->dpm; a.slot_major = d->slot_major;
        a.z_prev = d->z_prev; a.s_prev = d->s_prev; a.t_prev = d->t_prev;
        a.Q = d->Q; a.n_slots = d->n_slots; a.C = d->C; a.cp = d->cp; a.dW = d->dW; a.wgram = d->wgram;
        return pooled_wgrad(a, st);
    }
    }
}

extern "C" int ampnet_probe_input_wgrad_f32(const AmpnetInputWgradProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_input_wgrad: null descriptor");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AMPNET_REQUIRE((d->op == 0 || d->op == 1) && (d->mode == 0 || d->mode == 1) && d->Q >= 1 && d->n_slots >= 1 && d->Q % d->n_slots == 0,
                   "probe_input_wgrad: bad op / mode / sizes");
    const int64_t Q = d->Q, S = d->n_slots, nw = d->mode ? 12 : 3;
    AMPNET_REQUIRE(d->W && d->W_n >= 64 * nw, "probe_input_wgrad: W short");
    AMPNET_REQUIRE(d->mode == 0 || (d->T && d->T_n >= Q * 9), "probe_input_wgrad: T short");
    AMPNET_REQUIRE(d->dWeff && d->dWeff_n >= Q * 64 * 9, "probe_input_wgrad: dWeff short");
    if (d->op == 1) {
        AMPNET_REQUIRE(d->dW && d->dW_n >= 64 * nw && (d->mode == 0 || (d->dT && d->dT_n >= Q * 9)), "probe_input_wgrad: dW / dT short");
        return input_param_grads(d->dWeff, d->W, d->mode ? d->T : nullptr, d->Q, d->n_slots, d->perwin_slot_major, d->mode, d->dW,
                                 d->mode ? d->dT : nullptr, st);
    }
    int64_t rows = 0;
    int max_rows = 0;
    if (int rc = read_win_off(d->win_off, d->win_off_n, d->Q, st, rows, max_rows); rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE(d->x && d->x_n >= rows * 9 && d->dy && d->dy_n >= rows * 64, "probe_input_wgrad: x / dy short");
    if (d->fin_part_a) {
        AMPNET_REQUIRE(d->fin_part_b && d->fin_parts >= d->n_slots && d->fin_part_n >= (int64_t)d->fin_parts * 64 && d->fin_rows >= 1 &&
                           d->fin_gamma && d->fin_gamma_n >= 64 && d->fin_mean && d->fin_invstd && d->fin_in_n >= S * 64 && d->fin_P1 &&
                           d->fin_P2 && d->fin_P3 && d->fin_slot_ab && d->fin_out_n >= 2 * S * 64,
                       "probe_input_wgrad: fin_* short");
    } else {
        AMPNET_REQUIRE(d->P1 && d->P2 && d->P3 && d->P_n >= S * 64, "probe_input_wgrad: P1..P3 short");
    }
    PwInputWgrad a;
    a.x = d->x; a.dy = d->dy; a.W = d->W; a.T = d->mode ? d->T : nullptr; a.mode = d->mode; a.perwin_slot_major = d->perwin_slot_major;
    a.fin = BnBwdFin{d->fin_part_a, d->fin_part_b, d->fin_parts, d->fin_rows, d->fin_gamma, d->fin_mean, d->fin_invstd,
                     {d->fin_P1, d->fin_P2, d->fin_P3, d->fin_slot_ab}};
    if (!d->fin_part_a) {
        a.bn.P1 = ro(d->P1); a.bn.P2 = ro(d->P2); a.bn.P3 = ro(d->P3);
    }
    a.dWeff = d->dWeff; a.win_off = d->win_off; a.Q = d->Q; a.n_slots = d->n_slots;
    return pw_input_wgrad(a, st);
}

// ---- the head's kernels, the loss tail and the token path's small GEMMs (tests/test_head_layers_gpu.py) ------------------------------------
namespace ampnet {
namespace {
// op 7: y[0][i] = __expf(x[i]) (attention_core), y[1][i] = expf(x[i]), y[2][i] = logf(x[i]) (head_logits, ce_bwd): the functions the softmax bars rest on
__global__ __launch_bounds__(256) void exp_log_sweep_kernel(const float *__restrict__ x, float *__restrict__ y, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[i] = __expf(x[i]);
    y[(size_t)n + i] = expf(x[i]);
    y[2 * (size_t)n + i] = logf(x[i]);
}
}  // namespace
}  // namespace ampnet

extern "C" int ampnet_probe_head_f32(const AmpnetHeadProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_head: null descriptor");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AMPNET_REQUIRE(d->op >= 0 && d->op <= 7, "probe_head: op %d not built", d->op);
    AMPNET_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "probe_head: drop_p %f", (double)d->drop_p);
    if (d->op == 7) {
        AMPNET_REQUIRE(d->rows >= 1 && d->rows <= (1 << 24) && d->X && d->X_n >= d->rows && d->dX && d->dX_n >= 3 * (int64_t)d->rows, "probe_head: sweep buffers short");
        ProfScope prof("exp_log_sweep", 0.0, 0.0, st);
        hipLaunchKernelGGL(exp_log_sweep_kernel, dim3(cdiv(d->rows, 256)), dim3(256), 0, st, d->X, d->dX, d->rows);
        return check_launch("exp_log_sweep_kernel");
    }
    switch (d->op) {
    case 0: {
        AMPNET_REQUIRE(d->Q >= 1 && d->Q <= (1 << 20), "probe_head: Q %d", d->Q);
        const int64_t Q = d->Q;
        AMPNET_REQUIRE(d->gl && d->gl_n >= Q * HEAD_E && d->cent && d->cent_n >= Q * 2, "probe_head: gl / cent short");
        AMPNET_REQUIRE(d->w1 && d->w1_n >= 32 && d->b1 && d->b1_n >= 16 && d->w2 && d->w2_n >= HEAD_E * 16 && d->b2 && d->b2_n >= HEAD_E,
                       "probe_head: positional-encoding parameters short");
        AMPNET_REQUIRE(d->tok && d->tok_n >= Q * HEAD_E, "probe_head: tok short");
        AMPNET_REQUIRE((d->hid == nullptr) == (d->slope == nullptr) && (!d->hid || d->hid_n >= Q * 16), "probe_head: hid / slope short");
        ProfScope prof("posenc_tokens", 0.0, 0.0, st);
        return posenc_tokens(d->gl, d->cent, d->w1, d->b1, d->w2, d->b2, d->tok, d->Q, st, d->hid, d->slope);
    }
    case 1:
    case 2: {
        AMPNET_REQUIRE(d->B >= 1 && d->B <= 65535 && d->W >= 1 && d->W <= HEAD_MAX_W, "probe_head: B %d, W %d (1 <= W <= %d)", d->B, d->W, HEAD_MAX_W);
        const int64_t BW = (int64_t)d->B * d->W, np = (int64_t)d->B * HEAD_HEADS * d->W * d->W;
        AMPNET_REQUIRE(d->qkv && d->qkv_n >= BW * 3 * HEAD_E, "probe_head: qkv short");
        if (d->op == 1) {
            AMPNET_REQUIRE(!d->mask || d->mask_n >= BW, "probe_head: mask short");
            AMPNET_REQUIRE(!d->probs || d->probs_n >= np, "probe_head: probs short");
            AMPNET_REQUIRE(d->ctx && d->ctx_n >= BW * HEAD_E, "probe_head: ctx short");
            ProfScope prof("attention_core", 0.0, 0.0, st);
            return attention_core(d->qkv, d->mask, d->probs, d->ctx, d->B, d->W, d->drop_p, d->drop_seed, st);
        }
        AMPNET_REQUIRE(d->probs && d->probs_n >= np, "probe_head: probs short");
        AMPNET_REQUIRE(d->dctx && d->dctx_n >= BW * HEAD_E && d->dqkv && d->dqkv_n >= BW * 3 * HEAD_E, "probe_head: dctx / dqkv short");
        ProfScope prof("attention_core_bwd", 0.0, 0.0, st);
        return attention_core_bwd(d->qkv, d->probs, d->dctx, d->dqkv, d->B, d->W, d->drop_p, d->drop_seed, st);
    }
    case 3:
    case 4: {
        AMPNET_REQUIRE(d->C >= 1 && d->C <= HEAD_MAX_CLASSES, "probe_head: %d classes, supported 1..%d", d->C, HEAD_MAX_CLASSES);
        AMPNET_REQUIRE(d->R >= 1 && d->P >= 1 && d->R % d->P == 0, "probe_head: rows %d not a multiple of points per sample %d", d->R, d->P);
        const int64_t R = d->R, C = d->C;
        if (d->op == 3) {
            const int64_t blocks = cdiv(d->R, HEAD_LOGITS_ROWS);
            AMPNET_REQUIRE(d->z4 && covers(d->z4_n, R, d->ldz4, C), "probe_head: z4 [%d, %d] short", d->R, d->ldz4);
            AMPNET_REQUIRE(d->logits && d->logits_n >= R * C, "probe_head: logits short");
            AMPNET_REQUIRE(!d->targets || d->targets_n >= R, "probe_head: targets short");
            AMPNET_REQUIRE(!d->class_w || d->class_w_n >= C, "probe_head: class_w short");
            AMPNET_REQUIRE(!d->preds || d->preds_n >= R, "probe_head: preds short");
            AMPNET_REQUIRE(!d->loss_part || d->loss_part_n >= blocks * 2, "probe_head: loss_part short");
            AMPNET_REQUIRE(!d->loss_out || (d->loss_out_n >= 2 && d->loss_part && d->targets), "probe_head: loss_out needs 2 floats, loss_part and targets");
            HeadOut o;
            o.R = d->R; o.P = d->P; o.C = d->C;
            o.logits = d->logits; o.targets = d->targets; o.class_w = d->class_w; o.preds = d->preds;
            o.loss_part = d->targets ? d->loss_part : nullptr;
            int nb = 0;
            {
                ProfScope prof("head_logits", 0.0, 0.0, st);
                if (int rc = head_logits(o, d->z4, d->ldz4, &nb, st); rc != AMPNET_OK) return rc;
            }
            if (!d->loss_out) return AMPNET_OK;
            ProfScope prof("loss_finalize", 0.0, 0.0, st);
            return loss_finalize(d->loss_part, nb, d->loss_out, st);
        }
        const int64_t blocks = cdiv(d->R, HEAD_OUT_BWD_ROWS);
        AMPNET_REQUIRE(d->dlogits && d->dlogits_n >= R * C, "probe_head: dlogits short");
        AMPNET_REQUIRE(d->z3 && d->z3_n >= R * 64, "probe_head: z3 [%d, 64] short", d->R);
        AMPNET_REQUIRE(d->scale && d->shift && d->mean && d->invstd && d->bn_n >= 64, "probe_head: bn_3 constants short");
        AMPNET_REQUIRE(d->w4 && d->w4_n >= C * 64, "probe_head: w4 short");
        AMPNET_REQUIRE(d->dy3 && d->dy3_n >= R * 64, "probe_head: dy3 short");
        AMPNET_REQUIRE(d->part_a && d->part_b && d->part_n >= blocks * 64, "probe_head: part_a / part_b short (%lld workgroups)", (long long)blocks);
        AMPNET_REQUIRE(d->w4part && d->w4part_n >= blocks * (C * 64 + C), "probe_head: w4part short");
        HeadOutBwd o;
        o.dlogits = d->dlogits; o.z3 = d->z3; o.z_bf16 = d->z_bf16 ? 1 : 0;
        o.bn.scale = ro(d->scale); o.bn.shift = ro(d->shift); o.bn.mean = ro(d->mean); o.bn.invstd = ro(d->invstd);
        o.W = d->w4; o.drop_p = d->drop_p; o.drop_seed = d->drop_seed;
        o.R = d->R; o.P = d->P; o.C = d->C;
        o.dy3 = d->dy3; o.part_a = d->part_a; o.part_b = d->part_b; o.dWpart = d->w4part;
        ProfScope prof(o.z_bf16 ? "head_out_bwd<bf16>" : "head_out_bwd<f32>", 0.0, 0.0, st);
        return head_out_bwd(o, st);
    }
    default: {   // 5, 6
        AMPNET_REQUIRE(d->rows >= 1 && d->n_out >= 1 && d->n_in >= 1 && d->rows <= (1 << 20) && d->n_out <= 8192 && d->n_in <= 8192,
                       "probe_head: rows %d, n_out %d, n_in %d", d->rows, d->n_out, d->n_in);
        const int64_t rows = d->rows, no = d->n_out, ni = d->n_in;
        AMPNET_REQUIRE(d->G && covers(d->G_n, rows, d->ldg, no) && d->X && covers(d->X_n, rows, d->ldx, ni), "probe_head: G / X short");
        AMPNET_REQUIRE(d->dW && covers(d->dW_n, no, d->lddw, ni), "probe_head: dW short");
        AMPNET_REQUIRE(!d->db || d->db_n >= no, "probe_head: db short");
        if (d->op == 6) {
            AMPNET_REQUIRE(d->db, "probe_head: sgemm_wgrad_bias writes db");
            return sgemm_wgrad_bias(d->rows, d->n_out, d->n_in, d->G, d->ldg, d->X, d->ldx, d->dW, d->lddw, d->db, st);
        }
        AMPNET_REQUIRE(d->Wl && covers(d->Wl_n, no, d->ldw, ni), "probe_head: W short");
        AMPNET_REQUIRE(d->dX && covers(d->dX_n, rows, d->lddx, ni), "probe_head: dX short");
        AMPNET_REQUIRE(!d->dx_mul || covers(d->dx_mul_n, rows, d->lddx, ni), "probe_head: dx_mul short");
        LinBwdOpt o;
        o.db = d->db;
        o.dx_mul = d->dx_mul;
        return sgemm_linear_bwd(d->rows, d->n_out, d->n_in, d->G, d->ldg, d->X, d->ldx, d->Wl, d->ldw, d->dW, d->lddw, d->dX, d->lddx, st, o);
    }
    }
}

// ---- the BatchNorm / pooling glue kernels (tests/test_bn_glue_gpu.py, tests/test_syncbn_layers_gpu.py) -------------------------------------
// One launch of a kernel of pw_misc.hip, of a small kernel of bwd_misc.hip or of reduce_windows (pw_bwd.hip), or of its host entry point.  The
// host entry points branch on an installed collective (sync_bn_on()).  Ops 1 (bn_finalize), 6 (bn_bwd_finalize) and 10 (fc_bn_bwd) run with one
// installed, through the same entry points: they then take the global-batch branch (one exchange each, so every rank must make the same calls).
// Every other op is about the single-process form and refuses to run then.
namespace ampnet {
namespace {

constexpr int64_t BIG = 1 << 26;       // no probe buffer is larger than this many elements: index arithmetic in int stays exact

template <typename T> int bn_to_host(const T *src, int64_t n, std::vector<T> &h, hipStream_t st, const char *what)
{
    h.resize((size_t)n);
    if (n > 0 && (hipMemcpyAsync(h.data(), src, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
        return fail(AMPNET_E_LAUNCH, "probe_bn: copying %s failed", what);
    return AMPNET_OK;
}

// win_off on the host: Q + 1 ascending values from 0 up
int bn_win_off(const AmpnetBnProbe *d, hipStream_t st, std::vector<int32_t> &wo, int64_t &rows, int &max_rows)
{
    AMPNET_REQUIRE(d->win_off && d->win_off_n >= (int64_t)d->Q + 1, "probe_bn: win_off needs Q + 1 = %d entries (has %lld)", d->Q + 1, (long long)d->win_off_n);
    if (int rc = bn_to_host(d->win_off, (int64_t)d->Q + 1, wo, st, "win_off"); rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE(wo[0] == 0, "probe_bn: win_off[0] = %d != 0", wo[0]);
    max_rows = 0;
    for (int q = 0; q < d->Q; ++q) {
        AMPNET_REQUIRE(wo[q + 1] >= wo[q], "probe_bn: win_off not ascending at %d", q);
        if (wo[q + 1] - wo[q] > max_rows) max_rows = wo[q + 1] - wo[q];
    }
    rows = wo[d->Q];
    AMPNET_REQUIRE(rows <= BIG, "probe_bn: %lld rows", (long long)rows);
    return AMPNET_OK;
}

bool covers2(int64_t n, int64_t rows, int64_t ld, int64_t cols) { return rows <= 0 || (ld >= cols && n >= (rows - 1) * ld + cols); }

// the item offsets of ops 3, 4, 7: item i starts at sum_{j<i} it_C[j]; returns the total, -1 if an item is out of range
int64_t item_total(const AmpnetBnProbe *d, int n)
{
    int64_t t = 0;
    for (int i = 0; i < n; ++i) {
        if (d->it_C[i] < 1 || d->it_C[i] > 4096) return -1;
        t += d->it_C[i];
    }
    return t;
}

int probe_pw_input(const AmpnetBnProbe *d, hipStream_t st)
{
    AMPNET_REQUIRE((d->mode == 0 || d->mode == 1) && d->Q >= 1 && d->Q <= (1 << 16) && d->n_slots >= 1 && d->chunks >= 1 && d->chunks <= 64 && d->chunk_rows >= 1,
                   "probe_bn: pw_input sizes");
    AMPNET_REQUIRE(!(d->mode == 1 && d->perwin_slot_major) || d->Q % d->n_slots == 0, "probe_bn: pw_input slot-major T needs Q %% n_slots == 0");
    std::vector<int32_t> wo;
    int64_t rows = 0;
    int max_rows = 0;
    if (int rc = bn_win_off(d, st, wo, rows, max_rows); rc != AMPNET_OK) return rc;
    AMPNET_REQUIRE((int64_t)d->chunks * d->chunk_rows >= max_rows, "probe_bn: pw_input %d chunks of %d rows do not cover a window of %d rows", d->chunks,
                   d->chunk_rows, max_rows);
    const int64_t Q = d->Q, S = d->n_slots;
    AMPNET_REQUIRE(d->x && d->x_n >= rows * 9, "probe_bn: x [rows, 9] short");
    AMPNET_REQUIRE(d->W && d->W_n >= (d->mode ? 64 * 12 : 64 * 3), "probe_bn: pw_input W short");
    AMPNET_REQUIRE(d->mode == 0 || (d->T && d->T_n >= Q * 9), "probe_bn: T [Q, 9] short");
    AMPNET_REQUIRE(d->Z && d->Z_n >= rows * 64, "probe_bn: Z [rows, 64] short");
    AMPNET_REQUIRE((d->part_sum == nullptr) == (d->part_sq == nullptr), "probe_bn: part_sum and part_sq come together");
    if (d->part_rows) {
        AMPNET_REQUIRE(d->part_sum && d->stat_lanes >= d->n_slots && d->stat_lanes <= 2048, "probe_bn: pw_input stat_lanes %d", d->stat_lanes);
        const int64_t parts = (int64_t)cdiv(d->stat_lanes, d->n_slots) * S;
        AMPNET_REQUIRE(d->part_sum_n >= parts * 64 && d->part_sq_n >= parts * 64 && d->part_rows_n >= parts, "probe_bn: pw_input per-workgroup partials short");
    } else if (d->part_sum) {
        AMPNET_REQUIRE(d->part_sum_n >= Q * d->chunks * 64 && d->part_sq_n >= Q * d->chunks * 64, "probe_bn: pw_input per-chunk partials short");
    }
    PwInput a;
    a.x = d->x; a.W = d->W; a.T = d->mode ? d->T : nullptr; a.mode = d->mode; a.perwin_slot_major = d->perwin_slot_major; a.n_slots = d->n_slots;
    a.Z = d->Z; a.z_bf16 = d->z_bf16 ? 1 : 0; a.part_sum = d->part_sum; a.part_sq = d->part_sq; a.part_rows = d->part_rows;
    a.stat_lanes = d->stat_lanes; a.win_off = d->win_off; a.Q = d->Q; a.chunk_rows = d->chunk_rows; a.chunks = d->chunks;
    return pw_input(a, st);
}

int probe_bn_finalize(const AmpnetBnProbe *d, hipStream_t st)
{
    AMPNET_REQUIRE(d->n_slots >= 1 && d->n_slots <= 4096 && d->C >= 1 && d->C <= 4096, "probe_bn: bn_finalize sizes");
    const int64_t S = d->n_slots, C = d->C;
    AMPNET_REQUIRE(d->gamma && d->gamma_n >= C && d->beta && d->beta_n >= C, "probe_bn: gamma / beta [C] short");
    AMPNET_REQUIRE(d->scale && d->scale_n >= S * C && d->shift && d->shift_n >= S * C, "probe_bn: scale / shift [n_slots, C] short");
    AMPNET_REQUIRE((!d->mean || d->mean_n >= S * C) && (!d->invstd || d->invstd_n >= S * C), "probe_bn: mean / invstd short");
    AMPNET_REQUIRE((d->stat_mean == nullptr) == (d->stat_uvar == nullptr) && (!d->stat_mean || (d->stat_mean_n >= S * C && d->stat_uvar_n >= S * C)),
                   "probe_bn: stat_mean / stat_uvar short");
    BnFinalize a;
    a.n_slots = d->n_slots; a.C = d->C; a.layer = BnLayer{d->gamma, d->beta}; a.eps = d->eps;
    a.out = BnFwd{d->scale, d->shift, d->mean, d->invstd, d->stat_mean, d->stat_uvar};
    if (d->op == 2) {
        const int64_t body = S * (2 * C + 1);
        AMPNET_REQUIRE(d->gather_ranks >= 1 && d->gather_ranks <= 64 && d->gather_seg >= body, "probe_bn: gather_ranks %d, gather_seg %lld", d->gather_ranks,
                       (long long)d->gather_seg);
        AMPNET_REQUIRE(d->part_sum && d->part_sum_n >= (d->gather_ranks - 1) * d->gather_seg + body, "probe_bn: gathered segments short");
        return bn_finalize_gathered(a, d->part_sum, d->gather_ranks, (size_t)d->gather_seg, st);
    }
    AMPNET_REQUIRE(d->Q >= 1 && d->Q <= (1 << 20) && d->chunks >= 1 && d->chunks <= 64 && d->chunk_rows >= 1 && d->uniform_rows >= 0, "probe_bn: bn_finalize sizes");
    const int64_t parts = (int64_t)d->Q * d->chunks;
    AMPNET_REQUIRE(parts * C <= BIG, "probe_bn: bn_finalize partials too large");
    AMPNET_REQUIRE(d->part_sum && d->part_sum_n >= parts * C && d->part_sq && d->part_sq_n >= parts * C, "probe_bn: part_sum / part_sq [Q * chunks, C] short");
    if (d->part_rows) {
        AMPNET_REQUIRE(d->part_rows_n >= parts, "probe_bn: part_rows [Q * chunks] short");
    } else if (d->uniform_rows > 0) {
        AMPNET_REQUIRE((int64_t)d->chunks * d->chunk_rows >= d->uniform_rows, "probe_bn: chunks do not cover uniform_rows");
    } else {
        std::vector<int32_t> wo;
        int64_t rows = 0;
        int max_rows = 0;
        if (int rc = bn_win_off(d, st, wo, rows, max_rows); rc != AMPNET_OK) return rc;
        AMPNET_REQUIRE((int64_t)d->chunks * d->chunk_rows >= max_rows, "probe_bn: chunks do not cover a window of %d rows", max_rows);
    }
    AMPNET_REQUIRE(!d->merge_ws || d->merge_ws_n >= (int64_t)bn_finalize_merge_floats(d->n_slots, d->C), "probe_bn: merge_ws short");
    a.part = BnPartials{d->part_sum, d->part_sq, d->part_rows, d->Q * d->chunks}; a.chunk_rows = d->chunk_rows;
    a.uniform_rows = d->part_rows ? 0 : d->uniform_rows; a.win_off = (d->part_rows || d->uniform_rows > 0) ? nullptr : d->win_off;
    a.Q = d->Q; a.chunks = d->chunks; a.merge_ws = d->merge_ws;
    return bn_finalize(a, st);
}

int probe_items(const AmpnetBnProbe *d, hipStream_t st)
{
    AMPNET_REQUIRE(d->n_items >= 1 && d->n_items <= AMPNET_BN_PROBE_ITEMS && d->n_slots >= 1 && d->n_slots <= 64, "probe_bn: %d items, %d slots", d->n_items, d->n_slots);
    const int n = d->n_items;
    const int64_t tot = item_total(d, n), S = d->n_slots;
    AMPNET_REQUIRE(tot > 0, "probe_bn: it_C out of range");
    if (d->op == 3) {
        AMPNET_REQUIRE(d->gamma && d->gamma_n >= tot && d->beta && d->beta_n >= tot && d->rmean && d->rmean_n >= tot && d->rvar && d->rvar_n >= tot &&
                           d->scale && d->scale_n >= tot && d->shift && d->shift_n >= tot,
                       "probe_bn: bn_fold arrays short (%lld channels)", (long long)tot);
        BnFoldItem it[AMPNET_BN_PROBE_ITEMS];
        int64_t o = 0;
        for (int i = 0; i < n; o += d->it_C[i], ++i) it[i] = {d->gamma + o, d->beta + o, d->rmean + o, d->rvar + o, d->scale + o, d->shift + o, d->it_C[i]};
        return bn_fold(it, n, d->eps, st);
    }
    if (d->op == 4) {
        AMPNET_REQUIRE(d->stat_mean && d->stat_mean_n >= S * tot && d->stat_uvar && d->stat_uvar_n >= S * tot && d->rmean && d->rmean_n >= tot && d->rvar &&
                           d->rvar_n >= tot,
                       "probe_bn: bn_running_update arrays short");
        BnRunItem it[AMPNET_BN_PROBE_ITEMS];
        int64_t o = 0;
        for (int i = 0; i < n; o += d->it_C[i], ++i) it[i] = {d->stat_mean + S * o, d->stat_uvar + S * o, d->rmean + o, d->rvar + o, d->it_C[i], d->n_slots};
        return bn_running_update(it, n, d->momentum, st);
    }
    AMPNET_REQUIRE(d->slot_ab && d->slot_ab_n >= 2 * S * tot && d->dgamma && d->dgamma_n >= tot && d->dbeta && d->dbeta_n >= tot, "probe_bn: bn_param_grads arrays short");
    BnGradItem it[AMPNET_BN_PROBE_ITEMS];
    int64_t o = 0;
    for (int i = 0; i < n; o += d->it_C[i], ++i) it[i] = {d->slot_ab + 2 * S * o, d->dgamma + o, d->dbeta + o, d->it_C[i], d->n_slots};
    return bn_param_grads(it, n, st);
}

int probe_pool_finalize(const AmpnetBnProbe *d, hipStream_t st)
{
    AMPNET_REQUIRE((d->mode == 0 || d->mode == 1) && d->Q >= 1 && d->Q <= (1 << 16) && d->n_slots >= 1 && d->n_slots <= d->Q && d->C >= 1 && d->C <= 4096 &&
                       d->chunks >= 1 && d->chunks <= 64,
                   "probe_bn: pool_finalize sizes");
    AMPNET_REQUIRE(!d->out_slot_major || d->Q % d->n_slots == 0, "probe_bn: pool_finalize slot-major output needs Q %% n_slots == 0");
    const int64_t Q = d->Q, S = d->n_slots, C = d->C, parts = Q * d->chunks;
    AMPNET_REQUIRE(d->part_max && d->part_max_n >= parts * C, "probe_bn: part_max [Q * chunks, C] short");
    AMPNET_REQUIRE(d->pooled && d->pooled_n >= Q * C && (!d->arg || d->arg_n >= Q * C) && (!d->zext || d->zext_n >= Q * C), "probe_bn: pooled / arg / zext [Q, C] short");
    AMPNET_REQUIRE(d->scale && d->scale_n >= S * C && d->shift && d->shift_n >= S * C, "probe_bn: scale / shift [n_slots, C] short");
    AMPNET_REQUIRE(d->part_amax || !d->arg, "probe_bn: arg without part_amax");
    if (d->part_amax) {
        AMPNET_REQUIRE(d->part_amax_n >= parts * C, "probe_bn: part_amax short");
        std::vector<int32_t> wo, am;
        int64_t rows = 0;
        int max_rows = 0;
        if (int rc = bn_win_off(d, st, wo, rows, max_rows); rc != AMPNET_OK) return rc;
        if (int rc = bn_to_host(d->part_amax, parts * C, am, st, "part_amax"); rc != AMPNET_OK) return rc;
        for (int64_t p = 0; p < parts; ++p)
            for (int64_t c = 0; c < C; ++c) {
                const int r = am[(size_t)(p * C + c)], q = (int)(p / d->chunks);
                AMPNET_REQUIRE(r == -1 || (r >= wo[q] && r < wo[q + 1]), "probe_bn: part_amax[%lld][%lld] = %d outside window %d", (long long)p, (long long)c, r, q);
            }
    }
    PoolFinalize a;
    a.part_max = d->part_max; a.part_amax = d->part_amax; a.Q = d->Q; a.chunks = d->chunks; a.n_slots = d->n_slots; a.C = d->C;
    a.out_slot_major = d->out_slot_major; a.pooled = d->pooled; a.arg = d->arg; a.zext = d->zext;
    if (d->mode == 0) {
        a.scale = d->scale; a.shift = d->shift;
        return pool_finalize(a, st);
    }
    AMPNET_REQUIRE(d->C == 256 && d->part_amax, "probe_bn: the in-kernel BatchNorm form needs 256 channels and part_amax");
    AMPNET_REQUIRE(d->pfin_parts >= d->n_slots && d->pfin_parts % d->n_slots == 0 && d->pfin_parts <= (1 << 16), "probe_bn: pfin_parts %d", d->pfin_parts);
    const int64_t pp = d->pfin_parts;
    AMPNET_REQUIRE(d->part_sum && d->part_sum_n >= pp * 256 && d->part_sq && d->part_sq_n >= pp * 256 && d->part_rows && d->part_rows_n >= pp,
                   "probe_bn: the producer's partials [pfin_parts, 256] short");
    std::vector<int32_t> pr;
    if (int rc = bn_to_host((const int32_t *)d->part_rows, pp, pr, st, "part_rows"); rc != AMPNET_OK) return rc;
    for (int64_t p = 0; p < pp; ++p) AMPNET_REQUIRE(pr[(size_t)p] >= 0, "probe_bn: part_rows[%lld] = %d", (long long)p, pr[(size_t)p]);
    AMPNET_REQUIRE(d->gamma && d->gamma_n >= 256 && d->beta && d->beta_n >= 256, "probe_bn: gamma / beta short");
    AMPNET_REQUIRE(d->mean && d->mean_n >= S * C && d->invstd && d->invstd_n >= S * C && d->stat_mean && d->stat_mean_n >= S * C && d->stat_uvar && d->stat_uvar_n >= S * C,
                   "probe_bn: the BatchNorm outputs [n_slots, 256] short");
    a.pfin = BnPfin{{d->part_sum, d->part_sq, d->part_rows, d->pfin_parts}, {d->gamma, d->beta}, {d->scale, d->shift, d->mean, d->invstd, d->stat_mean, d->stat_uvar}};
    a.eps = d->eps;
    return pool_finalize(a, st);
}

int probe_bn_bwd_finalize(const AmpnetBnProbe *d, hipStream_t st)
{
    AMPNET_REQUIRE(d->Q >= 1 && d->Q <= (1 << 20) && d->n_slots >= 1 && d->n_slots <= 4096 && d->C >= 1 && d->C <= 4096 && d->chunks >= 1 && d->chunks <= 64 &&
                       d->part_Q >= 0 && d->part_Q <= (1 << 20) && d->uniform_rows >= 0,
                   "probe_bn: bn_bwd_finalize sizes");
    const int64_t S = d->n_slots, C = d->C, parts = (int64_t)(d->part_Q > 0 ? d->part_Q : d->Q) * d->chunks;
    AMPNET_REQUIRE(parts * C <= BIG, "probe_bn: bn_bwd_finalize partials too large");
    AMPNET_REQUIRE(d->part_a && d->part_a_n >= parts * C && d->part_b && d->part_b_n >= parts * C, "probe_bn: part_a / part_b short");
    if (d->uniform_rows <= 0) {
        std::vector<int32_t> wo;
        int64_t rows = 0;
        int max_rows = 0;
        if (int rc = bn_win_off(d, st, wo, rows, max_rows); rc != AMPNET_OK) return rc;
    } else {
        AMPNET_REQUIRE((int64_t)cdiv(d->Q, d->n_slots) * d->uniform_rows <= BIG, "probe_bn: rows per slot");
    }
    AMPNET_REQUIRE(d->gamma && d->gamma_n >= C && d->mean && d->mean_n >= S * C && d->invstd && d->invstd_n >= S * C, "probe_bn: gamma / mean / invstd short");
    AMPNET_REQUIRE(d->P1 && d->P1_n >= S * C && d->P2 && d->P2_n >= S * C && d->P3 && d->P3_n >= S * C && d->slot_ab && d->slot_ab_n >= 2 * S * C, "probe_bn: P1..P3 / slot_ab short");
    BnBwdFinalize a;
    a.part_a = d->part_a; a.part_b = d->part_b; a.win_off = d->uniform_rows > 0 ? nullptr : d->win_off; a.uniform_rows = d->uniform_rows;
    a.Q = d->Q; a.chunks = d->chunks; a.n_slots = d->n_slots; a.C = d->C; a.part_Q = d->part_Q;
    a.gamma = d->gamma; a.mean = d->mean; a.invstd = d->invstd; a.out = BnBwd{d->P1, d->P2, d->P3, d->slot_ab};
    return bn_bwd_finalize(a, st);
}

int probe_fc(const AmpnetBnProbe *d, hipStream_t st)
{
    AMPNET_REQUIRE(d->C >= 1 && d->C <= 4096 && d->per >= 1 && d->per <= (1 << 20), "probe_bn: fc sizes");
    const int64_t C = d->C;
    if (d->op == 10) {
        AMPNET_REQUIRE(d->n_slots >= 1 && d->n_slots <= 4096, "probe_bn: fc_bn_bwd n_slots %d", d->n_slots);
        const int64_t S = d->n_slots, rows = S * d->per;
        AMPNET_REQUIRE(rows * C <= BIG, "probe_bn: fc_bn_bwd too large");
        AMPNET_REQUIRE(d->da && d->da_n >= rows * C && d->z && d->z_n >= rows * C && d->g && d->g_n >= rows * C, "probe_bn: da / z / g [n_slots * per, C] short");
        AMPNET_REQUIRE(d->scale && d->scale_n >= S * C && d->shift && d->shift_n >= S * C && d->mean && d->mean_n >= S * C && d->invstd && d->invstd_n >= S * C,
                       "probe_bn: fc_bn_bwd constants [n_slots, C] short");
        AMPNET_REQUIRE(d->slot_ab && d->slot_ab_n >= 2 * S * C, "probe_bn: slot_ab short");
        return fc_bn_bwd(d->da, d->z, d->scale, d->shift, d->mean, d->invstd, d->n_slots, d->per, d->C, d->g, d->slot_ab, st);
    }
    AMPNET_REQUIRE(d->rows >= 1 && d->rows <= (1 << 20), "probe_bn: fc_act rows %d", d->rows);
    const int64_t rows = d->rows, groups = cdiv(d->rows, d->per);
    AMPNET_REQUIRE(rows * C <= BIG, "probe_bn: fc_act too large");
    AMPNET_REQUIRE(d->z && d->z_n >= rows * C && d->act && d->act_n >= rows * C && d->scale && d->scale_n >= groups * C && d->shift && d->shift_n >= groups * C,
                   "probe_bn: fc_act buffers short");
    if (d->op == 8) return fc_act(d->z, d->scale, d->shift, d->rows, d->C, d->per, d->act, st);
    const int64_t C1 = d->C1;
    AMPNET_REQUIRE(d->C1 >= 1 && d->C1 <= 4096 && rows * C1 <= BIG, "probe_bn: fc_act_pair C1 %d", d->C1);
    AMPNET_REQUIRE(d->z1 && d->z1_n >= rows * C1 && d->act1 && d->act1_n >= rows * C1 && d->s1 && d->s1_n >= groups * C1 && d->t1 && d->t1_n >= groups * C1,
                   "probe_bn: fc_act_pair second buffers short");
    return fc_act_pair(d->z, d->scale, d->shift, d->C, d->act, d->z1, d->s1, d->t1, d->C1, d->act1, d->rows, d->per, st);
}

// partials `stride` apart of [rows, cols] on ld_part, Q of them, from element `off` of a buffer of n elements
bool reduce_src_ok(int64_t n, int64_t off, int64_t Q, int64_t stride, int64_t rows, int64_t cols, int64_t ld)
{
    return Q >= 1 && Q <= (1 << 16) && rows >= 1 && cols >= 1 && rows * cols <= (1 << 22) && ld >= cols && stride >= 0 && off >= 0 &&
           off + (Q - 1) * stride + (rows - 1) * ld + cols <= n && n <= BIG;
}

int probe_reduce(const AmpnetBnProbe *d, hipStream_t st)
{
    if (d->op == 12) {
        AMPNET_REQUIRE(d->src && reduce_src_ok(d->src_n, 0, d->Q, d->stride, d->rows, d->cols, d->ld_part), "probe_bn: reduce_windows partials short");
        AMPNET_REQUIRE(d->dst && covers2(d->dst_n, d->rows, d->ld_dst, d->cols), "probe_bn: reduce_windows dst short");
        return reduce_windows(d->src, d->Q, (long)d->stride, d->rows, d->cols, d->ld_part, d->dst, d->ld_dst, d->accumulate ? 1 : 0, st);
    }
    AMPNET_REQUIRE(d->n_items >= 1 && d->n_items <= AMPNET_BN_PROBE_REDUCE && d->src && d->dst, "probe_bn: reduce_windows_multi %d items", d->n_items);
    ReduceItem it[AMPNET_BN_PROBE_REDUCE];
    for (int i = 0; i < d->n_items; ++i) {
        AMPNET_REQUIRE(reduce_src_ok(d->src_n, d->it_part_off[i], d->it_Q[i], d->it_stride[i], d->it_rows[i], d->it_cols[i], d->it_ld_part[i]),
                       "probe_bn: reduce_windows_multi item %d partials short", i);
        AMPNET_REQUIRE(d->it_dst_off[i] >= 0 && covers2(d->dst_n - d->it_dst_off[i], d->it_rows[i], d->it_ld_dst[i], d->it_cols[i]),
                       "probe_bn: reduce_windows_multi item %d dst short", i);
        it[i] = {d->src + d->it_part_off[i], d->it_Q[i], (long)d->it_stride[i], d->it_rows[i], d->it_cols[i], d->it_ld_part[i], d->dst + d->it_dst_off[i], d->it_ld_dst[i]};
    }
    return reduce_windows_multi(it, d->n_items, st);
}

}  // namespace
}  // namespace ampnet

extern "C" int ampnet_probe_bn_f32(const AmpnetBnProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_bn: null descriptor");
    AMPNET_REQUIRE(d->op >= 0 && d->op <= 16, "probe_bn: op %d not built", d->op);
    AMPNET_REQUIRE(!sync_bn_on() || d->op == 1 || d->op == 6 || d->op == 10, "probe_bn: a collective is installed; the probe launches the single-process forms only");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (d->op) {
    case 0: return probe_pw_input(d, st);
    case 1:
    case 2: return probe_bn_finalize(d, st);
    case 3:
    case 4:
    case 7: return probe_items(d, st);
    case 5: return probe_pool_finalize(d, st);
    case 6: return probe_bn_bwd_finalize(d, st);
    case 8:
    case 9:
    case 10: return probe_fc(d, st);
    case 11:
        AMPNET_REQUIRE(d->rows >= 1 && d->C >= 1 && d->C <= 4096 && (int64_t)d->rows * d->C <= BIG, "probe_bn: colsum sizes");
        AMPNET_REQUIRE(d->src && d->src_n >= (int64_t)d->rows * d->C && d->dst && d->dst_n >= d->C, "probe_bn: colsum buffers short");
        return colsum(d->src, d->rows, d->C, d->dst, st);
    case 12:
    case 13: return probe_reduce(d, st);
    case 14: {
        AMPNET_REQUIRE(d->Q >= 1 && d->Q <= 4096 && d->n_slots >= 1 && d->Q % d->n_slots == 0 && d->chunks >= 1 && d->chunks <= 64, "probe_bn: transpose64 sizes");
        const int64_t Q = d->Q;
        AMPNET_REQUIRE(d->src && d->src_n >= Q * d->chunks * 4096 && d->dst && d->dst_n >= Q * 4096 && (!d->add || d->add_n >= Q * 4096), "probe_bn: transpose64 buffers short");
        return transpose64_slot_major(d->src, d->dst, d->Q, d->n_slots, d->chunks, d->by_workgroup ? 1 : 0, d->add, st);
    }
    case 15:
        AMPNET_REQUIRE(d->Q >= 1 && d->Q <= (1 << 16) && d->k >= 1 && d->k <= 64, "probe_bn: add_identity sizes");
        AMPNET_REQUIRE(d->dst && d->dst_n >= (int64_t)d->Q * d->k * d->k, "probe_bn: add_identity T [Q, k, k] short");
        return add_identity(d->dst, d->Q, d->k, st);
    default:
        AMPNET_REQUIRE(d->rows >= 1 && d->rows <= BIG && d->idst && d->idst_n >= d->rows, "probe_bn: fill_i32_ramp dst short");
        return fill_i32_ramp(d->idst, d->rows, d->step, st);
    }
}

extern "C" int ampnet_probe_bn_plan(int Q, int chunks, int n_slots, int C, AmpnetBnPlan *o)
{
    using namespace ampnet;
    AMPNET_REQUIRE(o && Q >= 1 && chunks >= 1 && n_slots >= 1 && C >= 1, "probe_bn_plan: bad arguments");
    o->input_stat_lanes = pw_input_stat_lanes(Q, chunks, n_slots);
    o->input_stat_parts = cdiv(o->input_stat_lanes, n_slots) * n_slots;
    o->merge_floats = (int64_t)bn_finalize_merge_floats(n_slots, C);
    return AMPNET_OK;
}

// ---- the GRU recurrence and the classification head's kernels (tests/test_gru_cls_layers_gpu.py) ------------------------------------------
// One launch through the wrappers of head.h that ampnet_gru_head_* / ampnet_cls_head_* call themselves.
extern "C" int ampnet_probe_seq_f32(const AmpnetSeqProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_seq: null descriptor");
    AMPNET_REQUIRE(d->op >= 0 && d->op <= 7, "probe_seq: op %d not built", d->op);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d->op == 7) {
        AMPNET_REQUIRE(d->rows >= 1 && d->rows <= (1 << 24) && d->X && d->X_n >= d->rows && d->Y && d->Y_n >= 2 * (int64_t)d->rows, "probe_seq: sweep buffers short");
        ProfScope prof("gru_act_sweep", 0.0, 0.0, st);
        return gru_act_sweep(d->X, d->Y, d->rows, st);
    }
    AMPNET_REQUIRE(d->B >= 1 && d->B <= 65535, "probe_seq: B %d", d->B);
    const int64_t B = d->B, W = d->W, Q = B * W;
    switch (d->op) {
    case 0:
    case 1: {
        AMPNET_REQUIRE(d->W >= 1 && d->W <= 4096, "probe_seq: W %d (1 <= W <= 4096)", d->W);
        AMPNET_REQUIRE(d->Whh && d->Whh_n >= 3 * GRU_H * GRU_H, "probe_seq: Whh [192, 64] short");
        if (d->op == 0) {
            AMPNET_REQUIRE(d->gi && d->gi_n >= Q * 3 * GRU_H && d->bhh && d->bhh_n >= 3 * GRU_H, "probe_seq: gi / bhh short");
            AMPNET_REQUIRE(d->h_out && d->h_out_n >= Q * GRU_H && (!d->gates || d->gates_n >= Q * 4 * GRU_H), "probe_seq: h_out / gates short");
            ProfScope prof("gru_seq_kernel", 0.0, 0.0, st);
            return gru_seq(d->gi, d->Whh, d->bhh, d->h_out, d->gates, d->B, d->W, st);
        }
        AMPNET_REQUIRE(d->dH && d->dH_n >= Q * GRU_H && d->gates && d->gates_n >= Q * 4 * GRU_H && d->h_all && d->h_all_n >= Q * GRU_H,
                       "probe_seq: dH / gates / h_all short");
        AMPNET_REQUIRE(d->dgi && d->dgi_n >= Q * 3 * GRU_H && d->dgh && d->dgh_n >= Q * 3 * GRU_H && d->hprev_out && d->hprev_out_n >= Q * GRU_H,
                       "probe_seq: dgi / dgh / hprev_out short");
        ProfScope prof("gru_seq_bwd_kernel", 0.0, 0.0, st);
        return gru_seq_bwd(d->dH, d->gates, d->h_all, d->Whh, d->dgi, d->dgh, d->hprev_out, d->B, d->W, st);
    }
    case 2:
    case 3:
    case 6: {
        AMPNET_REQUIRE(d->W >= 1 && d->W <= HEAD_MAX_W, "probe_seq: W %d (1 <= W <= %d)", d->W, HEAD_MAX_W);
        if (d->op == 3) {
            AMPNET_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "probe_seq: drop_p %f", (double)d->drop_p);
            AMPNET_REQUIRE(d->probs && d->probs_n >= B * HEAD_HEADS * W * W && d->wout && d->wout_n >= B * W * W, "probe_seq: probs / wout short");
            ProfScope prof("cls_weights_kernel", 0.0, 0.0, st);
            return cls_weights(d->probs, d->B, d->W, d->drop_p, d->drop_seed, d->wout, st);
        }
        AMPNET_REQUIRE(d->o && d->o_n >= Q * 256 && d->cw && d->cw_n >= W && d->x && d->x_n >= B * 256, "probe_seq: o / cw / x short");
        if (d->op == 2) {
            AMPNET_REQUIRE(d->cb && d->cb_n >= 1, "probe_seq: cb short");
            ProfScope prof("cls_mix_kernel", 0.0, 0.0, st);
            return cls_mix(d->o, d->cw, d->cb, d->B, d->W, d->x, st);
        }
        AMPNET_REQUIRE(d->dx && d->dx_n >= B * 256 && d->d_o && d->d_o_n >= Q * 256 && d->cwpart && d->cwpart_n >= B * (W + 1), "probe_seq: dx / d_o / cwpart short");
        ProfScope prof("cls_mix_bwd_kernel", 0.0, 0.0, st);
        return cls_mix_bwd(d->dx, d->x, d->o, d->cw, d->B, d->W, d->d_o, d->cwpart, st);
    }
    case 4: {
        AMPNET_REQUIRE(d->z && d->z_n >= B * CLS_HID && d->act && d->act_n >= B * CLS_HID, "probe_seq: z / act [B, 128] short");
        AMPNET_REQUIRE(d->b2 && d->b2_n >= CLS_HID && d->gamma && d->gamma_n >= CLS_HID && d->beta && d->beta_n >= CLS_HID && d->rmean &&
                           d->rmean_n >= CLS_HID && d->rvar && d->rvar_n >= CLS_HID,
                       "probe_seq: b2 / gamma / beta / rmean / rvar [128] short");
        AMPNET_REQUIRE(d->scale && d->scale_n >= CLS_HID && d->shift && d->shift_n >= CLS_HID && d->mean && d->mean_n >= CLS_HID && d->invstd &&
                           d->invstd_n >= CLS_HID,
                       "probe_seq: scale / shift / mean / invstd [128] short");
        ProfScope prof("cls_bn_act_kernel", 0.0, 0.0, st);
        return cls_bn_act(d->z, d->b2, d->gamma, d->beta, d->rmean, d->rvar, d->B, d->train ? 1 : 0, d->scale, d->shift, d->mean, d->invstd, d->act, st);
    }
    default: {   // 5
        AMPNET_REQUIRE(d->C >= 1 && d->C <= CLS_MAX_CLASSES, "probe_seq: %d classes, supported 1..%d", d->C, CLS_MAX_CLASSES);
        AMPNET_REQUIRE(d->act && d->act_n >= B * CLS_HID && d->W3 && d->W3_n >= (int64_t)d->C * CLS_HID && d->b3 && d->b3_n >= d->C && d->out &&
                           d->out_n >= B * d->C,
                       "probe_seq: act / W3 / b3 / out short");
        ProfScope prof("cls_out_kernel", 0.0, 0.0, st);
        return cls_out(d->act, d->W3, d->b3, d->B, d->C, d->out, st);
    }
    }
}

// ---- the baseline single-window PointNet's kernels (tests/test_baseline_layers_gpu.py) -----------------------------------------------------
// One launch through the wrappers of baseline.h that ampnet_pointnet_seg_* / ampnet_pointnet_cls_* call themselves; ops 23 and 24 are the
// composed layer steps fwd_layer / bwd_layer.
namespace ampnet {
namespace {
const char *const BASELINE_KERNEL[] = {"bt_bias_kernel", "bt_stats_kernel", "bt_running_stats_kernel", "bt_bn_act_kernel", "bt_bn_bwd_sums_kernel",
                                       "bt_bn_bwd_apply_kernel", "bt_rowmax_kernel", "bl_rowmax_kernel", "bt_pool_scatter_kernel", "bt_mix_kernel",
                                       "bl_mix_kernel", "bt_mix_bwd_kernel", "bt_segsum_kernel", "bt_logits_kernel", "bt_logits_kernel", "bl_logits_kernel",
                                       "bt_fill_kernel", "bt_add_kernel", "bt_dropout_kernel", "bt_log_softmax_kernel", "bt_log_softmax_bwd_kernel",
                                       "bl_fold_kernel", "bl_affine_kernel", "bt_fwd_layer", "bt_bwd_layer"};
constexpr int64_t BASELINE_LIM = 1 << 24;
inline bool bp_has(const void *p, int64_t have, int64_t want) { return p && have >= want; }
inline bool bp_opt(const void *p, int64_t have, int64_t want) { return !p || have >= want; }
inline bool bp_dim(int64_t a) { return a >= 1 && a < BASELINE_LIM; }
}  // namespace
}  // namespace ampnet

extern "C" int ampnet_probe_baseline_f32(const AmpnetBaselineProbe *d, void *stream)
{
    using namespace ampnet;
    AMPNET_REQUIRE(d, "probe_baseline: null descriptor");
    AMPNET_REQUIRE(d->op >= 0 && d->op <= 24, "probe_baseline: op %d not built", d->op);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int op = d->op;
    const int64_t B = d->B, N = d->N, M = d->M, C = d->C, K = d->K, k = d->k, per = d->per;
    const bool rows_op = (op <= 5 && op != 2) || op >= 22;                               // [M, C]
    const bool win_op = op == 6 || op == 7 || op == 8 || (op >= 11 && op <= 15);         // [B, N, C] (11: [B, N, 9])
    // ---- every shape and extent first: nothing is launched, copied or recorded before all of them hold ----
    if (rows_op) AMPNET_REQUIRE(bp_dim(M) && bp_dim(C) && M * C < BASELINE_LIM, "probe_baseline: M %d C %d", d->M, d->C);
    if (op == 2 || op == 21) AMPNET_REQUIRE(bp_dim(C), "probe_baseline: C %d", d->C);
    if (win_op) AMPNET_REQUIRE(B >= 1 && B <= 65535 && bp_dim(N) && B * N * 9 < BASELINE_LIM, "probe_baseline: B %d N %d", d->B, d->N);
    if (win_op && op != 11) AMPNET_REQUIRE(bp_dim(C) && B * N * C < BASELINE_LIM, "probe_baseline: B %d N %d C %d", d->B, d->N, d->C);
    if (op == 19 || op == 20) AMPNET_REQUIRE(bp_dim(B) && C >= 1 && C <= 64, "probe_baseline: log_softmax B %d C %d (1 <= C <= 64)", d->B, d->C);
    if (op == 9 || op == 10) AMPNET_REQUIRE(bp_dim(M) && bp_dim(N) && M * 9 < BASELINE_LIM, "probe_baseline: mix M %d N %d", d->M, d->N);
    if (op >= 9 && op <= 11) AMPNET_REQUIRE(k == 2 || k == 3, "probe_baseline: k %d (2 or 3)", d->k);
    if (op >= 16 && op <= 18) AMPNET_REQUIRE(bp_dim(d->n), "probe_baseline: n %lld", (long long)d->n);
    if (op == 0 || op == 22 || op == 23) AMPNET_REQUIRE(!d->add || per >= 1, "probe_baseline: per %d with an addend", d->per);
    const int64_t MC = M * C, BC = B * C, BNC = B * N * C;
    const int64_t add_n = d->add && per >= 1 ? ((M - 1) / per + 1) * C : 0;
    const bool bn = d->gamma != nullptr;
    switch (op) {
    case 0:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, MC) && bp_opt(d->bias, d->bias_n, C) && bp_opt(d->add, d->add_n, add_n), "probe_baseline: z / bias / add short");
        break;
    case 1:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, MC) && bp_has(d->mean, d->mean_n, C) && bp_has(d->invstd, d->invstd_n, C) && bp_has(d->rm, d->rm_n, C) &&
                           bp_has(d->rv, d->rv_n, C),
                       "probe_baseline: z / mean / invstd / rm / rv short");
        break;
    case 2:
        AMPNET_REQUIRE(bp_has(d->rm, d->rm_n, C) && bp_has(d->rv, d->rv_n, C) && bp_has(d->mean, d->mean_n, C) && bp_has(d->invstd, d->invstd_n, C),
                       "probe_baseline: rm / rv / mean / invstd short");
        break;
    case 3:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, MC) && bp_has(d->a, d->a_n, MC) && bp_has(d->mean, d->mean_n, C) && bp_has(d->invstd, d->invstd_n, C) &&
                           bp_has(d->gamma, d->gamma_n, C) && bp_has(d->beta, d->beta_n, C),
                       "probe_baseline: z / a / mean / invstd / gamma / beta short");
        break;
    case 4:
    case 5:
        AMPNET_REQUIRE(bp_has(d->da, d->da_n, MC) && bp_has(d->a, d->a_n, MC) && bp_has(d->z, d->z_n, MC) && bp_has(d->mean, d->mean_n, C) &&
                           bp_has(d->invstd, d->invstd_n, C) && bp_has(d->dg, d->dg_n, C) && bp_has(d->dbe, d->dbe_n, C),
                       "probe_baseline: da / a / z / mean / invstd / dg / dbe short");
        AMPNET_REQUIRE(op == 4 || bp_has(d->gamma, d->gamma_n, C), "probe_baseline: gamma short");
        break;
    case 6:
    case 7:
        AMPNET_REQUIRE(bp_has(d->a, d->a_n, BNC) && bp_has(d->out, d->out_n, BC) && (op == 7 || bp_has(d->arg, d->arg_n, BC)), "probe_baseline: a / out / arg short");
        break;
    case 8: {
        AMPNET_REQUIRE(bp_has(d->x, d->x_n, BC) && bp_has(d->arg, d->arg_n, BC) && bp_has(d->a, d->a_n, BNC), "probe_baseline: x / arg / a short");
        std::vector<int32_t> h((size_t)BC);
        if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h.data(), d->arg, (size_t)BC * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(AMPNET_E_LAUNCH, "probe_baseline: copy of arg failed");
        for (int64_t i = 0; i < BC; ++i) AMPNET_REQUIRE(h[i] >= 0 && h[i] < N, "probe_baseline: arg[%lld] = %d outside [0, %d)", (long long)i, h[i], d->N);
        break;
    }
    case 9:
    case 10:
        AMPNET_REQUIRE(bp_has(d->x, d->x_n, M * 9) && bp_has(d->T, d->T_n, ((M - 1) / N + 1) * k * k) && bp_has(d->out, d->out_n, M * 9), "probe_baseline: x / T / out short");
        break;
    case 11:
        AMPNET_REQUIRE(bp_has(d->x, d->x_n, B * N * 9) && bp_has(d->da, d->da_n, B * N * 9) && bp_has(d->out, d->out_n, B * k * k), "probe_baseline: x / da / out short");
        break;
    case 12:
        AMPNET_REQUIRE(bp_has(d->da, d->da_n, BNC) && bp_has(d->out, d->out_n, BC), "probe_baseline: da / out short");
        break;
    case 13:
    case 14:
    case 15:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, BNC) && bp_has(d->out, d->out_n, BNC), "probe_baseline: z / out short");
        break;
    case 16:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, d->n), "probe_baseline: z short");
        break;
    case 17:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, d->n) && bp_has(d->x, d->x_n, d->n), "probe_baseline: z / x short");
        break;
    case 18:
        AMPNET_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "probe_baseline: drop_p %f", (double)d->drop_p);
        AMPNET_REQUIRE(bp_has(d->a, d->a_n, d->n) && bp_has(d->out, d->out_n, d->n), "probe_baseline: a / out short");
        break;
    case 19:
    case 20:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, BC) && bp_has(d->out, d->out_n, BC) && (op == 19 || bp_has(d->da, d->da_n, BC)), "probe_baseline: z / out / da short");
        break;
    case 21:
        AMPNET_REQUIRE(bp_opt(d->bias, d->bias_n, C) && bp_has(d->scale, d->scale_n, C) && bp_has(d->shift, d->shift_n, C), "probe_baseline: bias / scale / shift short");
        AMPNET_REQUIRE(!bn || (d->gamma_n >= C && bp_has(d->beta, d->beta_n, C) && bp_has(d->rm, d->rm_n, C) && bp_has(d->rv, d->rv_n, C)),
                       "probe_baseline: gamma / beta / rm / rv short");
        break;
    case 22:
        AMPNET_REQUIRE(bp_has(d->z, d->z_n, MC) && bp_has(d->scale, d->scale_n, C) && bp_has(d->shift, d->shift_n, C) && bp_opt(d->add, d->add_n, add_n),
                       "probe_baseline: z / scale / shift / add short");
        break;
    default: {   // 23, 24
        AMPNET_REQUIRE(K >= 1 && K <= 4096 && d->w0 >= 0 && d->lda >= K && d->ldw >= d->w0 + K && M * d->lda < BASELINE_LIM && C * d->ldw < BASELINE_LIM,
                       "probe_baseline: K %d lda %d ldw %d w0 %d", d->K, d->lda, d->ldw, d->w0);
        const int64_t A_n = (M - 1) * d->lda + K, W_n = (C - 1) * d->ldw + d->w0 + K;
        AMPNET_REQUIRE(bp_has(d->A, d->A_n, A_n) && bp_has(d->W, d->W_n, W_n) && bp_has(d->z, d->z_n, MC), "probe_baseline: A / W / z short");
        AMPNET_REQUIRE(!bn || (d->gamma_n >= C && bp_has(d->a, d->a_n, MC) && bp_has(d->mean, d->mean_n, C) && bp_has(d->invstd, d->invstd_n, C)),
                       "probe_baseline: gamma / a / mean / invstd short");
        if (op == 23) {
            AMPNET_REQUIRE(bp_opt(d->bias, d->bias_n, C) && bp_opt(d->add, d->add_n, add_n), "probe_baseline: bias / add short");
            AMPNET_REQUIRE(!bn || (bp_has(d->beta, d->beta_n, C) && bp_has(d->rm, d->rm_n, C) && bp_has(d->rv, d->rv_n, C)), "probe_baseline: beta / rm / rv short");
            break;
        }
        AMPNET_REQUIRE(bp_has(d->da, d->da_n, MC) && bp_has(d->dW, d->dW_n, W_n) && bp_opt(d->db, d->db_n, C), "probe_baseline: da / dW / db short");
        AMPNET_REQUIRE(!bn || (bp_has(d->dg, d->dg_n, C) && bp_has(d->dbe, d->dbe_n, C)), "probe_baseline: dg / dbe short");
        AMPNET_REQUIRE(!d->dA || (d->ld_dA >= K && M * d->ld_dA < BASELINE_LIM && d->dA_n >= (M - 1) * d->ld_dA + K), "probe_baseline: dA short (ld_dA %d)", d->ld_dA);
    }
    }
    // ---- the launch ----
    if (op >= 23) {
        Rec r{d->z, bn ? d->a : d->z, d->mean, d->invstd, d->M, d->K, d->C};
        if (op == 23) return fwd_layer(TLayer{d->W, d->bias, d->gamma, d->beta, d->rm, d->rv}, r, d->train == 0, d->A, d->lda, d->ldw, d->w0, d->add, d->per, st);
        return bwd_layer(TLayer{d->W, nullptr, d->gamma, nullptr, nullptr, nullptr}, TGrad{d->dW, d->db, bn ? d->dg : nullptr, bn ? d->dbe : nullptr}, r, nullptr,
                         nullptr, d->da, d->A, d->lda, d->ldw, d->w0, d->dA, d->ld_dA, d->accumulate, st);
    }
    ProfScope prof(BASELINE_KERNEL[op], 0.0, 0.0, st);
    switch (op) {
    case 0: bt_bias(d->z, (size_t)MC, d->C, d->bias, d->add, d->per, st); break;
    case 1: bt_stats(d->z, d->M, d->C, d->eps, d->momentum, d->mean, d->invstd, d->rm, d->rv, st); break;
    case 2: bt_running_stats(d->rm, d->rv, d->C, d->eps, d->mean, d->invstd, st); break;
    case 3: bt_bn_act(d->z, (size_t)MC, d->C, d->mean, d->invstd, d->gamma, d->beta, d->a, st); break;
    case 4: bt_bn_bwd_sums(d->da, d->a, d->z, d->M, d->C, d->mean, d->invstd, d->dg, d->dbe, st); break;
    case 5: bt_bn_bwd_apply(d->da, d->a, d->z, (size_t)MC, d->M, d->C, d->mean, d->invstd, d->gamma, d->dg, d->dbe, st); break;
    case 6: bt_rowmax(d->a, d->B, d->N, d->C, d->out, d->arg, st); break;
    case 7: bl_rowmax(d->a, d->B, d->N, d->C, d->out, st); break;
    case 8: bt_pool_scatter(d->x, d->arg, d->B, d->N, d->C, d->a, st); break;
    case 9: bt_mix(d->x, d->T, d->M, d->N, d->k, d->out, st); break;
    case 10: bl_mix(d->x, d->T, d->M, d->N, d->k, d->out, st); break;
    case 11: bt_mix_bwd(d->x, d->da, d->B, d->N, d->k, d->out, st); break;
    case 12: bt_segsum(d->da, d->B, d->N, d->C, d->out, st); break;
    case 13: bt_logits(d->z, d->B, d->N, d->C, d->out, st); break;
    case 14: bt_logits_to_rows(d->out, d->B, d->N, d->C, d->z, st); break;
    case 15: bl_logits(d->z, d->B, d->N, d->C, d->out, st); break;
    case 16: bt_fill(d->z, (size_t)d->n, d->value, st); break;
    case 17: bt_add(d->z, d->x, (size_t)d->n, st); break;
    case 18: bt_dropout(d->a, (size_t)d->n, d->drop_seed, d->drop_p, d->out, st); break;
    case 19: bt_log_softmax(d->z, d->B, d->C, d->out, st); break;
    case 20: bt_log_softmax_bwd(d->z, d->da, d->B, d->C, d->out, st); break;
    case 21: bl_fold(BlLayer{nullptr, d->bias, d->gamma, d->beta, d->rm, d->rv}, d->C, d->eps, d->scale, d->shift, st); break;
    default: bl_affine(d->z, (size_t)MC, d->C, d->scale, d->shift, d->add, d->per, d->relu, st); break;
    }
    return check_launch(BASELINE_KERNEL[op]);
}
