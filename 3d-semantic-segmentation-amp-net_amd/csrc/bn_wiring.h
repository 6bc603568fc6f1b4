// bn_wiring.h -- host side of bn_desc.h: each kind of BatchNorm launch argument is built from descriptors at ONE place, for the encoder, the
// heads and their backward alike.  (Which consumer may finish a BatchNorm itself is bn_fwd_in_kernel / bn_bwd_in_kernel, kernels.h.)
#pragma once
#include "bwd_misc.h"

namespace ampnet {

// the six forward arrays / the four backward arrays of one layer out of a workspace carver (any type with take<T>(n))
template <typename Carver> void carve_bn(Carver &c, BnSlot &b, int n_slots, int C)
{
    b.C = C;
    for (float **p : {&b.scale, &b.shift, &b.mean, &b.invstd, &b.smean, &b.suvar}) *p = c.template take<float>((size_t)n_slots * C);
}
template <typename Carver> void carve_bn_bwd(Carver &c, BnBwd &b, int n_slots, int C)
{
    for (float **p : {&b.P1, &b.P2, &b.P3}) *p = c.template take<float>((size_t)n_slots * C);
    b.slot_ab = c.template take<float>((size_t)2 * n_slots * C);
}

// the windows a layer ran on, as the backward finalize counts the rows of a slot
struct BnWindows {
    const int *win_off;            // may be nullptr when the windows are uniform
    int Q, n_slots, max_rows;
    long R;                        // total rows: max_rows * Q == R says every window has max_rows rows
};

// launched forward finalize of per-workgroup partials (every partial carries its own row count)
inline BnFinalize bn_finalize_args(const BnPartials &part, const BnLayer &layer, const BnFwd &out, int n_slots, int C, float *merge_ws)
{
    BnFinalize f;
    f.part = part; f.Q = part.parts; f.chunks = 1;
    f.n_slots = n_slots; f.C = C;
    f.layer = layer; f.out = out; f.merge_ws = merge_ws;
    return f;
}

// launched backward finalize: part_a / part_b hold `chunks` partials per window (part_Q == 0) or part_Q per-workgroup partials (chunks == 1)
inline BnBwdFinalize bn_bwd_finalize_args(const float *part_a, const float *part_b, int part_Q, int chunks, const BnWindows &w, int C, const float *gamma,
                                          const BnFwd &fwd, const BnBwd &out)
{
    BnBwdFinalize f;
    f.part_a = part_a; f.part_b = part_b; f.part_Q = part_Q; f.chunks = chunks;
    f.win_off = w.win_off; f.Q = w.Q; f.n_slots = w.n_slots; f.C = C;
    f.uniform_rows = (long)w.max_rows * w.Q == w.R ? w.max_rows : 0;
    f.gamma = gamma; f.mean = fwd.mean; f.invstd = fwd.invstd; f.out = out;
    return f;
}

// the same constants formed inside the consumer (PwBwd.fin, PwInputWgrad.fin): `parts` per-workgroup partials, uniform windows
inline BnBwdFin bn_bwd_fin(const float *part_a, const float *part_b, int parts, int slot_rows, const float *gamma, const BnFwd &fwd, const BnBwd &out)
{
    BnBwdFin f;
    f.part_a = part_a; f.part_b = part_b; f.parts = parts; f.rows = slot_rows;
    f.gamma = gamma; f.mean = fwd.mean; f.invstd = fwd.invstd; f.out = out;
    return f;
}

// dense gradient source of a layer with BatchNorm behind it: g = dy P1 + z P2 + P3
inline GradSrc grad_src(const float *dy, const float *z, int C, int z_bf16, const BnBwd &b)
{
    GradSrc g;
    g.dy = dy; g.z = z; g.C = C; g.z_bf16 = z_bf16;
    g.P1 = b.P1; g.P2 = b.P2; g.P3 = b.P3;
    return g;
}

}  // namespace ampnet
