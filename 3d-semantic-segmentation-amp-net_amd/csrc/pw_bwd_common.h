// pw_bwd_common.h -- what the fused-backward kernels share: pw_bwd_kernel (pw_bwd_fused.hip), pw_bwd_bf16_kernel (pw_bwd_bf16.hip),
// pw_bwd_x3_kernel and pw_bwd_x3n_kernel (pw_bwd_x3.hip).  The host planner (pw_bwd_blocks / items_per_block) and the fixed-order partial
// sums rely on all of them splitting the work over (window, chunk) items and walking the blocks of rows alike, so that is ONE text here.
//
// What is NOT here, and why: a piece moves into this header only where every instantiation of the calling kernel keeps its register
// metadata and its sequence of vector / LDS / memory instructions and waits (compared on the device assembly of both versions).  The bf16 and
// the split kernels keep both with the helpers below.  The fp32 kernel does not -- even the work split alone as a function renumbers the
// staging registers and moves instructions in 8 of its 13 instantiations -- so it shares the constants only and keeps its own copy of the
// split and the walk.  The PwBwd.fin prologue, the D-role lane constants and the flush (dWpart tile stores, dbpart and part_a / part_b
// reductions) were tried as functions in every kernel and changed the stream (the dense split kernel sits at 256 VGPRs and spills
// differently with each of them): they stay per kernel.  Staging, role assignment, K loops and epilogues are where the kernels really differ.
#pragma once
#include "kernels.h"

namespace ampnet {

constexpr int PW_BWD_THREADS = 512;
constexpr int PW_BWD_ITEM_ROWS = 256;      // granularity of the work split inside a slot = pw_bwd_item_rows(): the host sizes per-window shares with it

// ---- work split: items = (window of this slot, chunk of PW_BWD_ITEM_ROWS rows), contiguous share per workgroup (slot, jb) ----
struct PwBwdSplit {
    int cpw;                        // chunks (items) per window
    int item_begin, item_end;       // this workgroup's items
};
__device__ __forceinline__ PwBwdSplit pw_bwd_split(const PwBwd &a, int slot, int jb)
{
    const int per_slot = (a.Q - slot + a.n_slots - 1) / a.n_slots;
    const int cpw = (a.max_rows + PW_BWD_ITEM_ROWS - 1) / PW_BWD_ITEM_ROWS;
    const int n_items = per_slot * cpw;
    const int ipb = a.items_per_block > 0 ? a.items_per_block : (n_items + a.blocks_per_slot - 1) / a.blocks_per_slot;
    const int item_begin = min(jb * ipb, n_items), item_end = min(item_begin + ipb, n_items);
    return PwBwdSplit{cpw, item_begin, item_end};
}

// ---- the walk over blocks of ROWS rows (crosses item boundaries so that the prefetch never drains) ----
struct PwBwdPos {
    int item, row0, row_end;        // current block = rows [row0, min(row0 + ROWS, row_end))
};
// first block of the next non-empty item at or after `item`
__device__ __forceinline__ bool open_item(const PwBwd &a, const PwBwdSplit &sp, int slot, int item, PwBwdPos &p)
{
    for (; item < sp.item_end; ++item) {
        const int q = (item / sp.cpw) * a.n_slots + slot, ch = item % sp.cpw;
        const int rb = a.win_off[q] + ch * PW_BWD_ITEM_ROWS;
        const int re = min(a.win_off[q + 1], rb + PW_BWD_ITEM_ROWS);
        if (rb < re) {
            p.item = item;
            p.row0 = rb;
            p.row_end = re;
            return true;
        }
    }
    return false;
}
template <int ROWS>
__device__ __forceinline__ bool advance(const PwBwd &a, const PwBwdSplit &sp, int slot, PwBwdPos &p)
{
    if (p.row0 + ROWS < p.row_end) {
        p.row0 += ROWS;
        return true;
    }
    return open_item(a, sp, slot, p.item + 1, p);
}

// per-window matrix T[pidx][cy][cx] (the bmm transform, already "transposed": out[row][cy] = sum_cx g[row][cx] T[cy][cx]);
// the host keeps every workgroup inside one window (items_per_block divides the chunks per window)
__device__ __forceinline__ const float *pw_bwd_window_weight(const PwBwd &a, const PwBwdSplit &sp, int slot)
{
    const int bi = sp.item_begin / sp.cpw;
    const int pidx = a.perwin_slot_major ? slot * (a.Q / a.n_slots) + bi : bi * a.n_slots + slot;
    return a.W + (size_t)pidx * a.w_win_stride;
}

}  // namespace ampnet
