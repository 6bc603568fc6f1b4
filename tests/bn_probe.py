"""Layer-local float64 oracle of the BatchNorm / pooling glue kernels: pw_input, bn_finalize (per-chunk, per-workgroup, two-stage and gathered
forms), bn_fold, bn_running_update, pool_finalize (plain and with the in-kernel BatchNorm finish), bn_bwd_finalize, bn_param_grads, fc_act,
fc_act_pair, fc_bn_bwd, colsum, reduce_windows(_multi), transpose64_slot_major, add_identity and fill_i32_ramp.

The C side is ampnet_probe_bn_f32 (include/ampnet_hip.h, "test hooks"; csrc/layer_probe.hip): ONE launch of one of them, selected by `op`, on buffers
the test chose, every extent checked on the host first.  This module holds the ctypes mirrors of AmpnetBnProbe / AmpnetBnPlan and a float64
restatement of each operation, written from the comments of csrc/kernels.h and csrc/bwd_misc.h (PwInput, BnFinalize, BnFoldItem, BnRunItem,
PoolFinalize, BnBwdFinalize, BnGradItem, reduce_windows, ...), not from the kernel bodies.  tests/test_bn_refs_cpu.py holds the restatements to
torch in float64 (batch_norm, BatchNorm1d's running update, max_pool1d, autograd); the GPU tests are tests/test_bn_glue_gpu.py.

Bars: the project's one rule, pw_probe.bar = 8 eps sqrt(K) mag + 2 eps |x64| with eps = 2^-24.  K = the number of terms the kernel sums in fp32
(1 where it sums in double: only the roundings of the outputs remain), mag = the float64 sum of the absolute terms.  Where an output is formed
from outputs that carry a bar of their own (shift from scale, pooled from scale and shift, g from the slot sums) those bars are carried through.
Every restatement returns {output name: (float64 value, bar)}.

The global-batch forms (ampnet_set_collective: the sync_bn_on() branches of bn_finalize, bn_bwd_finalize, fc_bn_bwd; csrc/sync_bn.hip) are restated
on the WHOLE batch from the ranks' inputs: finalize_global_ref, bn_bwd_finalize_global_ref, fc_bn_bwd_global_ref (pool_bwd's is beside pool_bwd_ref in
tests/test_pooled_bwd_gpu.py).  Their bars add what the exchange carries in fp32 -- one rounding per rank and packed quantity, an all-reduce of
`world` fp32 terms (`allreduced`) -- carried through to the outputs; outputs that stay per-rank keep the single-process bars.  With one rank each
collapses to its single-process restatement.  The GPU tests are tests/test_syncbn_layers_gpu.py (two gloo ranks).
"""
import ctypes

import numpy as np
import torch

import pw_probe as PP
from pw_probe import EPS16, EPS32, L, bar, chan_merge, moment_bars

AMPNET_E_ARG = PP.AMPNET_E_ARG
ITEMS, REDUCE = 25, 13            # AMPNET_BN_PROBE_ITEMS, AMPNET_BN_PROBE_REDUCE
BN_EPS = float(np.float32(1e-5))  # the fp32 constants the kernels get
MOMENTUM = float(np.float32(0.1))
OPS = {"pw_input": 0, "bn_finalize": 1, "bn_finalize_gathered": 2, "bn_fold": 3, "bn_running_update": 4, "pool_finalize": 5, "bn_bwd_finalize": 6,
       "bn_param_grads": 7, "fc_act": 8, "fc_act_pair": 9, "fc_bn_bwd": 10, "colsum": 11, "reduce_windows": 12, "reduce_windows_multi": 13,
       "transpose64": 14, "add_identity": 15, "fill_i32_ramp": 16}

_p, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
POINTERS = ("x", "W", "T", "Z", "part_sum", "part_sq", "part_rows", "win_off", "gamma", "beta", "scale", "shift", "mean", "invstd", "stat_mean",
            "stat_uvar", "merge_ws", "rmean", "rvar", "part_max", "part_amax", "pooled", "arg", "zext", "part_a", "part_b", "P1", "P2", "P3",
            "slot_ab", "dgamma", "dbeta", "z", "da", "g", "act", "z1", "s1", "t1", "act1", "src", "dst", "add", "idst")


class BnProbe(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("op", "mode", "Q", "n_slots", "C", "C1", "chunks", "chunk_rows", "uniform_rows", "stat_lanes", "perwin_slot_major",
                                    "z_bf16", "out_slot_major", "part_Q", "pfin_parts", "gather_ranks", "n_items", "rows", "cols", "ld_part", "ld_dst",
                                    "accumulate", "by_workgroup", "per", "k", "step")] + \
               [("eps", _f32), ("momentum", _f32), ("stride", _i64), ("gather_seg", _i64), ("it_C", _i32 * ITEMS), ("pad0", _i32)] + \
               [(n, _i32 * REDUCE) for n in ("it_Q", "it_rows", "it_cols", "it_ld_part", "it_ld_dst")] + [("pad1", _i32)] + \
               [(n, _i64 * REDUCE) for n in ("it_stride", "it_part_off", "it_dst_off")] + \
               [x for n in POINTERS for x in ((n, _p), (n + "_n", _i64))]


class BnPlan(ctypes.Structure):
    _fields_ = [("input_stat_lanes", _i32), ("input_stat_parts", _i32), ("merge_floats", _i64)]


EXTENTS = {n: n + "_n" for n in POINTERS}


def set_tensors(desc, **tensors):
    PP.set_tensors(desc, EXTENTS, **tensors)


def new(op, **ints):
    d = BnProbe()
    d.op = OPS[op]
    d.eps, d.momentum = BN_EPS, MOMENTUM
    for k, v in ints.items():
        setattr(d, k, v)
    return d


def run(desc):
    """(return code, kernel names recorded) of one ampnet_probe_bn_f32 call, synchronised.  The glue kernels record no profile name: the
    list is empty either way and only says that no OTHER instrumented kernel ran."""
    lib = L.lib()
    lib.ampnet_probe_bn_f32.argtypes = [ctypes.POINTER(BnProbe), ctypes.c_void_p]
    lib.ampnet_profile_enable(1)
    try:
        rc = lib.ampnet_probe_bn_f32(ctypes.byref(desc), L.stream_ptr())
        torch.cuda.synchronize()
        names = PP.profile_names(lib)
    finally:
        lib.ampnet_profile_enable(0)
    return rc, names


def plan(Q, chunks, n_slots, C=64):
    lib = L.lib()
    lib.ampnet_probe_bn_plan.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(BnPlan)]
    p = BnPlan()
    L.check(lib.ampnet_probe_bn_plan(Q, chunks, n_slots, C, ctypes.byref(p)), "ampnet_probe_bn_plan")
    return p


def f64(x):
    return np.asarray(x, dtype=np.float64)


def worst(got, want_bar):
    want, b = want_bar
    return PP.err_ratio(got, want, b)


# ---- windows, chunks, slots ----------------------------------------------------------------------------------------------------------
def chunk_rows_of(win_off, chunks, chunk_rows):
    """rows [Q, chunks] of every chunk: chunk ch of window q covers rows ch * chunk_rows .. of the window, clipped to it."""
    w = np.diff(np.asarray(win_off, dtype=np.int64))
    return np.clip(w[:, None] - np.arange(chunks)[None, :] * chunk_rows, 0, chunk_rows)


def chunk_partials(z, win_off, chunks, chunk_rows):
    """float64 (mean, M2, rows) [Q * chunks, C] / [Q * chunks] of the rows z [rows, C]: what a producer leaves per chunk (empty chunk: zeros)."""
    z = f64(z)
    Q = len(win_off) - 1
    n = chunk_rows_of(win_off, chunks, chunk_rows)
    mean, m2 = np.zeros((Q * chunks, z.shape[1])), np.zeros((Q * chunks, z.shape[1]))
    for q in range(Q):
        for ch in range(chunks):
            if n[q, ch] > 0:
                r = z[win_off[q] + ch * chunk_rows:win_off[q] + ch * chunk_rows + n[q, ch]]
                mean[q * chunks + ch] = r.mean(0)
                m2[q * chunks + ch] = ((r - r.mean(0)) ** 2).sum(0)
    return mean, m2, n.reshape(-1)


def slot_of_partial(n_parts, chunks, n_slots):
    """slot of partial p = q * chunks + ch: q % n_slots (per-workgroup partials: chunks = 1, so p % n_slots)."""
    return (np.arange(n_parts) // chunks) % n_slots


# ---- pw_input ------------------------------------------------------------------------------------------------------------------------
def input_weights(W, T, mode, Q, n_slots, slot_major):
    """effective weights [Q, 64, nf] of every window and their operand magnitudes (kernels.h: PwInput)."""
    W = f64(W)
    if mode == 0:
        return np.broadcast_to(W[None, :, :3], (Q, 64, 3)), np.broadcast_to(np.abs(W[None, :, :3]), (Q, 64, 3))
    T = f64(T).reshape(-1, 3, 3)
    q = np.arange(Q)
    pidx = (q % n_slots) * (Q // n_slots) + q // n_slots if slot_major else q
    Tq = T[pidx]                                                           # [Q, f, d]
    weff = np.broadcast_to(W[None, :, 3:12], (Q, 64, 9)).copy()
    wmag = np.abs(weff)
    weff[:, :, :3] += np.einsum("qfd,cd->qcf", Tq, W[:, :3])
    wmag[:, :, :3] += np.einsum("qfd,cd->qcf", np.abs(Tq), np.abs(W[:, :3]))
    return weff, wmag


def input_ref(x, W, T, mode, win_off, n_slots, slot_major=0):
    """Z64 [rows, 64], mag [rows, 64] and K (3, or the 12 products of conv_1 on cat(xyz T, x))."""
    Q = len(win_off) - 1
    weff, wmag = input_weights(W, T, mode, Q, n_slots, slot_major)
    nf = 3 if mode == 0 else 9
    xx = f64(x)[:, :nf]
    q = PP.win_of_rows(win_off)
    Z = np.einsum("rf,rcf->rc", xx, weff[q])
    M = np.einsum("rf,rcf->rc", np.abs(xx), wmag[q])
    return Z, M, (3 if mode == 0 else 12)


# ---- bn_finalize -----------------------------------------------------------------------------------------------------------------------
def finalize_ref(means, m2s, rows, slots, n_slots, gamma, beta, eps=BN_EPS):
    """BatchNorm constants of every slot from the (mean, M2, rows) partials [P, C], [P, C], [P]; slots [P] = the slot of each partial.
    scale = gamma invstd, shift = beta - mean scale, invstd = 1 / sqrt(M2 / N + eps), stat_uvar = M2 / (N - 1) (N <= 1: M2);
    a slot with no row: mean 0, variance 0.  The sums are the kernel's in double: K = 1, only the output roundings are in the bars."""
    means, m2s, gamma, beta = f64(means), f64(m2s), f64(gamma), f64(beta)
    C = means.shape[1]
    out = {k: np.zeros((n_slots, C)) for k in ("mean", "mmag", "var", "uvar", "N")}
    for s in range(n_slots):
        sel = np.nonzero((np.asarray(slots) == s) & (np.asarray(rows) > 0))[0]
        N, mean, m2 = chan_merge([means[p] for p in sel], [m2s[p] for p in sel], [rows[p] for p in sel]) if len(sel) else (0.0, np.zeros(C), np.zeros(C))
        out["N"][s] = N
        out["mean"][s] = mean
        out["mmag"][s] = sum(rows[p] * np.abs(means[p]) for p in sel) / N if N > 0 else 0.0
        out["var"][s] = m2 / N if N > 0 else 0.0
        out["uvar"][s] = m2 / (N - 1.0) if N > 1 else m2
    invstd = 1.0 / np.sqrt(out["var"] + eps)
    scale = gamma[None, :] * invstd
    shift = beta[None, :] - out["mean"] * scale
    b_scale = bar(np.abs(scale), scale, 1)
    b_mean = bar(out["mmag"], out["mean"], 1)
    b_shift = bar(np.abs(beta)[None, :] + out["mmag"] * np.abs(scale), shift, 1) + out["mmag"] * b_scale
    return {"scale": (scale, b_scale), "shift": (shift, b_shift), "mean": (out["mean"], b_mean), "invstd": (invstd, bar(invstd, invstd, 1)),
            "stat_mean": (out["mean"], b_mean), "stat_uvar": (out["uvar"], bar(out["uvar"], out["uvar"], 1)), "N": out["N"]}


def concat_ranks(ranks):
    """(means, m2s, rows, slots) of the whole batch from the ranks' (means [P_r, C], m2s [P_r, C], rows [P_r], slots [P_r]): the partials one
    after the other, each with its slot."""
    return tuple(np.concatenate([np.asarray(r[i]) for r in ranks]) for i in range(4))


def finalize_global_ref(ranks, n_slots, gamma, beta, eps=BN_EPS):
    """bn_finalize under a collective (pw_misc.hip: rank merge -> all-gather -> gathered finalize): finalize_ref of the concatenated partials.
    Bars: finalize_ref's own (the output roundings of the double merge) plus, with more than one rank, what the all-gather carries in fp32:
    rank r's merged mean_r and M2_r are ONE rounding of a double sum each, d mean_r = bar(mag_r, mean_r, 1), d M2_r = bar(M2_r, M2_r, 1)
    (M2_r is a sum of non-negative terms: its own magnitude); the rows are integers, exact.  Carried through the merge
    mean = sum N_r mean_r / N, M2 = sum M2_r + N_r (mean_r - mean)^2:
      d mean = sum N_r d mean_r / N;  d M2 = sum d M2_r + 2 N_r |mean_r - mean| d mean_r + N_r d mean_r^2;  d var = d M2 / N;
      d invstd = invstd^3 d var / 2;  d uvar = d M2 / (N - 1) (N <= 1: d M2);  d scale = |gamma| d invstd;  d shift = |mean| d scale + |scale| d mean."""
    res = finalize_ref(*concat_ranks(ranks), n_slots, gamma, beta, eps)
    if len(ranks) == 1:
        return res
    gamma = f64(gamma)
    C = gamma.shape[0]
    mean, N = res["mean"][0], res["N"]
    d_mean, d_m2 = np.zeros((n_slots, C)), np.zeros((n_slots, C))
    for means, m2s, rows, slots in ranks:
        means, m2s = f64(means), f64(m2s)
        for s in range(n_slots):
            sel = np.nonzero((np.asarray(slots) == s) & (np.asarray(rows) > 0))[0]
            if not len(sel):
                continue
            Nr, mr, m2r = chan_merge([means[p] for p in sel], [m2s[p] for p in sel], [rows[p] for p in sel])
            mag = sum(rows[p] * np.abs(means[p]) for p in sel) / Nr
            dm = bar(mag, mr, 1)
            d_mean[s] += Nr * dm / N[s]
            d_m2[s] += bar(m2r, m2r, 1) + 2.0 * Nr * np.abs(mr - mean[s]) * dm + Nr * dm * dm
    Ns = np.where(N > 0, N, 1.0)
    invstd, scale = res["invstd"][0], res["scale"][0]
    d_inv = 0.5 * invstd ** 3 * d_m2 / Ns
    d_scale = np.abs(gamma)[None, :] * d_inv
    add = {"mean": d_mean, "stat_mean": d_mean, "invstd": d_inv, "scale": d_scale, "shift": np.abs(mean) * d_scale + np.abs(scale) * d_mean,
           "stat_uvar": d_m2 / np.where(N > 1, N - 1.0, 1.0)}
    return {k: ((v[0], v[1] + add[k]) if k in add else v) for k, v in res.items()}


def fold_ref(gamma, beta, rmean, rvar, eps=BN_EPS):
    """eval mode: scale = gamma / sqrt(rvar + eps), shift = beta - rmean scale (fp32 arithmetic in the kernel: one term each, K = 1)."""
    gamma, beta, rmean, rvar = f64(gamma), f64(beta), f64(rmean), f64(rvar)
    scale = gamma / np.sqrt(rvar + eps)
    shift = beta - rmean * scale
    b_scale = bar(np.abs(scale), scale, 1)
    return {"scale": (scale, b_scale), "shift": (shift, bar(np.abs(beta) + np.abs(rmean * scale), shift, 1) + np.abs(rmean) * b_scale)}


def running_ref(rmean, rvar, stat_mean, stat_uvar, momentum=MOMENTUM):
    """r <- (1 - momentum) r + momentum stat[s] for s = 0 .. n_slots - 1 in order (nn.BatchNorm1d fed the slots one after the other).
    fp32 in the kernel: 2 terms per slot in one chain, K = 2 n_slots, mag = the same recursion on the absolute values."""
    res = {}
    for name, r, st in (("rmean", rmean, stat_mean), ("rvar", rvar, stat_uvar)):
        r, st = f64(r).copy(), f64(st)
        m = np.abs(r)
        for s in range(st.shape[0]):
            r = (1.0 - momentum) * r + momentum * st[s]
            m = (1.0 - momentum) * m + momentum * np.abs(st[s])
        res[name] = (r, bar(m, r, 2 * st.shape[0]))
    return res


# ---- pool_finalize -----------------------------------------------------------------------------------------------------------------------
def pool_partials(z, win_off, chunks, chunk_rows, gamma, track=True):
    """What pw_gemm's pool epilogue leaves: per chunk the extreme of each column (max where gamma >= 0, else min) and the FIRST row it sits in;
    an empty chunk: row -1 (and -inf / +inf as the value).  fp32 values of z, exact."""
    z = np.asarray(z, dtype=np.float32)
    Q, C = len(win_off) - 1, z.shape[1]
    n = chunk_rows_of(win_off, chunks, chunk_rows)
    use_max = np.asarray(gamma) >= 0
    pmax = np.where(use_max, -np.inf, np.inf).astype(np.float32)[None, :].repeat(Q * chunks, 0)
    amax = np.full((Q * chunks, C), -1, dtype=np.int32)
    for q in range(Q):
        for ch in range(chunks):
            if n[q, ch] > 0:
                r0 = win_off[q] + ch * chunk_rows
                r = z[r0:r0 + n[q, ch]]
                a = np.where(use_max, r.argmax(0), r.argmin(0))
                pmax[q * chunks + ch] = r[a, np.arange(C)]
                amax[q * chunks + ch] = r0 + a
    return pmax, (amax if track else None)


def pool_ref(part_max, part_amax, scale, shift, Q, chunks, n_slots, slot_major, b_scale=None, b_shift=None):
    """pooled[orow(q), c] = relu(scale extreme + shift), extreme = max for scale >= 0 else min over the window's non-empty chunks, the earliest
    chunk on equal extremes; arg = that chunk's row, zext = the extreme (row q).  No non-empty chunk: arg -1, zext 0, pooled relu(shift).
    Without part_amax a chunk is empty iff its value is infinite, and arg is not produced.  b_scale / b_shift: bars the constants carry."""
    pm = f64(part_max).reshape(Q, chunks, -1)
    C = pm.shape[2]
    valid = (np.asarray(part_amax).reshape(Q, chunks, C) >= 0) if part_amax is not None else np.isfinite(pm)
    slot = np.arange(Q) % n_slots
    sc, sh = f64(scale)[slot], f64(shift)[slot]                               # [Q, C]
    use_max = sc >= 0
    key = np.where(use_max[:, None, :], pm, -pm)                             # the extreme is the max of key
    key = np.where(valid, key, -np.inf)
    chosen = key.argmax(1)                                                   # first chunk holding the extreme
    some = valid.any(1)
    best = np.where(some, np.take_along_axis(pm, chosen[:, None, :], 1)[:, 0, :], 0.0)
    arg = None
    if part_amax is not None:
        arg = np.where(some, np.take_along_axis(np.asarray(part_amax).reshape(Q, chunks, C), chosen[:, None, :], 1)[:, 0, :], -1)
    pre = best * sc + sh
    b = bar(np.abs(best * sc) + np.abs(sh), pre, 1)
    if b_scale is not None:
        b = b + np.abs(best) * f64(b_scale)[slot] + f64(b_shift)[slot]
    orow = (np.arange(Q) % n_slots) * (Q // n_slots) + np.arange(Q) // n_slots if slot_major else np.arange(Q)
    pooled, pb = np.zeros((Q, C)), np.zeros((Q, C))
    pooled[orow] = np.maximum(pre, 0.0)
    pb[orow] = b
    return {"pooled": (pooled, pb), "zext": (best, np.zeros_like(best)), "arg": arg}


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def bn_bwd_finalize_ref(part_a, part_b, slots, slot_rows, gamma, mean, invstd, n_slots):
    """A = sum dy, Bs = sum dy zhat over the slot's partials (slots [P]); s = gamma invstd; P1 = s, P2 = -s invstd Bs / n,
    P3 = -s A / n - P2 mean; slot_ab = (A, Bs); n = slot_rows[slot]; a slot with no row: P2 = P3 = 0.  Sums in double: K = 1."""
    pa, pb, gamma, mean, invstd = f64(part_a), f64(part_b), f64(gamma), f64(mean), f64(invstd)
    C = pa.shape[1]
    A, Bs, Am, Bm = (np.zeros((n_slots, C)) for _ in range(4))
    for s in range(n_slots):
        sel = np.asarray(slots) == s
        A[s], Bs[s], Am[s], Bm[s] = pa[sel].sum(0), pb[sel].sum(0), np.abs(pa[sel]).sum(0), np.abs(pb[sel]).sum(0)
    n = f64(slot_rows)[:, None]
    live = n > 0
    nn = np.where(live, n, 1.0)
    sv = gamma[None, :] * invstd
    P2 = np.where(live, -sv * invstd * Bs / nn, 0.0)
    P2m = np.where(live, np.abs(sv * invstd) * Bm / nn, 0.0)
    P3 = np.where(live, -sv * A / nn - P2 * mean, 0.0)
    P3m = np.where(live, np.abs(sv) * Am / nn + P2m * np.abs(mean), 0.0)
    ab = np.stack([A, Bs], -1)
    return {"P1": (sv, bar(np.abs(sv), sv, 1)), "P2": (P2, bar(P2m, P2, 1)), "P3": (P3, bar(P3m, P3, 1)),
            "slot_ab": (ab, bar(np.stack([Am, Bm], -1), ab, 1))}


def allreduced(sums, mags):
    """What the all-reduce of sync_bn.hip leaves of one packed quantity: (float64 sum over the ranks, its magnitude, its bar).  Rank r packs
    x_r as ONE fp32 rounding of a double sum: bar(mag_r, x_r, 1) each; the all-reduce then adds world fp32 terms: K = world, mag = the sum of
    the ranks' magnitudes.  One rank: the exchange is the identity and only the rank's own rounding remains."""
    tot, mag = sum(f64(x) for x in sums), sum(f64(m) for m in mags)
    b = sum(bar(f64(m), f64(x), 1) for x, m in zip(sums, mags))
    if len(sums) > 1:
        b = b + bar(mag, tot, len(sums))
    return tot, mag, b


def global_bwd_constants(A, Bs, n, sv, invstd, mean):
    """sync_constants_kernel: P1 = s, P2 = -s invstd Bs / n, P3 = -s A / n - P2 mean in double from the all-reduced A, Bs = `allreduced`
    triples [n_slots, C] and the global rows n [n_slots] (exact: integers below 2^24 carried as floats); a slot with no row on any rank:
    P2 = P3 = 0.  Bars: the output roundings (K = 1) plus the bars of A and Bs carried through."""
    (A, Am, bA), (Bs, Bm, bB) = A, Bs
    sv, invstd, mean = f64(sv), f64(invstd), f64(mean)
    n = f64(n)[:, None]
    live = n > 0
    nn = np.where(live, n, 1.0)
    P2 = np.where(live, -sv * invstd * Bs / nn, 0.0)
    P2m = np.where(live, np.abs(sv * invstd) * Bm / nn, 0.0)
    bP2 = np.where(live, np.abs(sv * invstd) * bB / nn, 0.0)
    P3 = np.where(live, -sv * A / nn - P2 * mean, 0.0)
    P3m = np.where(live, np.abs(sv) * Am / nn + P2m * np.abs(mean), 0.0)
    bP3 = np.where(live, np.abs(sv) * bA / nn + bP2 * np.abs(mean), 0.0)
    return {"P1": (sv, bar(np.abs(sv), sv, 1)), "P2": (P2, bar(P2m, P2, 1) + bP2), "P3": (P3, bar(P3m, P3, 1) + bP3)}


def bn_bwd_finalize_global_ref(ranks, gamma, mean, invstd, n_slots):
    """bn_bwd_finalize under a collective (bwd_misc.hip + sync_bn.hip: sync_pack_kernel, all-reduce, sync_constants_kernel).  ranks = one
    (part_a, part_b, slots, slot_rows) per rank, as bn_bwd_finalize_ref takes them.  A, Bs and n are summed over the ranks and P1, P2, P3
    come from the global sums (equal on every rank); slot_ab stays each rank's own: "slot_ab" is the LIST of the ranks' (value, bar)."""
    own = [bn_bwd_finalize_ref(pa, pb, slots, rows, gamma, mean, invstd, n_slots) for pa, pb, slots, rows in ranks]
    mags = []
    for pa, pb, slots, rows in ranks:
        pa, pb = np.abs(f64(pa)), np.abs(f64(pb))
        mags.append(np.stack([np.stack([pa[np.asarray(slots) == s].sum(0), pb[np.asarray(slots) == s].sum(0)], -1) for s in range(n_slots)]))
    A = allreduced([o["slot_ab"][0][..., 0] for o in own], [m[..., 0] for m in mags])
    Bs = allreduced([o["slot_ab"][0][..., 1] for o in own], [m[..., 1] for m in mags])
    n = sum(f64(rows) for _, _, _, rows in ranks)
    res = global_bwd_constants(A, Bs, n, f64(gamma)[None, :] * f64(invstd), invstd, mean)
    res["slot_ab"] = [o["slot_ab"] for o in own]
    return res


def param_grads_ref(slot_ab):
    """dbeta = sum_slots A, dgamma = sum_slots Bs of slot_ab [S, C, 2]; fp32 sums of S terms."""
    ab = f64(slot_ab)
    S = ab.shape[0]
    s, m = ab.sum(0), np.abs(ab).sum(0)
    return {"dbeta": (s[:, 0], bar(m[:, 0], s[:, 0], S)), "dgamma": (s[:, 1], bar(m[:, 1], s[:, 1], S))}


def fc_act_ref(z, s, t, per):
    """act[row] = relu(z[row] s[row // per] + t[row // per]) on [rows, C]: one fma."""
    z = f64(z)
    grp = np.arange(z.shape[0]) // per
    pre = z * f64(s)[grp] + f64(t)[grp]
    return {"act": (np.maximum(pre, 0.0), bar(np.abs(z * f64(s)[grp]) + np.abs(f64(t)[grp]), pre, 1))}


def fc_bn_bwd_ref(da, z, scale, shift, mean, invstd, n_slots, per):
    """Full BatchNorm + ReLU backward of an FC layer over the `per` rows of each slot: dy = da where z scale + shift > 0 (da of a dead element is
    ignored), A = sum dy, Bs = sum dy zhat, zhat = (z - mean) invstd, g = scale (dy - A / per - zhat Bs / per); slot_ab = (A, Bs).
    `sure`: the elements whose ReLU decision is outside the fp32 bar of the pre-activation (the cases are built with all of them sure).
    The sums are in double (K = 1, zhat formed in fp32: inside mag's 8 eps); g has three fp32 terms and carries the bars of A and Bs."""
    da, z = f64(da), f64(z)
    C = z.shape[1]
    slot = np.arange(z.shape[0]) // per
    sc, sh, mu, iv = (f64(v)[slot] for v in (scale, shift, mean, invstd))
    pre = z * sc + sh
    sure = np.abs(pre) > bar(np.abs(z * sc) + np.abs(sh), pre, 1)
    dy = np.where(pre > 0, da, 0.0)
    zh = (z - mu) * iv
    zhm = (np.abs(z) + np.abs(mu)) * iv
    A, Bs, Am, Bm = (np.zeros((n_slots, C)) for _ in range(4))
    for s in range(n_slots):
        r = slot == s
        A[s], Bs[s], Am[s], Bm[s] = dy[r].sum(0), (dy[r] * zh[r]).sum(0), np.abs(dy[r]).sum(0), (np.abs(dy[r]) * zhm[r]).sum(0)
    bA, bB = bar(Am, A, 1), bar(Bm, Bs, 1)
    an, bn = A[slot] / per, Bs[slot] / per
    g = sc * (dy - an - zh * bn)
    gm = np.abs(sc) * (np.abs(dy) + np.abs(an) + zhm * np.abs(bn))
    bg = bar(gm, g, 3) + np.abs(sc) * (bA[slot] + zhm * bB[slot]) / per
    ab = np.stack([A, Bs], -1)
    return {"g": (g, bg), "slot_ab": (ab, np.stack([bA, bB], -1)), "sure": sure}


def fc_bn_bwd_global_ref(das, zs, scale, shift, mean, invstd, n_slots, pers):
    """fc_bn_bwd under a collective (bwd_misc.hip + sync_bn.hip: sync_fc_apply_kernel): rank r holds per_r = pers[r] rows of every slot
    (da_r, z_r [n_slots * per_r, C]); the constants are the same on every rank.  The means of dy and dy zhat are taken over the ranks' rows
    together: g_r = scale (dy_r - A / n - zhat_r Bs / n) with A, Bs the `allreduced` sums of the ranks' own (A_r, Bs_r) and n = sum pers.
    Returns the LISTS "g", "slot_ab", "sure" of the ranks' results; slot_ab and sure are fc_bn_bwd_ref's of the rank's rows."""
    own = [fc_bn_bwd_ref(da, z, scale, shift, mean, invstd, n_slots, per) for da, z, per in zip(das, zs, pers)]
    mags = []
    for da, z, per, o in zip(das, zs, pers, own):          # the magnitudes of (A_r, Bs_r), as fc_bn_bwd_ref forms them
        da, z = f64(da), f64(z)
        slot = np.arange(z.shape[0]) // per
        sc, sh, mu, iv = (f64(v)[slot] for v in (scale, shift, mean, invstd))
        dy = np.where(z * sc + sh > 0, np.abs(da), 0.0).reshape(n_slots, per, -1)
        zhm = ((np.abs(z) + np.abs(mu)) * iv).reshape(n_slots, per, -1)
        mags.append((dy.sum(1), (dy * zhm).sum(1)))
    A, Am, bA = allreduced([o["slot_ab"][0][..., 0] for o in own], [m[0] for m in mags])
    Bs, Bm, bB = allreduced([o["slot_ab"][0][..., 1] for o in own], [m[1] for m in mags])
    n = float(sum(pers))
    gs = []
    for da, z, per in zip(das, zs, pers):
        da, z = f64(da), f64(z)
        slot = np.arange(z.shape[0]) // per
        sc, sh, mu, iv = (f64(v)[slot] for v in (scale, shift, mean, invstd))
        dy = np.where(z * sc + sh > 0, da, 0.0)
        zh, zhm = (z - mu) * iv, (np.abs(z) + np.abs(mu)) * iv
        an, bn = A[slot] / n, Bs[slot] / n
        g = sc * (dy - an - zh * bn)
        gm = np.abs(sc) * (np.abs(dy) + np.abs(an) + zhm * np.abs(bn))
        gs.append((g, bar(gm, g, 3) + np.abs(sc) * (bA[slot] + zhm * bB[slot]) / n))
    return {"g": gs, "slot_ab": [o["slot_ab"] for o in own], "sure": [o["sure"] for o in own]}


def colsum_ref(x):
    x = f64(x)
    s = x.sum(0)
    return {"out": (s, bar(np.abs(x).sum(0), s, x.shape[0]))}


def reduce_ref(part, dst0=None):
    """dst (=|+=) sum_q part[q] for part [Q, rows, cols]; dst0 = the destination's previous values in the accumulate form."""
    p = f64(part)
    s, m, K = p.sum(0), np.abs(p).sum(0), p.shape[0]
    if dst0 is not None:
        s, m, K = s + f64(dst0), m + np.abs(f64(dst0)), K + 1
    return {"dst": (s, bar(m, s, K))}


def transpose64_ref(src, Q, n_slots, chunks, by_workgroup, add=None):
    """dst[p(q)] = (sum of window q's `chunks` 64 x 64 partials)^T (+ add[p(q)]), p(q) = (q % n_slots) (Q / n_slots) + q / n_slots; the
    partials of window q sit at q * chunks + ch, or (by_workgroup) at ((q / n_slots) * chunks + ch) * n_slots + q % n_slots."""
    src = f64(src).reshape(-1, 64, 64)
    out, mag = np.zeros((Q, 64, 64)), np.zeros((Q, 64, 64))
    for q in range(Q):
        idx = [((q // n_slots) * chunks + ch) * n_slots + q % n_slots if by_workgroup else q * chunks + ch for ch in range(chunks)]
        p = (q % n_slots) * (Q // n_slots) + q // n_slots
        out[p], mag[p] = src[idx].sum(0).T, np.abs(src[idx]).sum(0).T
    if add is not None:
        out, mag = out + f64(add).reshape(Q, 64, 64), mag + np.abs(f64(add).reshape(Q, 64, 64))
    return {"dst": (out, bar(mag, out, chunks + 1))}


# ---- inputs shared by the CPU and GPU tests ----------------------------------------------------------------------------------------------
FC_PER = (1, 2, 8, 63, 64, 65, 200)
FC_C = (40, 256, 512)


def make_fc_bn_bwd(per, C, n_slots=3, seed=0):
    """z, da [n_slots * per, C] and BatchNorm constants of the slots' own statistics; rows the ReLU kills (about half, all of one column, none of
    another) with da non-zero everywhere.  fp32 arrays."""
    rng = np.random.default_rng(1000 * per + C + seed)
    rows = n_slots * per
    z = (rng.standard_normal((rows, C)) * (0.5 + rng.random(C)) + rng.standard_normal(C)).astype(np.float32)
    da = rng.standard_normal((rows, C)).astype(np.float32)
    gamma = (rng.standard_normal(C) * 0.8).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.3).astype(np.float32)
    beta[0], beta[1] = -50.0, 50.0                                             # column 0 all dead, column 1 all alive
    gamma[0], gamma[1] = abs(gamma[0]) + 0.1, abs(gamma[1]) + 0.1
    zz = f64(z).reshape(n_slots, per, C)
    mean = zz.mean(1)
    invstd = 1.0 / np.sqrt(zz.var(1) + BN_EPS)
    scale = gamma[None, :] * invstd
    shift = beta[None, :] - mean * scale
    return {"z": z, "da": da, "scale": scale.astype(np.float32), "shift": shift.astype(np.float32), "mean": mean.astype(np.float32),
            "invstd": invstd.astype(np.float32), "gamma": gamma, "beta": beta, "per": per, "C": C, "n_slots": n_slots}


FC_PERS = ((5, 3), (70, 57))          # rows of every slot on rank 0 | rank 1 (production shards are equal; the kernel takes n from the exchange)
FC_SLOTS = (1, 3)


def make_fc_bn_bwd_ranks(pers, C, n_slots, seed=1):
    """make_fc_bn_bwd at sum(pers) rows per slot -- the constants are the statistics of the WHOLE batch, the same on every rank -- dealt to
    the ranks: rank r gets rows sum(pers[:r]) .. + pers[r] of every slot.  One dict per rank.  (Seed 1: with seed 0 one element of the
    127-row, 512-channel case has its ReLU decision inside the fp32 bar; tests/test_bn_refs_cpu.py checks that every case is decided.)"""
    c = make_fc_bn_bwd(sum(pers), C, n_slots, seed)
    res, o = [], 0
    for per in pers:
        cut = lambda x: np.ascontiguousarray(x.reshape(n_slots, sum(pers), C)[:, o:o + per].reshape(n_slots * per, C))
        res.append(dict(c, z=cut(c["z"]), da=cut(c["da"]), per=per))
        o += per
    return res
