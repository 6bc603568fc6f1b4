"""Layer-local float64 oracle of the GRU recurrence (csrc/gru_head.hip: gru_seq_kernel, gru_seq_bwd_kernel) and of the classification head's
own kernels (csrc/cls_head.hip: cls_mix, cls_weights, cls_bn_act, cls_out, cls_mix_bwd).

The C side is ampnet_probe_seq_f32 (include/ampnet_hip.h, "test hooks"; csrc/layer_probe.hip): ONE launch of one of them, selected by `op`,
through the launch wrappers the product entry points call, on buffers the test chose, every extent checked on the host first.  This module
holds the ctypes mirror of AmpnetSeqProbe and a float64 restatement of each operation, written from the reference model
(pointNet/model/pointnetAtt.py:115-151, 212-258) and torch's definition of nn.GRU (gate order r, z, n), on the fp32 inputs.  Every restatement
returns {output name: (float64 value, bar)}; `dt=np.float32` evaluates the same formulas in fp32 numpy for tests/test_seq_refs_cpu.py, which
also holds the restatements to torch in float64.  Host side only; the GPU tests are tests/test_gru_cls_layers_gpu.py.

Bars (eps = 2^-24; pw_probe.bar(mag, x, K) = 8 eps sqrt(K) mag + 2 eps |x|)
  gate pre-activations      gi_g + b_hh,g + sum_k W_hh[g, k] h_k: K = 64 products + the bias + gi = 66, mag = the sum of the absolute terms;
                            in the chained form sum_k |W_hh[g, k]| bar(h_k) is carried in
  sigmoid                   s = 1 / (1 + __expf(-x)): d s / d e = -s^2, so a relative error rho of e = exp(-x) moves s by s (1 - s) rho,
                            rho = (2 |x| + FAST_EXP_ULP) eps (head_probe.py: measured for __expf); 4 eps s for the sum and the reciprocal;
                            s (1 - s) bar(x) for the argument; 2^-126 absolute (a result under the smallest normal may be flushed to 0)
  tanh                      n = tanhf(x): TANH_ULP eps |n| + (1 - n^2) bar(x) + 2^-126.  TANH_ULP = 4 assumes a 1-ulp function, as EXP_ULP = 4
                            did; tests/test_gru_cls_layers_gpu.py::test_tanh_sigmoid_sweep measures tanhf and the kernel's sigmoid on ~4100
                            points of [-90, 90] against float64 and requires the worst error <= 0.5 of these bars.
                            Measured on the MI355X: tanhf 1.76 eps worst relative error (x = 0.655), 0.44 of its bar: the 4 stands; the
                            sigmoid 63.6 eps worst (x = -86.8, the error of __expf), 0.46 of its bar with FAST_EXP_ULP = 21: stands.
  n's argument              fma(r, gh_n, gi_n): bar(|r gh_n| + |gi_n|, x, 1) + |gh_n| bar(r) + r bar(gh_n)
  h                         fma(z, h' - n, n): (1 - z) bar(n) + |h' - n| bar(z) + 3 eps |z (h' - n)| + 2 eps |n| + 2 eps |h| (+ z bar(h') chained)
  backward                  dh = dH + dh_next: bar(dh_next) + eps |dh|.  1 - n^2 in fp32 of the given n: eps n^2 absolute (the product) beside the
                            relative roundings, so bar(dnp) = |(1 - z)(1 - n^2)| bar(dh) + eps |dh (1 - z)| n^2 + 4 eps |dnp|;
                            dzp (hp - n, 1 - z, three products): |(hp - n) z (1 - z)| bar(dh) + 6 eps |dzp|; drp = dnp gh_n r (1 - r):
                            |gh_n r (1 - r)| bar(dnp) + 5 eps |drp|; dnr = dnp r: r bar(dnp) + eps |dnr|;
                            dh_next = dh z + the K = 192 contraction: bar(mag, x, 193) + sum |W_hh| bar(operand) + z bar(dh).  Chained only.
  cls_mix / cls_out / cwpart  bar with K = W + 1, 129, 256; d_o one product: bar(|x|, x, 1)
  cls_weights               8 terms of p keep / (1 - drop_p) (one product each): K = 9
  cls_bn_act                z + b2 is one fp32 addition (compared bitwise).  The statistics are summed in double: K = 1, only the roundings of
                            the outputs remain; shift, act carry the bars of scale / mean through; running update 0.9f r + 0.1f (float) m:
                            0.1 bar(m) + 2 eps |result|
  ReLU decisions            an element is compared where |pre-activation| > its bar; elsewhere it must be 0 or within the bar of the unmasked
                            value (`sure`); at most 1 % of a case may be undecided; a pre-activation that is exactly 0 in float64 by
                            construction is decided.  cls_mix_bwd decides by its INPUT x > 0: exact.
"""
import ctypes

import numpy as np
import torch

import pw_probe as PP
from pw_probe import EPS32, L, bar
from head_probe import FAST_EXP_ULP, TINY

EPS = EPS32
TANH_ULP = 4.0
H = 64                                               # GRU_H
G3 = 3 * H
CLS_HID, HEADS, E = 128, 8, 256
HEAD_MAX_W, CLS_MAX_CLASSES = 32, 16
BN_EPS = 1e-5                                        # cls_bn_act adds it in double
MOM9, MOM1 = float(np.float32(0.9)), float(np.float32(0.1))
AMPNET_E_ARG = PP.AMPNET_E_ARG
OPS = {"gru_seq": 0, "gru_seq_bwd": 1, "cls_mix": 2, "cls_weights": 3, "cls_bn_act": 4, "cls_out": 5, "cls_mix_bwd": 6, "sweep": 7}
KERNEL = {0: "gru_seq_kernel", 1: "gru_seq_bwd_kernel", 2: "cls_mix_kernel", 3: "cls_weights_kernel", 4: "cls_bn_act_kernel", 5: "cls_out_kernel",
          6: "cls_mix_bwd_kernel", 7: "gru_act_sweep"}

_p, _i64, _i32, _u32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_float
POINTERS = ("gi", "Whh", "bhh", "h_out", "gates", "dH", "h_all", "dgi", "dgh", "hprev_out", "o", "cw", "cb", "x", "probs", "wout", "z", "b2",
            "gamma", "beta", "rmean", "rvar", "scale", "shift", "mean", "invstd", "act", "W3", "b3", "out", "dx", "d_o", "cwpart", "X", "Y")


class SeqProbe(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("op", "B", "W", "C", "train", "rows")] + [("drop_p", _f32), ("drop_seed", _u32)] + \
               [x for n in POINTERS for x in ((n, _p), (n + "_n", _i64))]


EXTENTS = {n: n + "_n" for n in POINTERS}


def set_tensors(desc, **tensors):
    PP.set_tensors(desc, EXTENTS, **tensors)


def new(op, **ints):
    d = SeqProbe()
    d.op = OPS[op]
    for k, v in ints.items():
        setattr(d, k, v)
    return d


def run(desc):
    """(return code, kernel names recorded) of one ampnet_probe_seq_f32 call, synchronised."""
    lib = L.lib()
    lib.ampnet_probe_seq_f32.argtypes = [ctypes.POINTER(SeqProbe), ctypes.c_void_p]
    lib.ampnet_profile_enable(1)
    try:
        rc = lib.ampnet_probe_seq_f32(ctypes.byref(desc), L.stream_ptr())
        torch.cuda.synchronize()
        names = PP.profile_names(lib)
    finally:
        lib.ampnet_profile_enable(0)
    return rc, names


def f64(x):
    return np.asarray(x, dtype=np.float64)


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def A(x):
    return np.abs(f64(x))


def worst(x, ref):
    """worst |x - value| / bar of a (value, bar) pair; finite x required; an element with error 0 counts 0."""
    want, b = ref
    x = f64(x)
    assert x.shape == np.shape(want), (x.shape, np.shape(want))
    assert np.all(np.isfinite(x)), "non-finite where the contract writes"
    err = np.abs(x - f64(want))
    b = np.broadcast_to(f64(b), err.shape)
    r = np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))
    return float(r.max()) if r.size else 0.0


def worst_relu(got, pre_ref, sure):
    """The ReLU rule: where `sure`, relu(pre) at pre's bar; elsewhere 0 or within the bar of the unmasked value.  Returns the worst ratio."""
    pre, b = pre_ref
    got = f64(got)
    assert np.all(np.isfinite(got)), "non-finite where the contract writes"
    r = worst(np.where(sure, got, 0.0), (np.where(sure, np.maximum(f64(pre), 0.0), 0.0), b))
    un = ~sure
    assert np.all((got[un] == 0) | (np.abs(got[un] - f64(pre)[un]) <= np.broadcast_to(b, got.shape)[un])), "an undecided element is neither 0 nor the value"
    return r


# ---- the device functions ---------------------------------------------------------------------------------------------------------------
def sigmoid_ref(x, bx=0.0, dt=np.float64):
    """(s, bar) of 1 / (1 + exp(-x)) for an argument x carrying the bar bx."""
    x = np.asarray(x, dtype=dt)
    with np.errstate(over="ignore"):
        s = (dt(1) / (dt(1) + np.exp(-x))).astype(dt)
    s64 = f64(s)
    return s, s64 * (1.0 - s64) * ((2.0 * A(x) + FAST_EXP_ULP) * EPS + bx) + 4.0 * EPS * s64 + TINY


def tanh_ref(x, bx=0.0, dt=np.float64):
    x = np.asarray(x, dtype=dt)
    n = np.tanh(x).astype(dt)
    n64 = f64(n)
    return n, TANH_ULP * EPS * np.abs(n64) + (1.0 - n64 * n64) * bx + TINY


def sweep_points():
    """~4100 points of [-90, 90]: a uniform grid, a log-spaced set dense near 0 on both sides, 0 and the overflow edges of __expf."""
    lin = np.linspace(-90.0, 90.0, 2049)
    log = np.logspace(-6, np.log10(20.0), 1024)
    x = np.concatenate([lin, log, -log, [0.0, 87.0, -87.0, 88.5, -88.5, 89.0, -89.0, 30.0, -30.0]])
    return f32(x)


# ---- the GRU recurrence ---------------------------------------------------------------------------------------------------------------------
def gru_fwd_ref(gi, Whh, bhh, B, W, h_given=None, dt=np.float64):
    """r, z, n, ghn (= W_hn h + b_hn), h [B, W, 64] each with its bar.  h_given [B * W, 64]: step t starts from h_given's row t - 1 (the kernel's own
    fp32 state: the step-local form, no error compounds); None: chained from h = 0 with the bar of h carried step to step to first order."""
    gi = np.asarray(gi, dtype=dt).reshape(B, W, G3)
    Wm, bh = np.asarray(Whh, dtype=dt).reshape(G3, H), np.asarray(bhh, dtype=dt).reshape(G3)
    aW = A(Wm)
    out = {k: (np.zeros((B, W, H), dtype=dt), np.zeros((B, W, H))) for k in ("r", "z", "n", "ghn", "h")}
    hg = None if h_given is None else np.asarray(h_given, dtype=dt).reshape(B, W, H)
    h, bh_prev = np.zeros((B, H), dtype=dt), np.zeros((B, H))
    for t in range(W):
        if hg is not None:
            h, bh_prev = (hg[:, t - 1] if t > 0 else np.zeros((B, H), dtype=dt)), np.zeros((B, H))
        a = (h @ Wm.T + bh).astype(dt)                                           # [B, 192]
        am = A(h) @ aW.T + A(bh)
        carried = bh_prev @ aW.T
        pre_rz = (gi[:, t, :2 * H] + a[:, :2 * H]).astype(dt)
        b_rz = bar(am[:, :2 * H] + A(gi[:, t, :2 * H]), f64(pre_rz), H + 2) + carried[:, :2 * H]
        s, bs = sigmoid_ref(pre_rz, b_rz, dt)
        r, z, br, bz = s[:, :H], s[:, H:], bs[:, :H], bs[:, H:]
        an = a[:, 2 * H:]
        ban = bar(am[:, 2 * H:], f64(an), H + 1) + carried[:, 2 * H:]
        pre_n = (gi[:, t, 2 * H:] + r * an).astype(dt)
        bpn = bar(A(r * an) + A(gi[:, t, 2 * H:]), f64(pre_n), 1) + A(an) * br + A(r) * ban
        n, bn = tanh_ref(pre_n, bpn, dt)
        hn = (n + z * (h - n)).astype(dt)
        bhn = A(1.0 - f64(z)) * bn + A(h - n) * bz + 3 * EPS * A(z * (h - n)) + 2 * EPS * A(n) + 2 * EPS * A(hn) + A(z) * bh_prev
        for k, v, b in (("r", r, br), ("z", z, bz), ("n", n, bn), ("ghn", an, ban), ("h", hn, bhn)):
            out[k][0][:, t], out[k][1][:, t] = v, b
        h, bh_prev = hn, bhn
    return out


def pack_gates(ref):
    """gates [B * W, 256] = (r, z, n, ghn) of a gru_fwd_ref result, as fp32."""
    B, W, _ = ref["r"][0].shape
    return f32(np.concatenate([f64(ref[k][0]) for k in ("r", "z", "n", "ghn")], axis=2).reshape(B * W, 4 * H))


def gru_bwd_ref(dH, gates, h_all, Whh, B, W, dt=np.float64):
    """dgi, dgh [B * W, 192] and hprev [B * W, 64] by back-propagation through time from the given gates and hidden states; bars chained."""
    dH = np.asarray(dH, dtype=dt).reshape(B, W, H)
    g = np.asarray(gates, dtype=dt).reshape(B, W, 4, H)
    ha = np.asarray(h_all, dtype=dt).reshape(B, W, H)
    Wm = np.asarray(Whh, dtype=dt).reshape(G3, H)
    aW = A(Wm)
    dgi, dgh, bgi, bgh = (np.zeros((B, W, G3), dtype=dt if i < 2 else np.float64) for i in range(4))
    hprev = np.zeros((B, W, H), dtype=dt)
    dhn, bdhn = np.zeros((B, H), dtype=dt), np.zeros((B, H))
    for t in range(W - 1, -1, -1):
        r, z, n, ghn = g[:, t, 0], g[:, t, 1], g[:, t, 2], g[:, t, 3]
        hp = ha[:, t - 1] if t > 0 else np.zeros((B, H), dtype=dt)
        dh = (dH[:, t] + dhn).astype(dt)
        bdh = bdhn + EPS * A(dh)
        omz, omn = (dt(1) - z).astype(dt), (dt(1) - n * n).astype(dt)
        dnp = (dh * omz * omn).astype(dt)
        bdnp = A(omz * omn) * bdh + EPS * A(dh * omz) * f64(n) ** 2 + 4 * EPS * A(dnp)
        dzp = (dh * (hp - n) * z * omz).astype(dt)
        bdzp = A((hp - n) * z * omz) * bdh + 6 * EPS * A(dzp)
        k_r = (ghn * r * (dt(1) - r)).astype(dt)
        drp = (dnp * k_r).astype(dt)
        bdrp = A(k_r) * bdnp + 5 * EPS * A(drp)
        dnr = (dnp * r).astype(dt)
        bdnr = A(r) * bdnp + EPS * A(dnr)
        d3 = np.concatenate([drp, dzp, dnr], axis=1)                              # [B, 192]: what W_hh h + b_hh receives
        b3 = np.concatenate([bdrp, bdzp, bdnr], axis=1)
        dgi[:, t], bgi[:, t] = np.concatenate([drp, dzp, dnp], axis=1), np.concatenate([bdrp, bdzp, bdnp], axis=1)
        dgh[:, t], bgh[:, t] = d3, b3
        hprev[:, t] = hp
        dhn = (dh * z + d3 @ Wm).astype(dt)
        bdhn = bar(A(dh * z) + A(d3) @ aW, f64(dhn), G3 + 1) + b3 @ aW + A(z) * bdh
    rs = lambda a, c: a.reshape(B * W, c)
    return {"dgi": (rs(dgi, G3), rs(bgi, G3)), "dgh": (rs(dgh, G3), rs(bgh, G3)), "hprev": (rs(hprev, H), np.zeros((B * W, H)))}


# ---- the classification head ----------------------------------------------------------------------------------------------------------------
def seq_first_view(o, B, W):
    """The reference's attn_output.view(-1, W, 256) of the sequence-first [W, B, 256] tensor whose token (b, w) is row b W + w of o."""
    seq_first = np.ascontiguousarray(np.asarray(o).reshape(B, W, E).transpose(1, 0, 2))      # [W, B, 256]
    return seq_first.reshape(-1, W, E)                                                       # [B, W, 256]: memory re-read, not a transpose


def cls_mix_ref(o, cw, cb, B, W, dt=np.float64):
    """x [B, 256] = relu(conv_1(view)): pre (value, bar), `sure`, `zero` (pre-activation exactly 0 in float64: decided, x == 0)."""
    v = seq_first_view(np.asarray(o, dtype=dt), B, W)
    cw, cb = np.asarray(cw, dtype=dt).reshape(W), np.asarray(cb, dtype=dt).reshape(())
    pre = ((v * cw[None, :, None]).sum(1) + cb).astype(dt)
    mag = (A(v) * A(cw)[None, :, None]).sum(1) + A(cb)
    b = bar(mag, f64(pre), W + 1)
    zero = mag == 0.0
    return {"pre": (pre, b), "sure": (np.abs(f64(pre)) > b) | zero, "zero": zero}


def cls_mix_bwd_ref(dx, x, o, cw, B, W, dt=np.float64):
    """d_o [B * W, 256] and cwpart [B, W + 1] (column W: the bias) of the conv_1 + ReLU backward, decided by the given x > 0."""
    dx, x = np.asarray(dx, dtype=dt).reshape(B, E), np.asarray(x, dtype=dt).reshape(B, E)
    cw = np.asarray(cw, dtype=dt).reshape(W)
    v = seq_first_view(np.asarray(o, dtype=dt), B, W)
    dpre = np.where(x > 0, dx, dt(0)).astype(dt)
    dview = (cw[None, :, None] * dpre[:, None, :]).astype(dt)                               # [B, W, 256], gradient of the view
    d_seq_first = dview.reshape(W, B, E)                                                     # the view's memory IS the [W, B, 256] tensor's
    d_o = np.ascontiguousarray(d_seq_first.transpose(1, 0, 2)).reshape(B * W, E)
    part = np.concatenate([(dpre[:, None, :] * v).sum(2), dpre.sum(1, keepdims=True)], axis=1).astype(dt)
    pm = np.concatenate([(A(dpre)[:, None, :] * A(v)).sum(2), A(dpre).sum(1, keepdims=True)], axis=1)
    return {"d_o": (d_o, bar(A(d_o), f64(d_o), 1)), "cwpart": (part, bar(pm, f64(part), E))}


def cls_weights_ref(probs, B, W, drop_p=0.0, key=None, dt=np.float64):
    """out [B, W, W] = mean over the 8 heads of keep p / (1 - drop_p); keep = oracle.keep_mask over the flat [B, 8, W, W] index."""
    from oracle.ampnet_oracle import keep_mask
    p = np.asarray(probs, dtype=dt).reshape(B, HEADS, W, W)
    if drop_p > 0:
        keep = keep_mask(key[0], key[1], B * HEADS * W * W, drop_p).reshape(B, HEADS, W, W)
        p = np.where(keep, p * dt(PP.dscale32(drop_p)), dt(0)).astype(dt)
    out = (p.sum(1) * dt(1.0 / HEADS)).astype(dt)
    return {"out": (out, bar(A(p).sum(1) / HEADS, f64(out), HEADS + 1))}


def cls_bn_act_ref(z, b2, gamma, beta, rmean, rvar, B, train, dt=np.float64):
    """v = fp32(z + b2); train: mean / biased variance of v over the B rows, running update with the unbiased variance (B == 1: with the sum of
    squares itself, 0); eval: the running statistics.  scale = gamma invstd, shift = beta - mean scale, act = relu(v scale + shift)."""
    v = (f64(z).reshape(B, CLS_HID) + f64(b2)[None, :]).astype(np.float32)                 # one fp32 addition, exactly
    v64 = f64(v)
    gamma, beta = np.asarray(gamma, dtype=dt), np.asarray(beta, dtype=dt)
    res = {"v": (v, np.zeros_like(v64))}
    if train:
        m64 = v64.mean(0)                                                                # the contract: sums over the rows in double,
        q64 = ((v64 - m64) ** 2).sum(0)                                                  # whatever dt evaluates the rest
        m, q = m64.astype(dt), q64.astype(dt)
        var = (q64 / B).astype(dt)
        bm = bar(A(v).mean(0), f64(m), 1)
        uv = (q64 / (B - 1)).astype(dt) if B > 1 else q
        for name, r0, stat, bst in (("rmean", rmean, m, bm), ("rvar", rvar, uv, bar(A(uv), f64(uv), 1))):
            new = (dt(MOM9) * np.asarray(r0, dtype=dt) + dt(MOM1) * stat).astype(dt)
            res[name] = (new, MOM1 * bst + 2 * EPS * A(new))
    else:
        m, var = np.asarray(rmean, dtype=dt), np.asarray(rvar, dtype=dt)
        bm = np.zeros(CLS_HID)
        res["rmean"], res["rvar"] = (f64(rmean), np.zeros(CLS_HID)), (f64(rvar), np.zeros(CLS_HID))
    inv = (dt(1) / np.sqrt(var + dt(BN_EPS))).astype(dt)
    sc = (gamma * inv).astype(dt)
    sh = (beta - m * sc).astype(dt)
    b_inv = bar(A(inv), f64(inv), 1)
    b_sc = bar(A(sc), f64(sc), 1) + A(gamma) * b_inv
    b_sh = bar(A(beta) + A(m * sc), f64(sh), 1) + A(m) * b_sc + A(sc) * bm
    pre = (v.astype(dt) * sc[None, :] + sh[None, :]).astype(dt)
    b_pre = bar(A(v64 * f64(sc)) + A(sh), f64(pre), 1) + A(v64) * b_sc + b_sh
    res.update(scale=(sc, b_sc), shift=(sh, b_sh), mean=(m, bm + EPS * A(m)), invstd=(inv, b_inv), pre=(pre, b_pre),
               sure=np.abs(f64(pre)) > b_pre)
    return res


def cls_out_ref(act, W3, b3, dt=np.float64):
    act, W3, b3 = (np.asarray(t, dtype=dt) for t in (act, W3, b3))
    out = (act @ W3.T + b3).astype(dt)
    return {"out": (out, bar(A(act) @ A(W3).T + A(b3), f64(out), CLS_HID + 1))}


# ================================================================================================================================
# the committed cases: inputs as numpy fp32, shared by the GPU tests and tests/test_seq_refs_cpu.py
# ================================================================================================================================
def rng(seed):
    return np.random.default_rng(seed)


GRU_B, GRU_W = (1, 3), (1, 2, 3, 17, 32)
GRU_VARIANTS = ("normal", "strong", "saturated")


def make_gru(B, W, variant, seed=0):
    """gi [B * W, 192] with |gi| <= 2, Whh uniform in +-1/8 (strong: +-1), bhh in +-1/4.  saturated: a third of the gate inputs at +-30 and +-100
    (the r / z inputs of units 0 .. 20 at +-100 and of units 21 .. 41 at +-30, the n inputs of units 0 .. 20 at +-30, signs drawn)."""
    g = rng(100 * W + 10 * B + GRU_VARIANTS.index(variant) + seed)
    gi = f32(g.uniform(-2, 2, (B * W, G3)))
    Whh = f32(g.uniform(-1, 1, (G3, H)) * (1.0 if variant == "strong" else 0.125))
    bhh = f32(g.uniform(-0.25, 0.25, G3))
    if variant == "saturated":
        sg = lambda n: g.choice([-1.0, 1.0], (B * W, n))                                 # noqa: E731
        for base in (0, H):
            gi[:, base:base + 21] = 100.0 * sg(21)
            gi[:, base + 21:base + 42] = 30.0 * sg(21)
        gi[:, 2 * H:2 * H + 21] = 30.0 * sg(21)
    return dict(gi=gi, Whh=Whh, bhh=bhh, B=B, W=W)


GRU_BWD_VARIANTS = ("plain", "small_r", "last_only")


def make_gru_bwd(B, W, variant, seed=0):
    """The float64 forward of a case whose last hidden state is far from 0 (z near 0 and |n| near 1 at the last step), rounded to fp32: gates, h_all;
    dH [B * W, 64].  small_r: r < 0.2 everywhere (the r inputs shifted by -5); last_only: dH zero except at the last step of every sample."""
    g = rng(7000 + 100 * W + 10 * B + GRU_BWD_VARIANTS.index(variant) + seed)
    gi = f32(g.uniform(-2, 2, (B * W, G3)))
    Whh = f32(g.uniform(-1, 1, (G3, H)) * 0.125)
    bhh = f32(g.uniform(-0.25, 0.25, G3))
    if variant == "small_r":
        gi[:, :H] -= 5.0
    last = np.arange(B) * W + W - 1
    gi[last, H:2 * H] -= 4.0                                                               # z small: the last h is (almost) n
    gi[last, 2 * H:] = f32(g.choice([-1.0, 1.0], (B, H)) * g.uniform(1.5, 2.5, (B, H)))     # |n| > 0.8
    fw = gru_fwd_ref(gi, Whh, bhh, B, W)
    dH = f32(g.standard_normal((B * W, H)))
    if variant == "last_only":
        keep = np.zeros(B * W, dtype=bool)
        keep[last] = True
        dH[~keep] = 0.0
    return dict(gi=gi, Whh=Whh, bhh=bhh, gates=pack_gates(fw), h_all=f32(f64(fw["h"][0]).reshape(B * W, H)), dH=dH, B=B, W=W)


CLS_BW = ((1, 1), (1, 32), (2, 3), (3, 2), (4, 6), (6, 4), (7, 5), (5, 32))
CLS_WEIGHTS_BW = CLS_BW[:-1] + ((2, 32),)


def make_cls_mix(B, W, seed=0):
    """o [B * W, 256], cw [W] with negative entries and (W > 1) one exact zero, cb; columns 5 and 77 of o are exactly 0 and, for even B, cb = 0:
    x is exactly 0 there.  dx [B, 256] for the backward; x for the backward = the float64 forward rounded (about half exactly 0)."""
    g = rng(300 + 40 * B + W + seed)
    o = f32(g.standard_normal((B * W, E)))
    o[:, [5, 77]] = 0.0
    cw = f32(g.uniform(-1, 1, W))
    cw[0] = -abs(cw[0]) - 0.1
    if W > 1:
        cw[W // 2] = 0.0
    cb = f32([0.0 if B % 2 == 0 else 0.25])
    fw = cls_mix_ref(o, cw, cb, B, W)
    return dict(o=o, cw=cw, cb=cb, dx=f32(g.standard_normal((B, E))), x=f32(np.maximum(f64(fw["pre"][0]), 0.0)), B=B, W=W)


def make_cls_weights(B, W, seed=0):
    """softmax rows [B, 8, W, W]; for W > 1 the last key of sample 0 and the first key of the last sample are masked: exact zeros."""
    g = rng(500 + 40 * B + W + seed)
    s = g.standard_normal((B, HEADS, W, W)) * 2
    if W > 1:
        s[0, :, :, W - 1] = -np.inf
        s[B - 1, :, :, 0] = -np.inf
    e = np.exp(s - s.max(-1, keepdims=True))
    return dict(probs=f32(e / e.sum(-1, keepdims=True)), B=B, W=W, key=(seed + 3, 0))


BN_B = (1, 2, 3, 8, 33)


def make_cls_bn(B, seed=0):
    """z [B, 128], b2; gamma with negative entries and gamma[3] = 0; channel 7: mean 300 against a spread of 0.01 (mean^2 >> variance);
    running statistics of the sign of the batch's."""
    g = rng(900 + B + seed)
    z = f32(g.standard_normal((B, CLS_HID)) * (0.5 + g.random(CLS_HID)) + g.standard_normal(CLS_HID))
    z[:, 7] = f32(300.0 + 0.01 * g.standard_normal(B))
    b2 = f32(g.uniform(-0.5, 0.5, CLS_HID))
    gamma = f32(g.uniform(0.5, 1.5, CLS_HID) * np.where(np.arange(CLS_HID) % 5 == 2, -1, 1))
    gamma[3] = 0.0
    beta = f32(g.uniform(-0.5, 0.5, CLS_HID))
    m = (f64(z) + f64(b2)).mean(0)
    rmean = f32(m * g.uniform(0.2, 1.5, CLS_HID))
    rvar = f32(g.uniform(0.5, 2.0, CLS_HID))
    rvar[7] = 1e-4
    return dict(z=z, b2=b2, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar, B=B)


OUT_C, OUT_B = (1, 2, 5, 16), (1, 3)


def make_cls_out(B, C, seed=0):
    g = rng(1300 + 20 * B + C + seed)
    return dict(act=f32(np.maximum(g.standard_normal((B, CLS_HID)), 0.0)), W3=f32(g.uniform(-1, 1, (C, CLS_HID)) / 8), b3=f32(g.uniform(-0.5, 0.5, C)),
                B=B, C=C)
