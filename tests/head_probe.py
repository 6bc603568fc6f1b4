"""Layer-local float64 oracle of the segmentation head's own kernels, the loss tail and Adam.

The C side is ampnet_probe_head_f32 (include/ampnet_hip.h, "test hooks"; csrc/layer_probe.hip): ONE launch of posenc_tokens, attention_core,
attention_core_bwd, head_logits (+ loss_finalize), head_out_bwd, sgemm_linear_bwd or sgemm_wgrad_bias on buffers the test chose, every extent
checked on the host first.  This module holds the ctypes mirror of AmpnetHeadProbe and a float64 restatement of each operation, written from
the kernels' comments (csrc/attention.hip, head_bwd.hip, loss.hip, adam.hip) and pointNet/model/pointnetAtt.py:176-209, on the fp32 inputs.
Every restatement returns {output name: (float64 value, bar)}; `dt=np.float32` evaluates the same formulas in fp32 numpy (BLAS / pairwise
summation orders, not the kernels') for tests/test_head_refs_cpu.py.  Host side only; the GPU tests are tests/test_head_layers_gpu.py and
tests/test_loss_adam_gpu.py.

Bars (eps = 2^-24)
  contraction of length K   pw_probe.bar: 8 eps sqrt(K) sum|u||v| + 2 eps |x64|, plus the bars of rounded operands carried through the sum
                            (K = 32 scores, W context / dq / dk / dv, C da3, rows dW / db / part_a / part_b, 16 and 2 positional encoding)
  exp / log                 relative error of f(x) <= (2 |x| + EXP_ULP) eps: one rounding of the argument (|x| eps) and the function itself;
                            for exp(s - m) of computed scores additionally bar(s_j) + max_j bar(s_j) (the error of the argument).
                            EXP_ULP = 4 assumes a 1-ulp function; test_head_layers_gpu.py::test_exp_log_sweep measures __expf, expf and
                            logf on the device against float64 and requires the worst error <= 0.5 of this.  Measured on the MI355X:
                            expf 1.38 eps and logf 3.00 eps worst (0.24 and 0.48 of the bar: the 4 stands); __expf (attention_core) grows
                            as ~1.23 |x| eps, 64.56 eps worst at |x| = 87, 0.59 of (2|x| + 4) eps: it missed, so its constant is the
                            smallest that the float64 sweep supports, FAST_EXP_ULP = 21 (max over x of 2 rel / eps - 2 |x| = 20.47).
  softmax                   rel(p_j) = rel(e_j) + sum_k p_k rel(e_k) + (n + 3) eps   (n terms summed, one reciprocal, one product),
                            plus 2^-126 absolute: an exponential under the smallest normal fp32 may be flushed to 0
  masks                     an element the ReLU decides is compared where |pre-activation| > its bar 2 eps (|z s| + |t|) (one fma);
                            elsewhere it must be 0 or within the bar of the unmasked value.  Sums over rows carry |value| of such elements.
  Adam                      see adam_ref.
"""
import ctypes
import math

import numpy as np
import torch

import pw_probe as PP
from pw_probe import EPS32, L, bar, keep_mask

EPS = EPS32
EXP_ULP = 4.0
FAST_EXP_ULP = 21.0                                   # __expf: measured, see the docstring
TINY = 2.0 ** -126                                    # smallest normal fp32: an exponential below it may be flushed to 0
QSCALE = float(np.float32(0.17677669529663687))      # attention.hip: 1 / sqrt(32) as the fp32 constant
LEAK = float(np.float32(0.01))                       # F.leaky_relu_ slope as the fp32 constant
HEADS, D, E = 8, 32, 256
HL_ROWS, HB_ROWS = 256, 1024                         # head.h: HEAD_LOGITS_ROWS, HEAD_OUT_BWD_ROWS
AMPNET_E_ARG = PP.AMPNET_E_ARG

_p, _i64, _i32, _u32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_float


def _pn(*names):
    return [x for n in names for x in ((n, _p), (n + "_n", _i64))]


class HeadProbe(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("op", "B", "W", "Q", "R", "P", "C", "ldz4", "z_bf16", "rows", "n_out", "n_in", "ldg", "ldx", "ldw", "lddw",
                                    "lddx", "pad0")] + \
               [("drop_p", _f32), ("drop_seed", _u32)] + \
               [(n, _p) for n in ("gl", "cent", "w1", "b1", "w2", "b2")] + [(n + "_n", _i64) for n in ("gl", "cent", "w1", "b1", "w2", "b2")] + \
               [("tok", _p), ("hid", _p), ("slope", _p), ("tok_n", _i64), ("hid_n", _i64)] + \
               _pn("qkv", "mask", "probs", "ctx", "dctx", "dqkv", "z4", "logits", "targets", "class_w", "preds", "loss_part", "loss_out",
                   "dlogits", "z3") + \
               [(n, _p) for n in ("scale", "shift", "mean", "invstd")] + [("bn_n", _i64)] + \
               _pn("w4", "dy3") + [("part_a", _p), ("part_b", _p), ("part_n", _i64)] + \
               _pn("w4part", "G", "X", "Wl", "dW", "dX", "db", "dx_mul")


EXTENTS = {n: n + "_n" for n in ("gl", "cent", "w1", "b1", "w2", "b2", "tok", "qkv", "mask", "probs", "ctx", "dctx", "dqkv", "z4", "logits",
                                 "targets", "class_w", "preds", "loss_part", "loss_out", "dlogits", "z3", "w4", "dy3", "w4part", "G", "X", "Wl",
                                 "dW", "dX", "db", "dx_mul")}
EXTENTS.update(hid="hid_n", slope="hid_n", scale="bn_n", shift="bn_n", mean="bn_n", invstd="bn_n", part_a="part_n", part_b="part_n")


def set_tensors(desc, **tensors):
    PP.set_tensors(desc, EXTENTS, **tensors)


def run(desc):
    """(return code, kernel names recorded) of one ampnet_probe_head_f32 call, synchronised."""
    lib = L.lib()
    lib.ampnet_probe_head_f32.argtypes = [ctypes.POINTER(HeadProbe), ctypes.c_void_p]
    lib.ampnet_profile_enable(1)
    try:
        rc = lib.ampnet_probe_head_f32(ctypes.byref(desc), L.stream_ptr())
        torch.cuda.synchronize()
        names = PP.profile_names(lib)
    finally:
        lib.ampnet_profile_enable(0)
    return rc, names


def f64(x):
    return np.asarray(x, dtype=np.float64)


def exp_rel(x, ulp=EXP_ULP):
    """relative error bound of an fp32 exp / log of the rounded argument x."""
    return (2.0 * np.abs(x) + ulp) * EPS


def keep_flat(key, n, p):
    """keep[i], i = the flat element index the kernel hashes; key = the oracle's (seed, stream) pair (pw_probe.drop_base gives the kernel's base)."""
    return np.ones(n, dtype=bool) if p <= 0.0 else keep_mask(key[0], key[1], n, p)


# ---- positional encoding -------------------------------------------------------------------------------------------------------------
def posenc_ref(gl, cent, w1, b1, w2, b2, dt=np.float64):
    """tok = gl + fc2(leaky_relu(fc1(cent))); hid [Q, 16], slope [Q, 16] (1 or 0.01), `sure`: where the sign of fc1's output is decided."""
    gl, cent, w1, b1, w2, b2 = (np.asarray(x, dtype=dt) for x in (gl, cent, w1, b1, w2, b2))
    v = cent @ w1.T + b1
    vm = np.abs(f64(cent)) @ np.abs(f64(w1)).T + np.abs(f64(b1))
    bv = bar(vm, f64(v), 2)
    pos = v > 0
    hid = np.where(pos, v, dt(LEAK) * v)
    bh = np.where(pos, 1.0, LEAK) * bv + EPS * np.abs(f64(hid))
    tok = gl + (hid @ w2.T + b2)
    tm = np.abs(f64(hid)) @ np.abs(f64(w2)).T + np.abs(f64(b2)) + np.abs(f64(gl))
    bt = bar(tm, f64(tok), 16) + bh @ np.abs(f64(w2)).T
    return {"tok": (tok, bt), "hid": (hid, bh), "slope": (np.where(pos, 1.0, LEAK), np.zeros_like(bv)), "sure": np.abs(f64(v)) > bv}


# ---- attention --------------------------------------------------------------------------------------------------------------------------
def _split(qkv, B, W, dt):
    x = np.asarray(qkv, dtype=dt).reshape(B, W, 3, HEADS, D)
    return x[:, :, 0].transpose(0, 2, 1, 3), x[:, :, 1].transpose(0, 2, 1, 3), x[:, :, 2].transpose(0, 2, 1, 3)     # [B, 8, W, 32] each


def attention_ref(qkv, mask, B, W, drop_p=0.0, key=None, dt=np.float64):
    """probs [B, 8, W, W] (post-softmax, pre-dropout; a row whose keys are all masked is zeros) and ctx [B * W, 256]."""
    q, k, v = _split(qkv, B, W, dt)
    q = q * dt(QSCALE)
    s = np.einsum("bhid,bhjd->bhij", q, k)
    sm = np.einsum("bhid,bhjd->bhij", np.abs(f64(q)), np.abs(f64(k)))
    bs = bar(sm, f64(s), D) + EPS * sm                               # + the rounding of q * qscale
    if mask is not None:
        mk = np.asarray(mask).astype(bool).reshape(B, 1, 1, W)
        s = np.where(mk, -np.inf, s)
        bs = np.where(mk, 0.0, bs)
    m = s.max(-1, keepdims=True)
    dead = ~np.isfinite(m)
    with np.errstate(invalid="ignore"):
        x = np.where(dead | ~np.isfinite(s), -np.inf, s - np.where(dead, 0.0, m))
    e = np.exp(x)                                                   # exp(-inf) = 0: masked keys, fully masked rows
    tot = e.sum(-1, keepdims=True)
    p = np.where(tot > 0, e / np.where(tot > 0, tot, 1), 0).astype(dt)
    p64 = f64(p)
    re = np.where(p64 > 0, bs + bs.max(-1, keepdims=True) + exp_rel(np.where(np.isfinite(x), x, 0.0), FAST_EXP_ULP), 0.0)
    bp = p64 * (re + (p64 * re).sum(-1, keepdims=True) + (W + 3) * EPS) + np.where(p64 > 0, TINY, 0.0)
    keep = keep_flat(key, B * HEADS * W * W, drop_p).reshape(B, HEADS, W, W)
    ds = PP.dscale32(drop_p) if drop_p > 0 else 1.0
    pd = np.where(keep, p * dt(ds), 0).astype(dt)
    bpd = np.where(keep, bp * ds, 0.0) + EPS * np.abs(f64(pd))
    ctx = np.einsum("bhij,bhjd->bhid", pd, v)
    cm = np.einsum("bhij,bhjd->bhid", np.abs(f64(pd)), np.abs(f64(v)))
    bc = bar(cm, f64(ctx), W) + np.einsum("bhij,bhjd->bhid", bpd, np.abs(f64(v)))
    flat = lambda t: t.transpose(0, 2, 1, 3).reshape(B * W, E)
    return {"probs": (p, bp), "ctx": (flat(ctx), flat(bc))}


def attention_bwd_ref(qkv, probs, dctx, B, W, drop_p=0.0, key=None, dt=np.float64):
    """dqkv [B * W, 768]: the gradients of softmax(q k^T / sqrt(d)) [dropout] v wrt q, k, v given the saved probs and d(ctx)."""
    q, k, v = _split(qkv, B, W, dt)
    q = q * dt(QSCALE)
    p = np.asarray(probs, dtype=dt).reshape(B, HEADS, W, W)
    dc = np.asarray(dctx, dtype=dt).reshape(B, W, HEADS, D).transpose(0, 2, 1, 3)
    A = lambda t: np.abs(f64(t))
    keep = keep_flat(key, B * HEADS * W * W, drop_p).reshape(B, HEADS, W, W)
    ds = PP.dscale32(drop_p) if drop_p > 0 else 1.0
    kf = np.where(keep, dt(ds), dt(0))
    pd = p * kf
    dv = np.einsum("bhij,bhid->bhjd", pd, dc)
    dvm = np.einsum("bhij,bhid->bhjd", A(pd), A(dc))
    bdv = bar(dvm, f64(dv), W) + EPS * dvm
    dP = np.einsum("bhid,bhjd->bhij", dc, v) * kf
    dPm = np.einsum("bhid,bhjd->bhij", A(dc), A(v)) * f64(kf)
    bdP = bar(dPm, f64(dP), D) + EPS * A(dP)
    dot = (dP * p).sum(-1, keepdims=True)
    dotm = (A(dP) * A(p)).sum(-1, keepdims=True)
    bdot = bar(dotm, f64(dot), W) + (bdP * A(p)).sum(-1, keepdims=True)
    dS = p * (dP - dot)
    bdS = A(p) * (bdP + bdot) + 2 * EPS * A(p) * (A(dP) + A(dot))
    dq = np.einsum("bhij,bhjd->bhid", dS, k) * dt(QSCALE)
    dqm = np.einsum("bhij,bhjd->bhid", A(dS), A(k)) * QSCALE
    bdq = bar(dqm, f64(dq), W) + QSCALE * np.einsum("bhij,bhjd->bhid", bdS, A(k)) + EPS * A(dq)
    dk = np.einsum("bhji,bhjd->bhid", dS, q)
    dkm = np.einsum("bhji,bhjd->bhid", A(dS), A(q))
    bdk = bar(dkm, f64(dk), W) + np.einsum("bhji,bhjd->bhid", bdS, A(q)) + EPS * dkm
    pack = lambda a, b, c: np.stack([a, b, c], axis=2).transpose(0, 3, 2, 1, 4).reshape(B * W, 3 * E)     # [B, 8, 3, W, 32] -> [B, W, 3, 8, 32]
    return {"dqkv": (pack(dq, dk, dv), pack(bdq, bdk, bdv))}


# ---- logits tail + weighted cross-entropy ------------------------------------------------------------------------------------------------
def live_targets(targets, C):
    t = np.asarray(targets).reshape(-1)
    return (t >= 0) & (t < C)


def logits_ref(z4, R, P, C, targets=None, class_w=None, dt=np.float64):
    """logits [R / P, C, P] (an exact transpose), preds [R] (first maximum), per-workgroup partials [blocks, 2] = (sum w nll, sum w) of
    HL_ROWS rows each, loss2 = (ce, sum w).  A target outside [0, C) is ignored, like -1."""
    z = np.asarray(z4, dtype=dt)[:R, :C]
    out = {"logits": z.reshape(R // P, P, C).transpose(0, 2, 1), "preds": np.argmax(z, axis=1)}      # numpy's argmax: the first maximum
    if targets is None:
        return out
    t = np.asarray(targets).reshape(-1)[:R]
    live = live_targets(t, C)
    tc = np.where(live, t, 0)
    w = np.where(live, np.ones(C, dtype=dt)[tc] if class_w is None else np.asarray(class_w, dtype=dt)[tc], 0).astype(dt)
    m = z.max(1)
    x = z - m[:, None]
    se = np.exp(x).sum(1)
    lse = np.log(se)
    lt = z[np.arange(R), tc]
    nll = np.where(live, w * ((m + lse) - lt), 0).astype(dt)
    e64 = np.exp(f64(x))
    rse = (e64 * exp_rel(f64(x))).sum(1) / e64.sum(1) + C * EPS
    bl = rse + exp_rel(f64(se)) * np.abs(f64(lse))
    A = lambda a: np.abs(f64(a))
    bn = np.where(live, A(w) * (bl + EPS * (A(m) + A(lse)) + EPS * (A(m + lse) + A(lt))) + EPS * A(nll), 0.0)
    nb = -(-R // HL_ROWS)
    pad = nb * HL_ROWS - R
    blk = lambda a: np.concatenate([f64(a), np.zeros(pad)]).reshape(nb, HL_ROWS)
    part = np.stack([blk(nll).sum(1), blk(w).sum(1)], axis=1)
    # 256 values: a 6-level shuffle tree and a 4-term sum, <= 10 roundings of partial sums of magnitude <= sum |.|
    bpart = np.stack([blk(bn).sum(1) + 10 * EPS * blk(A(nll)).sum(1), 10 * EPS * blk(A(w)).sum(1)], axis=1)
    num, den = part[:, 0].sum(), part[:, 1].sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        ce = num / den
        bce = bpart[:, 0].sum() / den + abs(ce) * bpart[:, 1].sum() / den + EPS * abs(ce)     # double-precision finalize, one cast
    out.update(loss_part=(part, bpart), loss2=(np.array([ce, den]), np.array([bce, bpart[:, 1].sum() + EPS * den])), wnll=nll, w=w)
    return out


def ce_bwd_ref(logits, targets, class_w, wsum, gscale, dt=np.float64):
    """dlogits [B, C, P] = gscale w[t] / wsum (softmax(logits[b, :, p]) - onehot(t)); 0 where the target is not in [0, C)."""
    lg = np.asarray(logits, dtype=dt)
    B, C, P = lg.shape
    z = lg.transpose(0, 2, 1).reshape(B * P, C)
    t = np.asarray(targets).reshape(-1)
    live = live_targets(t, C)
    tc = np.where(live, t, 0)
    w = np.where(live, np.ones(C, dtype=dt)[tc] if class_w is None else np.asarray(class_w, dtype=dt)[tc], 0).astype(dt)
    x = z - z.max(1, keepdims=True)
    e = np.exp(x)
    p = e / e.sum(1, keepdims=True)
    oh = (np.arange(C)[None, :] == tc[:, None]).astype(dt)
    kk = (dt(gscale) * w / dt(wsum))[:, None]
    d = np.where(live[:, None], kk * (p - oh), 0).astype(dt)
    p64, re = f64(p), exp_rel(f64(x))
    bp = p64 * (re + (p64 * re).sum(1, keepdims=True) + (C + 3) * EPS) + TINY
    bd = np.abs(f64(kk)) * (bp + 5 * EPS * np.abs(p64 - f64(oh)))            # k: two roundings; p - onehot, the product: three more
    rs = lambda a: a.reshape(B, P, C).transpose(0, 2, 1)
    return {"dlogits": (rs(d), rs(np.where(live[:, None], bd, 0.0)))}


# ---- conv_4 backward + dropout + bn_3 / ReLU mask ---------------------------------------------------------------------------------------
def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def head_out_bwd_ref(dlogits, z3, scale, shift, mean, invstd, w4, P, drop_p=0.0, key=None, dt=np.float64):
    """dy3 [R, 64], dW4 [C, 64], db4 [C], part_a / part_b [64] (sums over ALL rows: the test sums the per-workgroup partials).
    z3 is what the kernel reads (already bf16-rounded in the bf16 mode).  `sure` [R, 64]: where the ReLU decision is outside its bar."""
    dl = np.asarray(dlogits, dtype=dt)
    Bn, C, _ = dl.shape
    R = Bn * P
    d = dl.transpose(0, 2, 1).reshape(R, C)
    z, sc, sh, me, iv, w = (np.asarray(x, dtype=dt) for x in (z3, scale, shift, mean, invstd, w4))
    A = lambda a: np.abs(f64(a))
    pre = z * sc + sh
    bpre = 2 * EPS * (A(z * sc) + A(sh))
    sure = A(pre) > bpre
    keep = keep_flat(key, R * 64, drop_p).reshape(R, 64)
    ds = PP.dscale32(drop_p) if drop_p > 0 else 1.0
    av = np.where(keep, np.maximum(pre, 0) * dt(ds), 0).astype(dt)
    bav = np.where(keep, (bpre + EPS * A(av)) * ds, 0.0)
    da = (d @ w) * dt(ds)
    dam = (A(d) @ A(w)) * ds
    bda = bar(dam, f64(da), C) + EPS * A(da)
    mask = av > 0
    dy = np.where(mask, da, 0).astype(dt)
    unsure = keep & ~sure
    zh = (z - me) * iv
    bzh = 2 * EPS * A(zh)
    dW = d.T @ av
    bdW = bar(A(d).T @ A(av), f64(dW), R) + A(d).T @ bav
    db = d.sum(0)
    bdb = bar(A(d).sum(0), f64(db), R)
    m64 = np.where(mask, dam, 0.0)
    pa = dy.sum(0)
    bpa = bar(m64.sum(0), f64(pa), R) + np.where(mask, bda, 0.0).sum(0) + np.where(unsure, A(da), 0.0).sum(0)
    pb = (dy * zh).sum(0)
    bpb = bar((m64 * A(zh)).sum(0), f64(pb), R) + np.where(mask, bda * A(zh) + A(da) * bzh, 0.0).sum(0) + np.where(unsure, A(da * zh), 0.0).sum(0)
    return {"dy3": (dy, np.where(mask, bda, 0.0)), "da3": (da, bda), "dW4": (dW, bdW), "db4": (db, bdb), "part_a": (pa, bpa), "part_b": (pb, bpb),
            "sure": sure | ~keep}


# ---- linear backward ------------------------------------------------------------------------------------------------------------------
def linear_bwd_ref(G, X, W=None, dx_mul=None, dt=np.float64):
    """dW = G^T X, db = column sums of G, dX = G W (times dx_mul) for G [rows, n_out], X [rows, n_in], W [n_out, n_in]."""
    G, X = np.asarray(G, dtype=dt), np.asarray(X, dtype=dt)
    A = lambda a: np.abs(f64(a))
    rows = G.shape[0]
    dW = G.T @ X
    out = {"dW": (dW, bar(A(G).T @ A(X), f64(dW), rows)), "db": (G.sum(0), bar(A(G).sum(0), f64(G.sum(0)), rows))}
    if W is not None:
        W = np.asarray(W, dtype=dt)
        dX = G @ W
        m = A(G) @ A(W)
        if dx_mul is not None:
            mul = np.asarray(dx_mul, dtype=dt)
            dX, m = dX * mul, m * A(mul)
        out["dX"] = (dX, bar(m, f64(dX), G.shape[1]) + (EPS * A(dX) if dx_mul is not None else 0.0))
    return out


# ---- orthogonality regulariser ------------------------------------------------------------------------------------------------------
def reg_fwd_ref(F, dt=np.float64):
    """G = I - F F^T per matrix [n, 64, 64], part [n] = sum G^2, reg = sqrt(sum part)."""
    F = np.asarray(F, dtype=dt).reshape(-1, 64, 64)
    A = lambda a: np.abs(f64(a))
    eye = np.eye(64, dtype=dt)
    G = eye - F @ F.transpose(0, 2, 1)
    bG = bar(A(F) @ A(F).transpose(0, 2, 1) + np.eye(64), f64(G), 64)
    part = (G * G).sum((1, 2))
    bpart = bar((f64(G) ** 2).sum((1, 2)), f64(part), 4096) + (2 * A(G) * bG).sum((1, 2))
    s = float(f64(part).sum())
    reg = math.sqrt(s)
    breg = (bpart.sum() / (2 * reg) if reg > 0 else math.sqrt(bpart.sum())) + EPS * reg       # the finalize sums in double
    return {"G": (G, bG), "part": (part, bpart), "reg": (np.array([reg]).astype(dt), np.array([breg]))}


def reg_bwd_ref(F, G, reg, coef, dF0=None, dt=np.float64):
    """dF0 + coef d(reg)/dF, d(reg)/dF = -2 G F / reg (0 where reg == 0), from the fp32 G and reg the forward kept."""
    F, G = np.asarray(F, dtype=dt).reshape(-1, 64, 64), np.asarray(G, dtype=dt).reshape(-1, 64, 64)
    A = lambda a: np.abs(f64(a))
    r = dt(reg)
    kk = dt(-2.0) * dt(coef) / r if r > 0 else dt(0)
    d = G @ F
    out = kk * d
    b = abs(float(kk)) * bar(A(G) @ A(F), f64(d), 64) + 4 * EPS * A(out)
    if dF0 is not None:
        out = np.asarray(dF0, dtype=dt).reshape(-1, 64, 64) + out
        b = b + EPS * A(out)
    return {"dF": (out, b)}


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, step, lr, b1, b2, eps, gscale=1.0):
    """One step of adam_kernel in float64 on the fp32 state and the fp32 hyper-parameters (the C ABI takes lr, betas and eps as floats;
    the host forms 1 - beta^t in double): (p, m, v) and their bars.

    adam_kernel per element: gi = g gs (exact for gs a power of two); mi = b1 m + (1 - b1) gi: 1 - b1 is exact (b1 in [0.5, 1]), two products
    and one sum = 3 roundings, each relative to a term of |b1 m| + |(1 - b1) gi|; vi likewise ((1 - b2) gi gi: two products, b2 v one, the
    sum one, <= 3 on any term).  Bar 4 eps of those magnitudes.
    delta = step_size mi / (sqrt(vi) isb + eps): mi 3 eps (relative to |mi| when m and g agree in sign: the cases use such states, since with
    cancellation in mi no bound relative to |delta| exists), vi 3 eps -> sqrt 1.5 + 1, the product with isb 1, the sum 1: denominator <= 4.5;
    step_size and isb are rounded from double on the host: 1 each; the product and the quotient: 2.  3 + 4.5 + 2 + 2 = 11.5 <= 16.
    p - delta: one rounding of the result, <= eps (|p| + |delta|) <= 2 eps |p| + eps |delta| (inside the 16)."""
    lr, b1, b2, eps, gscale = (float(np.float32(x)) for x in (lr, b1, b2, eps, gscale))
    p, g, m, v = (f64(x) for x in (p, g, m, v))
    gi = g * gscale
    mi = b1 * m + (1 - b1) * gi
    vi = b2 * v + (1 - b2) * gi * gi
    bm = 4 * EPS * (np.abs(b1 * m) + np.abs((1 - b1) * gi))
    bv = 4 * EPS * (np.abs(b2 * v) + np.abs((1 - b2) * gi * gi))
    delta = (lr / (1 - b1 ** step)) * mi / (np.sqrt(vi) / math.sqrt(1 - b2 ** step) + eps)
    pn = p - delta
    return {"p": (pn, 2 * EPS * np.abs(pn) + 16 * EPS * np.abs(delta)), "m": (mi, bm), "v": (vi, bv), "delta": delta}


def worst(x, ref):
    """worst |x - value| / bar of a (value, bar) pair; finite x required; an element with bar 0 must be exact."""
    want, b = ref
    x = f64(x)
    assert x.shape == np.shape(want), (x.shape, np.shape(want))
    assert np.all(np.isfinite(x)), "non-finite where the contract writes"
    err = np.abs(x - f64(want))
    b = np.broadcast_to(f64(b), err.shape)
    r = np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))
    return float(r.max()) if r.size else 0.0


# ================================================================================================================================
# the committed cases: inputs as numpy fp32, shared by the GPU tests and by tests/test_head_refs_cpu.py (which checks the exclusion caps)
# ================================================================================================================================
def rng(seed):
    return np.random.default_rng(seed)


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


ATT_W, ATT_B = (1, 2, 3, 9, 31, 32), (1, 5, 64)
ATT_VARIANTS = ("plain", "mask1", "maskall", "drop", "eval", "large")


def make_attention(W, B, variant, seed=0):
    """qkv [B * W, 768], dctx [B * W, 256], mask [B, W] uint8 or None, drop_p, key.  mask1: one key of every sample masked (none where
    W == 1: that is maskall); maskall: sample B // 2 has every key masked, the others one; large: |scores| up to ~30."""
    g = rng(1000 * W + 10 * B + seed)
    qkv = f32(g.standard_normal((B * W, 3 * E)))
    if variant == "large":
        qkv[:, :2 * E] *= 3.6                 # q k / sqrt(32) of std 3.6^2 = 13: the extreme scores reach |s| ~ 30 and beyond
    mask = None
    if variant in ("mask1", "maskall"):
        mask = np.zeros((B, W), dtype=np.uint8)
        if W > 1:
            mask[np.arange(B), g.integers(0, W, B)] = 1
        if variant == "maskall":
            mask[B // 2, :] = 1
    drop_p = 0.3 if variant == "drop" else 0.0
    return dict(qkv=qkv, dctx=f32(g.standard_normal((B * W, E))), mask=mask, drop_p=drop_p, key=(seed + 11, 0), B=B, W=W,
                want_probs=variant != "eval")


POSENC_Q = (1, 7, 576)


def make_posenc(Q, seed=0):
    """centroids on a dyadic grid, weights in eighths and biases in quarters: fc1's output is exact in fp32, so some hidden units are exactly
    0 (centroid row 0 is the origin and b1[0] = b1[5] = 0) and the sign of every other is decided exactly."""
    g = rng(77 + Q + seed)
    cent = f32(g.integers(-8, 9, (Q, 2)) / 4.0)
    cent[0] = 0.0
    w1 = f32(g.integers(-8, 9, (16, 2)) / 8.0)
    b1 = f32(g.integers(-4, 5, 16) / 4.0)
    b1[[0, 5]] = 0.0
    return dict(gl=f32(g.standard_normal((Q, E))), cent=cent, w1=w1, b1=b1, w2=f32(g.uniform(-1, 1, (E, 16)) / 4), b2=f32(g.uniform(-0.5, 0.5, E)), Q=Q)


LOGIT_C, LOGIT_P, LOGIT_B = (1, 2, 5, 8), (1, 255, 256, 257, 1000), (1, 3)


def make_logits(C, P, B, ldz4, class_w, seed=0):
    """z4 [R, ldz4] with NaN padding columns, targets over -1, valid and >= C, rows of equal logits (the first-maximum rule)."""
    g = rng(31 * C + 7 * P + B + ldz4 + seed)
    R = B * P
    z = np.full((R, ldz4), np.nan, dtype=np.float32)
    z[:, :C] = f32(g.standard_normal((R, C)) * 3)
    z[::5, :C] = z[::5, :1]                                        # every class equal: argmax 0
    if C > 2:
        z[1::7, C - 1] = z[1::7, 1] = np.abs(z[1::7, :C]).max(1) + 1     # two equal maxima: the lower class wins
    t = g.integers(-1, C + 2, R).astype(np.int64)                  # -1 ignored, C and C + 1 outside: ignored too
    t[R // 2] = 0                                                  # at least one live row
    w = f32([1.0, 2.0, 2.0, 1.0, 1.0, 0.5, 4.0, 1.0][:C]) if class_w else None
    return dict(z4=z, targets=t, class_w=w, R=R, P=P, C=C, B=B, ldz4=ldz4)


HOB_R, HOB_C = (1, 63, 64, 65, 1023, 1024, 1025, 6052), (1, 5, 8)


def make_head_out(R, C, drop_p, zb, seed=0):
    """z3 of unit scale against bn_3 constants of order 1 (some scales negative): |pre-activation| <= its bar ~ 1e-7 for about one element
    in 1e7, far below the 0.1 % cap.  R is one sample (P = R) except R = 6052 = 4 x 1513."""
    g = rng(13 * R + C + int(drop_p * 10) + 2 * zb + seed)
    P = 1513 if R == 6052 else R
    z3 = f32(g.standard_normal((R, 64)))
    zread = bf16_round(z3) if zb else z3
    mean, var = f32(g.uniform(-0.3, 0.3, 64)), f32(g.uniform(0.5, 2.0, 64))
    invstd = f32(1.0 / np.sqrt(var + 1e-5))
    gamma = f32(g.uniform(0.5, 1.5, 64) * np.where(np.arange(64) % 7 == 3, -1, 1))
    beta = f32(g.uniform(-0.5, 0.5, 64))
    scale = f32(gamma * invstd)
    shift = f32(beta - mean * scale)
    return dict(dlogits=f32(g.standard_normal((R // P, C, P)) / 64), z3=z3, zread=zread, scale=scale, shift=shift, mean=mean, invstd=invstd,
                w4=f32(g.uniform(-1, 1, (C, 64)) / 8), R=R, P=P, C=C, drop_p=drop_p, key=(seed + 5, 2), zb=zb)


LIN_ROWS, LIN_SHAPES = (3, 12, 576), ((128, 256), (256, 256), (768, 256), (256, 16), (16, 2))


def make_linear(rows, n_out, n_in, ldw, seed=0):
    g = rng(rows + 3 * n_out + n_in + ldw + seed)
    Wl = np.full((n_out, ldw), np.nan, dtype=np.float32)
    Wl[:, :n_in] = f32(g.uniform(-1, 1, (n_out, n_in)) / np.sqrt(n_in))
    return dict(G=f32(g.standard_normal((rows, n_out))), X=f32(g.standard_normal((rows, n_in))), Wl=Wl,
                dx_mul=f32(np.where(g.random((rows, n_in)) < 0.5, 1.0, 0.01)), rows=rows, n_out=n_out, n_in=n_in, ldw=ldw)


def make_reg(n, kind, seed=0):
    """kind 'mixed': near-orthogonal matrices, for n > 1 the last one exactly orthogonal (a signed permutation); 'zero': all exactly orthogonal, reg == 0."""
    g = rng(400 + n + seed)
    F = f32(np.eye(64)[None] + g.standard_normal((n, 64, 64)) * 0.05)
    perm = lambda: np.eye(64)[g.permutation(64)] * g.choice([-1.0, 1.0], 64)[:, None]
    if kind == "zero":
        F = f32(np.stack([perm() for _ in range(n)]))
    elif n > 1:
        F[-1] = perm()
    return F


ADAM_STEPS = (1, 2, 3, 10, 1000, 100000)
ADAM_SIZES = (0, 1, 255, 2048, 2049, 300001)
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def make_adam(n_tensors, seed=0, big_at=None):
    """lists of fp32 (p, g, m, v): sizes cycle through ADAM_SIZES without the largest, which appears once (at big_at, default the last tensor:
    it sizes the grid of its launch).  m carries the sign of g (see adam_ref); tensor 1 (if any) is the all-zero no-op case."""
    g = rng(900 + n_tensors + seed)
    big_at = n_tensors - 1 if big_at is None else big_at
    out = []
    for i in range(n_tensors):
        n = ADAM_SIZES[-1] if i == big_at else ADAM_SIZES[i % (len(ADAM_SIZES) - 1)]
        gr = f32(g.standard_normal(n) * 10.0 ** g.integers(-4, 1))
        m = f32(np.sign(gr) * np.abs(g.standard_normal(n)) * 0.1)
        v = f32(g.random(n) * 0.01)
        p = f32(g.standard_normal(n))
        if i == 1:
            gr, m, v = np.zeros_like(gr), np.zeros_like(m), np.zeros_like(v)
        out.append((p, gr, m, v))
    return out


PAD_W = (1, 2, 9, 32)


def pad_P(W):
    return (W, 1024 * W - W, 9 * 2048 // W * W if (9 * 2048) % W else 9 * 2048, (8192 + 9 * 7 + W - 1) // W * W)


def make_pad_targets(B, P, W, seed=0):
    """[B, P] int64: column 0 of sample 0 all -1; column W - 1 of sample 0 live only in its LAST element; the last sample all -1."""
    g = rng(50 + P + W + seed)
    t = g.integers(-1, 5, (B, P)).astype(np.int64)
    t[0, 0::W] = -1
    if W > 1:
        t[0, W - 1::W] = -1
        t[0, P - 1] = 3
    t[B - 1] = -1
    return t


def pad_mask_ref(t, W):
    B = t.shape[0]
    return (torch.from_numpy(t).view(B, -1, W) == -1).all(1).numpy().astype(np.uint8)
