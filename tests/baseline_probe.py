"""Layer-local float64 oracle of the baseline single-window PointNet's kernels: csrc/baseline_train.hip (bt_bias, bt_stats, bt_running_stats,
bt_bn_act, bt_bn_bwd_sums, bt_bn_bwd_apply, bt_rowmax, bt_pool_scatter, bt_mix, bt_mix_bwd, bt_segsum, bt_logits both ways, bt_fill, bt_add,
bt_dropout, bt_log_softmax, bt_log_softmax_bwd and the composed fwd_layer / bwd_layer) and csrc/baseline.hip (bl_fold, bl_affine, bl_rowmax,
bl_mix, bl_logits).

The C side is ampnet_probe_baseline_f32 (include/ampnet_hip.h, "test hooks"; csrc/layer_probe.hip): ONE launch of one of them, selected by
`op`, through the launch wrappers of csrc/baseline.h that the product entry points call, on buffers the test chose, every extent checked on
the host first.  This module holds the ctypes mirror of AmpnetBaselineProbe and a float64 restatement of each operation, written from the
reference model (pointNet/model/pointnet.py: nn.BatchNorm1d in train and eval mode, nn.MaxPool1d, torch.bmm on x[:, :, :k], F.log_softmax,
nn.Dropout) on the fp32 inputs.  Every restatement returns {output name: (float64 value, bar)}; `dt=np.float32` evaluates the same formulas in
fp32 numpy for tests/test_baseline_refs_cpu.py, which also holds the restatements to torch in float64.  Host side only; the GPU tests are
tests/test_baseline_layers_gpu.py.

Bars (eps = 2^-24; pw_probe.bar(mag, x, K) = 8 eps sqrt(K) mag + 2 eps |x|; no constant here was fitted to a kernel's output)
  bt_bias, bt_add       at most two fp32 additions: bar(|z| + |bias| + |add|, x, 1); with ONE operand present the result is one rounding: bitwise
  bt_stats              the kernel sums in double (K = 1): what remains is the rounding of the outputs.  mean: bar(mean |z|, mu, 1); the variance
                        is a sum of squares, every term positive: bar(var, var, 1), carried through invstd = (var + eps)^-1/2 as
                        invstd / (2 (var + eps)) bar(var) + 3 eps invstd (the addition, the root, the reciprocal).  So a column with
                        mean^2 >> variance is held to its VARIANCE (a one-pass E z^2 - mu^2 in fp32 misses it), and a constant column
                        gives invstd = 1 / sqrt(eps) at 3 eps.  Running update
                        (1 - m) r + m s in fp32: bar(|(1 - m) r| + |m s|, new, 1) + m bar(s), s the mean or the UNBIASED variance
  bt_running_stats, bl_fold   1 / sqrtf(rv + eps): bar(|inv|, inv, 1); scale = g / sqrtf(..): bar(|s|, s, 1); shift = fma(b - rm, s, be):
                        bar(|b - rm| |s| + |be|, shift, 1) + |b - rm| bar(s)
  bt_bn_act, bl_affine  one subtraction, one product, one fma (one addition, one fma): bar(|zh g| + |be|, pre, 1) (bar(|v s| + |t|, y, 1)).
                        ReLU decisions: an element is compared only where |pre-activation| > its bar; elsewhere it must be 0 or within the bar
                        of the unmasked value; at most 1 % of a case may be undecided (asserted per case on the reference alone in
                        tests/test_baseline_refs_cpu.py)
  bt_bn_bwd_sums        double sums (K = 1) of g = da (a > 0) and of g zh with zh = (z - mean) invstd in fp32 (two roundings, inside the 8 eps):
                        dbe bar(sum |g|, dbe, 1), dg bar(sum |g zh|, dg, 1).  The mask reads the INPUT a: exact, no decision rule
  bt_bn_bwd_apply       dz = gamma invstd (g - dbe / M - zh dg / M): |gamma invstd| bar(|g| + |dbe| / M + |zh dg| / M, inner, 1) + 2 eps |dz|
  bt_mix, bl_mix        k fmas: bar(sum |x| |T|, out, k); columns k .. 8 are copies
  bt_mix_bwd, bt_segsum double sums of exact products: K = 1
  bt_log_softmax        head_probe's exp / log model (EXP_ULP = 4, measured there for expf and logf on the device at 0.24 and 0.48 of it, under the
                        0.5 the issue of a new constant would need: none is new here): se = sum_c exp(z - m) has the relative error
                        rse = sum e rel(z - m) / se + C eps; log: rse + rel(se) |log se|; then m + log se and z - lse, one rounding each:
                        eps (|m| + |log se| + |lse| + |z| + |out|)
  bt_log_softmax_bwd    p = exp(z - m) / se as in head_probe.ce_bwd_ref: p (rel + sum p rel + (C + 3) eps) + 2^-126; tot = sum_c d_out in fp32:
                        bar(sum |d|, tot, C); dz = d - p tot: |tot| bar(p) + p bar(tot) + 2 eps |p tot| + eps (|d| + |dz|)
  exact                 bt_rowmax / bl_rowmax values and bt_rowmax's arg (np.argmax: the first maximum), bt_pool_scatter, bt_logits both ways,
                        bl_logits, bt_fill, bt_dropout (the oracle's keep_mask; a kept value is the fp32 product a * (1 / (1 - p)))
"""
import ctypes

import numpy as np
import torch

import pw_probe as PP
from pw_probe import EPS32, L, bar, keep_mask
from head_probe import TINY, exp_rel                 # exp_rel carries EXP_ULP = 4

EPS = EPS32
BN_EPS = float(np.float32(1e-5))                     # the fp32 constants the kernels get
MOMENTUM = float(np.float32(0.1))
AMPNET_E_ARG = PP.AMPNET_E_ARG
OPS = {"bt_bias": 0, "bt_stats": 1, "bt_running_stats": 2, "bt_bn_act": 3, "bt_bn_bwd_sums": 4, "bt_bn_bwd_apply": 5, "bt_rowmax": 6, "bl_rowmax": 7,
       "bt_pool_scatter": 8, "bt_mix": 9, "bl_mix": 10, "bt_mix_bwd": 11, "bt_segsum": 12, "bt_logits": 13, "bt_logits_to_rows": 14, "bl_logits": 15,
       "bt_fill": 16, "bt_add": 17, "bt_dropout": 18, "bt_log_softmax": 19, "bt_log_softmax_bwd": 20, "bl_fold": 21, "bl_affine": 22,
       "fwd_layer": 23, "bwd_layer": 24}
KERNEL = {v: k + "_kernel" for k, v in OPS.items()}
KERNEL[14] = "bt_logits_kernel"
COMPOSED = (23, 24)                                  # several launches, no name of their own

_p, _i64, _i32, _u32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_float
INTS = ("op", "B", "N", "M", "C", "K", "k", "per", "relu", "train", "accumulate", "lda", "ldw", "w0", "ld_dA", "pad0")
POINTERS = ("z", "a", "da", "mean", "invstd", "gamma", "beta", "rm", "rv", "bias", "add", "dg", "dbe", "out", "arg", "x", "T", "W", "dW", "db",
            "dA", "A", "scale", "shift")


class BaselineProbe(ctypes.Structure):
    _fields_ = [(n, _i32) for n in INTS] + [(n, _f32) for n in ("eps", "momentum", "value", "drop_p")] + [("drop_seed", _u32), ("pad1", _u32), ("n", _i64)] + \
               [x for n in POINTERS for x in ((n, _p), (n + "_n", _i64))]


EXTENTS = {n: n + "_n" for n in POINTERS}


def set_tensors(desc, **tensors):
    """also keeps the tensors alive as long as the descriptor: it holds raw pointers, and a freed block is handed to the next allocation"""
    PP.set_tensors(desc, EXTENTS, **tensors)
    desc.__dict__.setdefault("_keep", {}).update(tensors)


def new(op, **ints):
    d = BaselineProbe()
    d.op = OPS[op]
    d.eps, d.momentum = BN_EPS, MOMENTUM
    for k, v in ints.items():
        setattr(d, k, v)
    return d


def run(desc):
    """(return code, kernel names recorded) of one ampnet_probe_baseline_f32 call, synchronised."""
    lib = L.lib()
    lib.ampnet_probe_baseline_f32.argtypes = [ctypes.POINTER(BaselineProbe), ctypes.c_void_p]
    lib.ampnet_profile_enable(1)
    try:
        rc = lib.ampnet_probe_baseline_f32(ctypes.byref(desc), L.stream_ptr())
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


def _rows(per, M):
    return np.arange(M) // max(per, 1)


# ---- elementwise -------------------------------------------------------------------------------------------------------------------------
def bias_ref(z, bias, add, per, dt=np.float64):
    """z[row, c] + bias[c] + add[row // per, c], either addend optional."""
    z = np.asarray(z, dtype=dt)
    v, mag = z, A(z)
    if bias is not None:
        v, mag = (v + np.asarray(bias, dtype=dt)[None, :]).astype(dt), mag + A(bias)[None, :]
    if add is not None:
        ad = np.asarray(add, dtype=dt)[_rows(per, z.shape[0])]
        v, mag = (v + ad).astype(dt), mag + A(ad)
    return {"z": (v, bar(mag, f64(v), 1))}


def add_ref(y, x, dt=np.float64):
    v = (np.asarray(y, dtype=dt) + np.asarray(x, dtype=dt)).astype(dt)
    return {"z": (v, bar(A(y) + A(x), f64(v), 1))}


def stats_ref(z, rm, rv, eps=BN_EPS, momentum=MOMENTUM, dt=np.float64):
    """nn.BatchNorm1d in train mode over the M rows of z [M, C]: mean, invstd of the biased variance, and the running update with the unbiased
    variance (M == 1: with the sum of squares itself, 0)."""
    z64 = f64(z)
    M = z64.shape[0]
    m64 = z64.mean(0)                                                                 # the contract: sums over the rows in double,
    q64 = ((z64 - m64) ** 2).sum(0)                                                   # whatever dt evaluates the rest
    m, var = m64.astype(dt), (q64 / M).astype(dt)
    uv = (q64 / (M - 1)).astype(dt) if M > 1 else q64.astype(dt)
    bm = bar(A(z).mean(0), m64, 1)
    bvar = bar(f64(var), f64(var), 1)
    inv = (dt(1) / np.sqrt(var + dt(eps))).astype(dt)
    inv64 = f64(inv)
    binv = inv64 / (2.0 * (f64(var) + eps)) * bvar + 3 * EPS * inv64
    res = {"mean": (m, bm), "invstd": (inv, binv)}
    m9, m1 = dt(np.float32(1.0) - np.float32(momentum)), dt(np.float32(momentum))
    for name, r0, stat, bst in (("rm", rm, m, bm), ("rv", rv, uv, bar(A(uv), f64(uv), 1))):
        r0 = np.asarray(r0, dtype=dt)
        new_ = (m9 * r0 + m1 * stat).astype(dt)
        res[name] = (new_, bar(A(f64(m9) * f64(r0)) + A(f64(m1) * f64(stat)), f64(new_), 1) + float(m1) * bst)
    return res


def running_stats_ref(rm, rv, eps=BN_EPS, dt=np.float64):
    rv = np.asarray(rv, dtype=dt)
    inv = (dt(1) / np.sqrt(rv + dt(eps))).astype(dt)
    return {"mean": (np.asarray(rm, dtype=dt), np.zeros(len(rv))), "invstd": (inv, bar(A(inv), f64(inv), 1))}


def bn_act_ref(z, mean, invstd, gamma, beta, dt=np.float64):
    """pre = (z - mean) invstd gamma + beta, a = relu(pre); `sure` where the ReLU is decided."""
    z, mean, invstd, gamma, beta = (np.asarray(t, dtype=dt) for t in (z, mean, invstd, gamma, beta))
    zh = ((z - mean[None, :]) * invstd[None, :]).astype(dt)
    pre = (zh * gamma[None, :] + beta[None, :]).astype(dt)
    b = bar(A(zh) * A(gamma)[None, :] + A(beta)[None, :], f64(pre), 1)
    return {"pre": (pre, b), "sure": A(pre) > b, "a": (np.maximum(pre, dt(0)), b)}


def bn_bwd_sums_ref(da, a, z, mean, invstd, dt=np.float64):
    da, z, mean, invstd = (np.asarray(t, dtype=dt) for t in (da, z, mean, invstd))
    g = np.where(np.asarray(a) > 0, da, dt(0))
    zh = ((z - mean[None, :]) * invstd[None, :]).astype(dt)
    dbe, dg = f64(g).sum(0), (f64(g) * f64(zh)).sum(0)                                  # the contract: double sums
    return {"dbe": (dbe.astype(dt), bar(A(g).sum(0), dbe, 1)), "dg": (dg.astype(dt), bar((A(g) * A(zh)).sum(0), dg, 1))}


def bn_bwd_apply_ref(da, a, z, mean, invstd, gamma, dg, dbe, dt=np.float64):
    da, z, mean, invstd, gamma, dg, dbe = (np.asarray(t, dtype=dt) for t in (da, z, mean, invstd, gamma, dg, dbe))
    M = dt(z.shape[0])
    g = np.where(np.asarray(a) > 0, da, dt(0))
    zh = ((z - mean[None, :]) * invstd[None, :]).astype(dt)
    inner = (g - dbe[None, :] / M - zh * dg[None, :] / M).astype(dt)
    gi = (gamma * invstd).astype(dt)
    dz = (gi[None, :] * inner).astype(dt)
    mag = A(g) + A(dbe)[None, :] / float(M) + A(zh) * A(dg)[None, :] / float(M)
    return {"dz": (dz, A(gi)[None, :] * bar(mag, f64(inner), 1) + 2 * EPS * A(dz))}


def fold_ref(bias, gamma, beta, rm, rv, C, eps=BN_EPS, dt=np.float64):
    """scale / shift of y = (z + b - rm) g / sqrt(rv + eps) + be; without BatchNorm scale = 1, shift = b; without bias b = 0."""
    b = np.zeros(C, dtype=dt) if bias is None else np.asarray(bias, dtype=dt)
    if gamma is None:
        return {"scale": (np.ones(C, dtype=dt), np.zeros(C)), "shift": (b, np.zeros(C))}
    gamma, beta, rm, rv = (np.asarray(t, dtype=dt) for t in (gamma, beta, rm, rv))
    s = (gamma / np.sqrt(rv + dt(eps))).astype(dt)
    bs = bar(A(s), f64(s), 1)
    d = (b - rm).astype(dt)
    sh = (d * s + beta).astype(dt)
    return {"scale": (s, bs), "shift": (sh, bar(A(d) * A(s) + A(beta), f64(sh), 1) + A(d) * bs)}


def affine_ref(z, scale, shift, add, per, dt=np.float64):
    z, scale, shift = (np.asarray(t, dtype=dt) for t in (z, scale, shift))
    v = z if add is None else (z + np.asarray(add, dtype=dt)[_rows(per, z.shape[0])]).astype(dt)
    pre = (v * scale[None, :] + shift[None, :]).astype(dt)
    b = bar(A(v) * A(scale)[None, :] + A(shift)[None, :], f64(pre), 1) + (EPS * A(v) * A(scale)[None, :] if add is not None else 0.0)
    return {"pre": (pre, b), "sure": A(pre) > b}


# ---- pooling, transposes, the mix ---------------------------------------------------------------------------------------------------------
def rowmax_ref(a, B, N, C):
    a = np.asarray(a).reshape(B, N, C)
    return {"out": a.max(1), "arg": a.argmax(1).astype(np.int32)}


def pool_scatter_ref(d_pool, arg, B, N, C):
    out = np.zeros((B, N, C), dtype=np.float32)
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    out[bi, np.asarray(arg).reshape(B, C), ci] = np.asarray(d_pool).reshape(B, C)
    return out


def mix_ref(x, T, N, k, dt=np.float64):
    """cat([x[:, :k] @ T[row // N], x[:, k:]], 1) on rows x [R, 9]."""
    x = np.asarray(x, dtype=dt)
    R = x.shape[0]
    t = np.asarray(T, dtype=dt).reshape(-1, k, k)[np.arange(R) // N]
    head = np.einsum("ri,rij->rj", x[:, :k], t).astype(dt)
    mag = np.einsum("ri,rij->rj", A(x[:, :k]), A(t))
    return {"head": (head, bar(mag, f64(head), k)), "tail": x[:, k:]}


def mix_bwd_ref(x, d_xin, B, N, k, dt=np.float64):
    """dT[b, i, j] = sum over the rows of window b of x[row, i] d_xin[row, j]; the kernel sums in double."""
    x, d = f64(x).reshape(B, N, 9)[:, :, :k], f64(d_xin).reshape(B, N, 9)[:, :, :k]
    dT = np.einsum("bni,bnj->bij", x, d)
    return {"dT": (dT.astype(dt), bar(np.einsum("bni,bnj->bij", np.abs(x), np.abs(d)), dT, 1))}


def segsum_ref(dz, B, N, C, dt=np.float64):
    d = f64(dz).reshape(B, N, C)
    s = d.sum(1)
    return {"out": (s.astype(dt), bar(np.abs(d).sum(1), s, 1))}


def logits_ref(z, B, N, C):
    """z [B * N, C] -> logits [B, C, N], exact."""
    return np.ascontiguousarray(np.asarray(z).reshape(B, N, C).transpose(0, 2, 1))


def dropout_ref(a, seed, p):
    a = f32(a).reshape(-1)
    keep = keep_mask(seed, 0, a.size, p)
    return {"keep": keep, "out": np.where(keep, a * np.float32(PP.dscale32(p)), np.float32(0)).astype(np.float32)}


# ---- log_softmax -----------------------------------------------------------------------------------------------------------------------------
def log_softmax_ref(z, dt=np.float64):
    z = np.asarray(z, dtype=dt)
    C = z.shape[1]
    m = z.max(1, keepdims=True)
    x = (z - m).astype(dt)
    se = np.exp(x).sum(1, keepdims=True).astype(dt)
    ls = np.log(se).astype(dt)
    lse = (m + ls).astype(dt)
    out = (z - lse).astype(dt)
    e64 = np.exp(f64(x))
    rse = (e64 * exp_rel(f64(x))).sum(1, keepdims=True) / e64.sum(1, keepdims=True) + C * EPS
    bl = rse + exp_rel(f64(se)) * A(ls)
    return {"out": (out, bl + EPS * (A(m) + A(ls) + A(lse) + A(z) + A(out)))}


def log_softmax_bwd_ref(z, d_out, dt=np.float64):
    z, d = np.asarray(z, dtype=dt), np.asarray(d_out, dtype=dt)
    C = z.shape[1]
    x = (z - z.max(1, keepdims=True)).astype(dt)
    e = np.exp(x).astype(dt)
    p = (e / e.sum(1, keepdims=True)).astype(dt)
    tot = d.sum(1, keepdims=True).astype(dt)
    dz = (d - p * tot).astype(dt)
    p64, re = f64(p), exp_rel(f64(x))
    bp = p64 * (re + (p64 * re).sum(1, keepdims=True) + (C + 3) * EPS) + TINY
    btot = bar(A(d).sum(1, keepdims=True), f64(tot), C)
    return {"dz": (dz, A(tot) * bp + p64 * btot + 2 * EPS * A(p * tot) + EPS * (A(d) + A(dz)))}


# ================================================================================================================================
# the committed cases: inputs as numpy fp32, shared by the GPU tests and tests/test_baseline_refs_cpu.py
# ================================================================================================================================
def rng(seed):
    return np.random.default_rng(seed)


BIAS_CASES = [(M, C, per, kind) for (M, C, per) in ((7, 1, 1), (21, 5, 7), (9, 64, 9), (13, 100, 7), (3, 100, 1), (5, 64, 1))
              for kind in ("bias", "add", "both")]
STATS_M, STATS_C = (2, 3, 4, 5, 16, 513), (4, 64, 65, 130)
BWD_M, BWD_C = (2, 5, 513), (40, 64, 65)
POOL_N, POOL_C, POOL_B = (1, 2, 3, 4, 5, 7, 513), (1, 64, 65, 256), (1, 3)
SCATTER_BC = ((1, 1), (1, 255), (1, 256), (1, 257), (3, 65))
MIX_K, MIX_R = (2, 3), (1, 255, 256, 257)
MIX_BWD_N = (1, 255, 256, 257, 600)
SEG_N, SEG_C = (1, 3, 4, 5, 513), (1, 64, 65)
LOGITS_BNC = ((1, 1, 1), (2, 1, 5), (3, 7, 1), (2, 37, 9), (3, 100, 64))
FLAT_N = (1, 255, 256, 257)
DROP_P = (0.3, 0.5, 0.999)
LSM_B, LSM_C, LSM_SHIFT = (1, 63, 64, 65), (1, 2, 40, 64), (0.0, 80.0, -80.0)
FOLD_C = (4, 64, 65, 130)
LAYER_CASES = [dict(M=70, C=64, K=2, lda=9, ldw=2, w0=0, bn=1, bias=1, add=0, dA=0),
               dict(M=70, C=64, K=3, lda=9, ldw=3, w0=0, bn=1, bias=0, add=0, dA=0),
               dict(M=70, C=64, K=9, lda=9, ldw=9, w0=0, bn=1, bias=1, add=0, dA=1),
               dict(M=66, C=40, K=64, lda=64, ldw=64 + 24, w0=24, bn=1, bias=1, add=1, dA=1),      # conv_1 of the head on cat([global, local])
               dict(M=66, C=40, K=64, lda=64, ldw=64, w0=0, bn=1, bias=0, add=0, dA=2),             # dA accumulated
               dict(M=3, C=9, K=64, lda=64, ldw=64, w0=0, bn=0, bias=1, add=0, dA=1)]               # a T-Net's fc_3: no BatchNorm


def make_bias(M, C, per, kind, seed=0):
    g = rng(100 + 7 * M + C + per + seed)
    return dict(z=f32(g.standard_normal((M, C))), bias=f32(g.standard_normal(C)) if kind in ("bias", "both") else None,
                add=f32(g.standard_normal(((M - 1) // per + 1, C))) if kind in ("add", "both") else None)


def make_stats(M, C, seed=0):
    """z [M, C] with column 0 at mean^2 >> variance (1000 +- 1) and column 1 constant; running statistics away from (0, 1)."""
    g = rng(200 + 13 * M + C + seed)
    z = f32(g.standard_normal((M, C)) * g.uniform(0.5, 3.0, C) + g.uniform(-2.0, 2.0, C))
    z[:, 0] = f32(1000.0 + g.standard_normal(M))
    z[:, 1] = np.float32(2.5)
    return dict(z=z, rm=f32(g.uniform(-1.0, 1.0, C)), rv=f32(g.uniform(0.5, 2.0, C)), gamma=f32(g.uniform(0.5, 1.5, C) * g.choice([-1.0, 1.0], C)),
                beta=f32(g.uniform(-0.5, 0.5, C)))


def make_bn_bwd(M, C, seed=0):
    """A layer's tape (z, its statistics, a = relu(bn(z)) as fp32 would leave it) and an upstream gradient set on EVERY row, dead ones included."""
    c = make_stats(M, C, seed + 31)
    st = stats_ref(c["z"], c["rm"], c["rv"])
    mean, invstd = f32(st["mean"][0]), f32(st["invstd"][0])
    a = f32(np.maximum(bn_act_ref(c["z"], mean, invstd, c["gamma"], c["beta"], dt=np.float32)["pre"][0], 0))
    da = f32(rng(300 + M + C + seed).standard_normal((M, C)))
    return dict(z=c["z"], a=a, da=da, mean=mean, invstd=invstd, gamma=c["gamma"])


TIE_ROWS = {"low_late": (1, 4), "low_first": (4, 5)}
POOL_CASES = [(B, N, C, kind) for B in POOL_B for N in POOL_N for C in POOL_C
              for kind in ("relu", "ties") + tuple(k for k, (_, hi) in TIE_ROWS.items() if N > hi)]


def make_pool(B, N, C, kind, seed=0):
    """a [B, N, C] >= 0 as after ReLU.  'relu': continuous values, about half of them 0, columns c % 5 == 0 all zero.  'ties': small integers,
    so maxima repeat within and across the four row groups (rows r, r + 4, ..).  'low_late' / 'high_first': the maximum of every column sits at
    two rows only: rows 1 and 4 (the LOW row is in group 1, the higher one in group 0: the cross-group rule must prefer the lower row over group
    0's own) or rows 4 and 5 (the low row is group 0's second, the higher one group 1's: the other way round)."""
    g = rng(400 + 17 * N + C + B + seed)
    if kind == "relu":
        a = np.maximum(g.standard_normal((B, N, C)), 0.0)
        a[:, :, ::5] = 0.0
    elif kind == "ties":
        a = g.integers(0, 3, (B, N, C)).astype(np.float64)
    else:
        a = g.uniform(0.0, 1.0, (B, N, C))
        lo, hi = TIE_ROWS[kind]
        a[:, lo] = 5.0
        a[:, hi] = 5.0
    return f32(a)


def make_mix(R, N, k, seed=0):
    g = rng(500 + R + 3 * N + k + seed)
    return dict(x=f32(g.standard_normal((R, 9))), T=f32(g.standard_normal(((R - 1) // N + 1, k, k))))


def make_lsm(B, C, shift, seed=0):
    g = rng(600 + 5 * B + C + seed)
    return dict(z=f32(g.standard_normal((B, C)) * 3.0 + shift), d=f32(g.standard_normal((B, C))))


def make_fold(C, bias, bn, seed=0):
    g = rng(700 + C + 2 * bias + bn + seed)
    return dict(bias=f32(g.standard_normal(C)) if bias else None, gamma=f32(g.uniform(0.5, 1.5, C) * g.choice([-1.0, 1.0], C)) if bn else None,
                beta=f32(g.uniform(-0.5, 0.5, C)), rm=f32(g.uniform(-1.0, 1.0, C)), rv=f32(g.uniform(0.5, 2.0, C)))


def make_layer(c, seed=0):
    g = rng(800 + c["M"] + c["C"] + c["K"] + c["w0"] + seed)
    M, C = c["M"], c["C"]
    st = make_stats(M, C, seed + 77)
    return dict(A=f32(g.standard_normal((M, c["lda"]))), W=f32(g.standard_normal((C, c["ldw"])) * 0.3), bias=f32(g.standard_normal(C)) if c["bias"] else None,
                add=f32(g.standard_normal(((M - 1) // 22 + 1, C))) if c["add"] else None, per=22, gamma=st["gamma"] if c["bn"] else None, beta=st["beta"],
                rm=st["rm"], rv=st["rv"], da=f32(g.standard_normal((M, C))), dA0=f32(g.standard_normal((M, c["K"] + 2))))


# ---- the backward entry points repeat the train forward's shape limits: refused on the host before anything is read ------------------------
def backward_shape_refusals():
    """[(entry point, B, N, classes, return code, error text)] of ampnet_pointnet_seg_bwd_f32 / ampnet_pointnet_cls_bwd_f32 called with shapes the train
    forward refuses.  Every pointer is a non-NULL dummy that a refusal never dereferences; needs no GPU."""
    lib = L.lib()
    vp = ctypes.c_void_p
    tab = (vp * (21 * 6))(*([1] * (21 * 6)))
    lib.ampnet_pointnet_seg_bwd_f32.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]
    lib.ampnet_pointnet_cls_bwd_f32.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_uint32, vp, vp, vp,
                                                ctypes.c_size_t, vp]
    out = []
    for B, N, C in ((1, 8, 4), (0, 8, 4), (2, 0, 4), (2, 8, 65), (2, 8, 0), (4096, 4096, 4)):
        p = ctypes.cast(tab, vp)
        out.append(("seg", B, N, C, lib.ampnet_pointnet_seg_bwd_f32(p, p, 1, p, B, N, C, p, None, p, 0, None), PP.last_error()))
        out.append(("cls", B, N, C, lib.ampnet_pointnet_cls_bwd_f32(p, p, 1, p, B, N, C, 0.3, 1, p, None, p, 0, None), PP.last_error()))
    return out
