"""The train-mode (batch-statistics) set abstraction of the C ABI (include/ampnet_hip.h: ampnet_sa_train_forward_f32,
ampnet_sa_train_backward_f32) against the float64 restatement tests/sa_train_ref.py, which is fed the same groups and the kernel's own
choice of the max's row.  The bars are derived in sa_train_ref.sa_train's docstring; the worst error / bar ratio of every output of every
case is printed.  Depth and width that the bars of a chained restatement cannot settle are checked layer by layer on the backward's own
tape (ampnet_sa_train_backward_tape, sa_train_ref.check_layers)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import sa_train_ref as R                           # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -1234.5
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The inputs of a case, computed once and shared (nobody writes to them)."""
    return R.case_inputs(sub("synthetic"), name)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Outs:
    """Output tensors in front of 64 guard words each, which the kernels must leave alone."""

    def __init__(self, prefill):
        self.prefill, self.bufs = prefill, {}

    def new(self, name, shape, dtype=torch.float32):
        numel = int(np.prod(shape))
        fill = self.prefill if dtype == torch.float32 else -77
        buf = torch.full((numel + 64,), fill, dtype=dtype, device=DEV)
        buf[numel:] = int(GUARD) if dtype != torch.float32 else GUARD
        self.bufs[name] = buf
        return buf[:numel].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for name, buf in self.bufs.items():
            assert (buf[-64:] == (GUARD if buf.dtype == torch.float32 else int(GUARD))).all(), f"{name}: written past its end"


def _forward(L, xyz, centres, group_idx, feats, layers, prefill=float("nan"), momentum=R.MOMENTUM, ws_short=0, save_mean="auto"):
    """The train forward on device tensors (layers: tuples of six DEVICE tensors, whose running statistics are updated in place)
    -> (out, save_mean, save_invstd)."""
    B, s, nsample = group_idx.shape
    couts = [int(layer[0].shape[0]) for layer in layers]
    o = _Outs(prefill)
    out = o.new("out", (B, s, couts[-1]))
    sm = o.new("save_mean", (sum(couts),)) if isinstance(save_mean, str) else save_mean
    si = o.new("save_invstd", (sum(couts),))
    D = 0 if feats is None else feats.shape[2]
    try:
        need = L.sa_train_forward_workspace_bytes(D, B, s, nsample, couts)
    except L.AmpnetError:
        need = 1 << 20                                             # a refused shape: the forward has to say so itself
    ws = torch.full((need - ws_short,), 0xAB, dtype=torch.uint8, device=DEV)
    L.sa_train_forward_f32(xyz, centres, group_idx, feats, layers, [R.BN_EPS] * len(layers), momentum, out, sm, si, ws)
    o.check()
    return out, sm, si


def _backward(L, xyz, centres, group_idx, feats, layers, sm, si, dout, prefill=float("nan"), ws_short=0, tape=False):
    """The train backward on device tensors -> {name: device tensor}; tape: also x{l} and dz{l}, read from the workspace through the
    test hook."""
    B, s, nsample = group_idx.shape
    couts = [int(layer[0].shape[0]) for layer in layers]
    o = _Outs(prefill)
    res = {"arg": o.new("arg", (B, s, couts[-1]), torch.int32)}
    if feats is not None:
        res["dfeats"] = o.new("dfeats", feats.shape)
    grads = []
    for l, layer in enumerate(layers):
        grads.append(tuple(o.new(f"{k}{l}", layer[j].shape) for k, j in (("dW", 0), ("dbias", 1), ("dgamma", 1), ("dbeta", 1))))
        res.update({f"{k}{l}": g for k, g in zip(("dW", "dbias", "dgamma", "dbeta"), grads[-1])})
    D = 0 if feats is None else feats.shape[2]
    try:
        need = L.sa_train_backward_workspace_bytes(D, B, s, nsample, couts)
    except L.AmpnetError:
        need = 1 << 20
    ws = torch.full((need - ws_short + 256,), 0xAB, dtype=torch.uint8, device=DEV)        # 256 guard bytes behind what the call is given
    L.sa_train_backward_f32(xyz, centres, group_idx, feats, layers, [R.BN_EPS] * len(layers), sm, si, dout, res.get("dfeats"), grads,
                            ws[:need - ws_short], arg_out=res["arg"])
    o.check()
    assert (ws[need - ws_short:] == 0xAB).all(), "the workspace was written past its end"
    if tape:
        M = B * s * nsample
        words = ws[:need // 4 * 4].view(torch.float32)
        for l in range(len(layers)):
            xo, xs, dzo, dzs = L.sa_train_backward_tape(D, B, s, nsample, couts, l)
            res[f"x{l}"] = words[xo // 4:xo // 4 + M * xs].view(M, xs).clone()
            res[f"dz{l}"] = words[dzo // 4:dzo // 4 + M * dzs].view(M, dzs).clone()
    return res


def _run(L, i, prefill=float("nan"), tape=False):
    """Forward and backward of a case from its numpy inputs -> {name: numpy array}."""
    xyz, centres, group_idx, feats, dout = (_t(i[k]) for k in ("xyz", "centres", "group_idx", "feats", "dout"))
    layers = [tuple(_t(a) for a in layer) for layer in i["layers"]]              # fresh running statistics for every run
    out, sm, si = _forward(L, xyz, centres, group_idx, feats, layers, prefill)
    res = {"out": out}
    off = 0
    for l, layer in enumerate(layers):
        c = layer[0].shape[0]
        res.update({f"save_mean{l}": sm[off:off + c], f"save_invstd{l}": si[off:off + c], f"running_mean{l}": layer[4],
                    f"running_var{l}": layer[5]})
        off += c
    res.update(_backward(L, xyz, centres, group_idx, feats, layers, sm, si, dout, prefill, tape=tape))
    return {k: v.cpu().numpy() for k, v in res.items()}


def _three_runs(L, i, name, tape=False):
    """A run on NaN-prefilled outputs (every element must be written), a second one (the same bits) and one under a bf16 precision scope
    (the same bits: exact fp32 whatever the matrix precision is) -> the first run's outputs."""
    got = _run(L, i, tape=tape)
    for k, v in got.items():
        assert np.isfinite(v).all(), (name, k)
    again = _run(L, i, prefill=-7.0, tape=tape)
    for k in got:
        assert np.array_equal(got[k], again[k]), (name, k)
    with L.precision_scope("bf16"):
        scoped = _run(L, i, tape=tape)
    for k in got:
        assert np.array_equal(got[k], scoped[k]), (name, k)
    for l, layer in enumerate(i["layers"]):
        assert (got[f"dbias{l}"] == 0).all(), (name, l)            # the bias has no effect on a batch-normalised output
        assert not np.array_equal(got[f"running_mean{l}"], layer[4]) and not np.array_equal(got[f"running_var{l}"], layer[5]), (name, l)
    return got


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_sa_train_within_the_derived_bar(name):
    L = sub("_lib")
    i = _inputs(name)
    got = _three_runs(L, i, name)
    tape, _ = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    R.check_argmax(got["arg"], tape[-1], i["group_idx"])           # the kernel's choice of the max's row is admissible
    want = R.sa_train(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], i["dout"], got["arg"], tape)
    assert sorted(got) == sorted(list(want) + ["arg"])
    ratios = {}
    for k in R.output_names(len(i["layers"]), i["feats"] is not None):
        v, bar = want[k]
        assert got[k].shape == v.shape, (name, k)
        err = np.abs(got[k].astype(np.float64) - v)
        ratios[k] = float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max())     # (0 / 0: an exact value met exactly)
    print(f"sa_train {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    # (`out` above is compared at arg_out: out[g, c] is the forward's relu(y) at the row the backward found the maximum in)
    assert (got["out"] >= 0).all() and (got["out"] != 0).any()
    if i["feats"] is not None:
        for c, u in enumerate(i["unpicked"]):
            assert (got["dfeats"][c, u] == 0).all(), (name, c, u)  # in no group: exact zeros, and written
        assert not np.array_equal(got["dfeats"][0], got["dfeats"][1]) and (got["dfeats"] != 0).any()
    if name == "unpicked":
        assert all(len(u) >= 2 for u in i["unpicked"])
    if name == "sparse_ball":
        assert (i["count"] == 1).any()                             # some ball holds its centre alone: its other slots are rows all the same
    if name == "negative_gamma":
        for k, v in got.items():
            assert k.startswith("dbias") or k == "arg" or (v != 0).mean() > 0.2, (k, float((v != 0).mean()))      # the ReLU did not wipe the case out
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


@pytest.mark.parametrize("name", [c[0] for c in R.LOCAL])
def test_every_layer_alone_on_the_backward_tape(name):
    L = sub("_lib")
    i = _inputs(name)
    got = _three_runs(L, i, name, tape=True)
    ratios = R.check_layers(i, got)                                # asserts the cap on undecided ReLU inputs and check_argmax
    print(f"sa_train local {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k, v in got.items():
        assert k.startswith("dbias") or (v != 0).any(), (name, k)
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


def test_sa_train_refusals():
    """Every misuse is an AmpnetError that says what is wrong; the eval entry points' limits hold here too."""
    L = sub("_lib")
    i = _inputs("tail_group")                                      # n 70, s 9, nsample 20, D 6, [32, 64]
    xyz, centres, group_idx, feats, dout = (_t(i[k]) for k in ("xyz", "centres", "group_idx", "feats", "dout"))
    dev = lambda ls: [tuple(_t(a) for a in layer) for layer in ls]
    layers = dev(i["layers"])
    before = [layer[4].clone() for layer in layers]
    out, sm, si = _forward(L, xyz, centres, group_idx, feats, layers)
    one = (xyz[:1], centres[:1, :1].contiguous(), group_idx[:1, :1, :1].contiguous(), feats[:1])
    with pytest.raises(L.AmpnetError, match="M = n_clouds"):       # one row has no batch statistics
        _forward(L, *one, layers)
    with pytest.raises(L.AmpnetError, match="M = n_clouds"):
        _backward(L, *one, layers, sm, si, dout[:1, :1].contiguous())
    for m in (-0.1, 1.5, float("nan")):
        with pytest.raises(L.AmpnetError, match="momentum"):
            _forward(L, xyz, centres, group_idx, feats, layers, momentum=m)
    for need in (L.sa_train_forward_workspace_bytes, L.sa_train_backward_workspace_bytes):
        with pytest.raises(L.AmpnetError, match="exceed 16777216"):            # row counts are carried as floats: M past 2^24 is refused
            need(6, 2, (1 << 18) + 1, 32, [32, 64])
        assert need(6, 2, 1 << 18, 32, [32]) > 0                               # 2^24 rows themselves are accepted
    with pytest.raises(L.AmpnetError, match="workspace"):
        _forward(L, xyz, centres, group_idx, feats, layers, ws_short=1)
    with pytest.raises(L.AmpnetError, match="workspace"):
        _backward(L, xyz, centres, group_idx, feats, layers, sm, si, dout, ws_short=1)
    with pytest.raises(L.AmpnetError, match="save_mean"):
        _forward(L, xyz, centres, group_idx, feats, layers, save_mean=None)
    with pytest.raises(L.AmpnetError, match="dout"):
        _backward(L, xyz, centres, group_idx, feats, layers, sm, si, dout[:, :, :32].contiguous())
    # the eval entry points' limits (tests/test_set_abstraction_gpu.py, tests/test_sa_backward_gpu.py)
    s48, s128, s32 = (torch.zeros(c, device=DEV) for c in (48, 128, 32))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _forward(L, xyz, centres, group_idx, feats, dev(R.make_layers(1, 9, [48])))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _backward(L, xyz, centres, group_idx, feats, dev(R.make_layers(1, 9, [48])), s48, s48, torch.zeros((2, 9, 48), device=DEV))
    with pytest.raises(L.AmpnetError, match="layers"):
        _forward(L, xyz, centres, group_idx, feats, dev(R.make_layers(1, 9, [32, 32, 32, 32])))
    with pytest.raises(L.AmpnetError, match="layers"):
        _backward(L, xyz, centres, group_idx, feats, dev(R.make_layers(1, 9, [32, 32, 32, 32])), s128, s128, torch.zeros((2, 9, 32), device=DEV))
    big = torch.zeros((2, 9, 65), dtype=torch.int32, device=DEV)
    with pytest.raises(L.AmpnetError, match="nsample"):
        _forward(L, xyz, centres, big, feats, layers)
    with pytest.raises(L.AmpnetError, match="nsample"):
        _backward(L, xyz, centres, big, feats, layers, sm, si, dout)
    wide = torch.zeros((2, 70, 318), device=DEV)
    with pytest.raises(L.AmpnetError, match="320"):
        _forward(L, xyz, centres, group_idx, wide, dev(R.make_layers(1, 321, [32])))
    with pytest.raises(L.AmpnetError, match="320"):
        _backward(L, xyz, centres, group_idx, wide, dev(R.make_layers(1, 321, [32])), s32, s32, torch.zeros((2, 9, 32), device=DEV))
    # the LDS limit of the backward: nsample = 64 (two row tiles) with cin_0 = 320 and [256, 256, 256] -- from all four entry points
    stack = [256, 256, 256]
    for need in (L.sa_train_forward_workspace_bytes, L.sa_train_backward_workspace_bytes):
        with pytest.raises(L.AmpnetError, match="workspace_bytes.*LDS"):
            need(317, 2, 9, 64, stack)
        assert need(317, 2, 9, 32, stack) > 0                      # the same stack at nsample = 32 is accepted
    with pytest.raises(L.AmpnetError, match="tape.*LDS"):
        L.sa_train_backward_tape(317, 2, 9, 64, stack, 0)
    with pytest.raises(L.AmpnetError, match="layer 3"):
        L.sa_train_backward_tape(317, 2, 9, 32, stack, 3)
    dummy = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    p = ctypes.c_void_p(dummy.data_ptr())
    table = (ctypes.c_void_p * 18)(*[dummy.data_ptr()] * 18)
    gtable = (ctypes.c_void_p * 12)(*[dummy.data_ptr()] * 12)
    couts, epss = (ctypes.c_int * 3)(*stack), (ctypes.c_float * 3)(*[1e-5] * 3)
    nbytes = ctypes.c_size_t(dummy.numel() * 4)
    rc = L.lib().ampnet_sa_train_forward_f32(p, 2, 70, 3, p, 9, p, 64, p, 317, table, couts, epss, 3, ctypes.c_float(0.1), p, p, p, p, nbytes,
                                             None)                 # (refused before any launch)
    assert rc != 0
    with pytest.raises(L.AmpnetError, match="ampnet_sa_train_forward_f32.*LDS"):
        L.check(rc, "ampnet_sa_train_forward_f32")
    rc = L.lib().ampnet_sa_train_backward_f32(p, 2, 70, 3, p, 9, p, 64, p, 317, table, couts, epss, 3, p, None, gtable, None, p, nbytes, None)
    assert rc != 0
    with pytest.raises(L.AmpnetError, match="ampnet_sa_train_backward_f32.*LDS"):
        L.check(rc, "ampnet_sa_train_backward_f32")
    # nothing above touched the statistics of the one call that ran
    f = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])[0]
    for l, layer in enumerate(layers):
        v, bar = f[l]["rm"]
        assert (np.abs(layer[4].cpu().numpy() - v) <= bar).all() and not torch.equal(layer[4], before[l])
