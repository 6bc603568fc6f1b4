"""The train-mode (batch-statistics) feature propagation of the C ABI (include/ampnet_hip.h: ampnet_fp_train_forward_f32,
ampnet_fp_train_backward_f32) against the float64 restatement tests/fp_train_ref.py, which is fed the same neighbours and squared
distances.  The bars are derived in fp_train_ref.fp_train's docstring; the worst error / bar ratio of every output of every case is
printed.  Depth and width that the bars cannot settle are checked by composition: an L-layer call against L chained one-layer calls."""
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
import fp_train_ref as R                           # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -1234.5
NAMES = [c[0] for c in R.CASES]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, reference) of a restatement case, computed once and shared (nobody writes to them)."""
    i = R.case_inputs(sub("synthetic"), name)
    want, _ = R.fp_train(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])
    return i, want


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Outs:
    """Output tensors in front of 64 guard floats each, which the kernels must leave alone."""

    def __init__(self, prefill):
        self.prefill, self.bufs = prefill, {}

    def new(self, name, shape):
        numel = int(np.prod(shape))
        buf = torch.full((numel + 64,), self.prefill, dtype=torch.float32, device=DEV)
        buf[numel:] = GUARD
        self.bufs[name] = buf
        return buf[:numel].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for name, buf in self.bufs.items():
            assert (buf[-64:] == GUARD).all(), f"{name}: written past its end"


def _forward(L, p1, p2, idx, dist2, layers, prefill=float("nan"), momentum=R.MOMENTUM, ws_short=0, save_mean="auto"):
    """The train forward on device tensors (layers: tuples of six DEVICE tensors, whose running statistics are updated in place)
    -> (out, save_mean, save_invstd)."""
    B, n, _ = idx.shape
    couts = [int(layer[0].shape[0]) for layer in layers]
    o = _Outs(prefill)
    out = o.new("out", (B, n, couts[-1]))
    sm = o.new("save_mean", (sum(couts),)) if isinstance(save_mean, str) else save_mean
    si = o.new("save_invstd", (sum(couts),))
    D1 = 0 if p1 is None else p1.shape[2]
    try:
        need = L.fp_train_forward_workspace_bytes(D1, p2.shape[2], B, n, couts)
    except L.AmpnetError:
        need = 1 << 20                                             # a refused shape: the forward has to say so itself
    ws = torch.full((need - ws_short,), 0xAB, dtype=torch.uint8, device=DEV)
    L.fp_train_forward_f32(p1, p2, idx, dist2, layers, [R.BN_EPS] * len(layers), momentum, out, sm, si, ws)
    o.check()
    return out, sm, si


def _backward(L, p1, p2, idx, dist2, layers, sm, si, dout, prefill=float("nan"), ws_short=0):
    """The train backward on device tensors -> {name: device tensor}."""
    B, n, _ = idx.shape
    couts = [int(layer[0].shape[0]) for layer in layers]
    o = _Outs(prefill)
    res = {"dpoints2": o.new("dpoints2", p2.shape)}
    if p1 is not None:
        res["dpoints1"] = o.new("dpoints1", p1.shape)
    grads = []
    for l, layer in enumerate(layers):
        grads.append(tuple(o.new(f"{k}{l}", layer[j].shape) for k, j in (("dW", 0), ("dbias", 1), ("dgamma", 1), ("dbeta", 1))))
        res.update({f"{k}{l}": g for k, g in zip(("dW", "dbias", "dgamma", "dbeta"), grads[-1])})
    D1 = 0 if p1 is None else p1.shape[2]
    try:
        need = L.fp_train_backward_workspace_bytes(D1, p2.shape[2], B, n, couts)
    except L.AmpnetError:
        need = 1 << 20
    ws = torch.full((need - ws_short,), 0xAB, dtype=torch.uint8, device=DEV)
    L.fp_train_backward_f32(p1, p2, idx, dist2, layers, [R.BN_EPS] * len(layers), sm, si, dout, res.get("dpoints1"), res["dpoints2"], grads, ws)
    o.check()
    return res


def _run(L, i, prefill=float("nan")):
    """Forward and backward of a case from its numpy inputs -> {fp_train_ref name: numpy array}."""
    p1, p2, idx, dist2, dout = (_t(i[k]) for k in ("points1", "points2", "idx", "dist2", "dout"))
    layers = [tuple(_t(a) for a in layer) for layer in i["layers"]]              # fresh running statistics for every run
    out, sm, si = _forward(L, p1, p2, idx, dist2, layers, prefill)
    res = {"out": out}
    off = 0
    for l, layer in enumerate(layers):
        c = layer[0].shape[0]
        res.update({f"save_mean{l}": sm[off:off + c], f"save_invstd{l}": si[off:off + c], f"running_mean{l}": layer[4],
                    f"running_var{l}": layer[5]})
        off += c
    res.update(_backward(L, p1, p2, idx, dist2, layers, sm, si, dout, prefill))
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", NAMES)
def test_fp_train_within_the_derived_bar(name):
    L = sub("_lib")
    i, want = _case(name)
    got = _run(L, i)                                               # every output starts as NaN: every element must be written
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        assert np.isfinite(v).all(), (name, k)
    again = _run(L, i, prefill=-7.0)
    for k in got:
        assert np.array_equal(got[k], again[k]), (name, k)         # bitwise the same on a second run
    with L.precision_scope("bf16"):
        scoped = _run(L, i)
    for k in got:
        assert np.array_equal(got[k], scoped[k]), (name, k)        # exact fp32 whatever the precision scope
    ratios = {}
    for k in R.output_names(len(i["layers"]), i["points1"] is not None):
        v, bar = want[k]
        assert got[k].shape == v.shape, (name, k)
        err = np.abs(got[k].astype(np.float64) - v)
        ratios[k] = float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max())     # (0 / 0: an exact value met exactly)
    print(f"fp_train {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for l in range(len(i["layers"])):
        assert (got[f"dbias{l}"] == 0).all(), (name, l)            # the bias has no effect on a batch-normalised output
    for c, u in enumerate(i["unpicked"]):
        assert (got["dpoints2"][c, u] == 0).all(), (name, c, u)    # nobody's neighbour: exact zeros, and written
    if name == "unpicked":
        assert all(len(u) >= 2 for u in i["unpicked"])
    if name == "negative_gamma":
        for k, v in got.items():
            assert k.startswith("dbias") or (v != 0).mean() > 0.2, (k, float((v != 0).mean()))      # the ReLU did not wipe the case out
    assert not np.array_equal(got["dpoints2"][0], got["dpoints2"][1])
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


@pytest.mark.parametrize("name", [c[0] for c in R.COMPOSE])
def test_layers_compose_bit_for_bit(name):
    """Depth and width by composition: the L-layer forward and backward equal the chain of L one-layer calls, bit for bit.  Layer l >= 1
    of the chain takes the previous call's output as points2 with identity neighbours (s = n, k = 1, idx[i] = i, dist2 = 0): the
    interpolation weight is exactly 1 and dpoints2 is dx exactly; its dout is the next call's dpoints2.  Both sides run the same per-layer
    code on the same rows in the same tile order, so equal bits are expected."""
    L = sub("_lib")
    i = R.case_inputs(sub("synthetic"), name)
    p1, p2, idx, dist2, dout = (_t(i[k]) for k in ("points1", "points2", "idx", "dist2", "dout"))
    fused = [tuple(_t(a) for a in layer) for layer in i["layers"]]
    chain = [tuple(_t(a) for a in layer) for layer in i["layers"]]
    nl = len(fused)
    B, n, _ = idx.shape
    out, sm, si = _forward(L, p1, p2, idx, dist2, fused)
    got = _backward(L, p1, p2, idx, dist2, fused, sm, si, dout)
    ident = torch.arange(n, dtype=torch.int32, device=DEV).repeat(B, 1)[:, :, None].contiguous()
    zero = torch.zeros((B, n, 1), dtype=torch.float32, device=DEV)
    args = [(p1, p2, idx, dist2)]
    fwd = []
    for l in range(nl):
        fwd.append(_forward(L, *args[l], [chain[l]]))
        args.append((None, fwd[l][0].contiguous(), ident, zero))
    assert torch.equal(out, fwd[-1][0])
    assert torch.equal(sm, torch.cat([f[1] for f in fwd])) and torch.equal(si, torch.cat([f[2] for f in fwd]))
    for l in range(nl):
        assert torch.equal(fused[l][4], chain[l][4]) and torch.equal(fused[l][5], chain[l][5]), (name, l)      # the running statistics
        assert not torch.equal(fused[l][4], _t(i["layers"][l][4])), (name, l)                                  # .. which did move
    d = dout
    for l in range(nl - 1, -1, -1):
        one = _backward(L, *args[l], [chain[l]], fwd[l][1], fwd[l][2], d.contiguous())
        for k in ("dW", "dgamma", "dbeta", "dbias"):
            assert torch.equal(got[f"{k}{l}"], one[f"{k}0"]), (name, k, l)
        d = one["dpoints2"]
    assert torch.equal(got["dpoints2"], one["dpoints2"])
    if p1 is not None:
        assert torch.equal(got["dpoints1"], one["dpoints1"])
    for k, v in got.items():
        assert torch.isfinite(v).all() and (k.startswith("dbias") or (v != 0).any()), (name, k)


def test_fp_train_refusals():
    """Every misuse is an AmpnetError that says what is wrong; the eval entry points' limits hold here too."""
    L = sub("_lib")
    i, _ = _case("tail_tile")                                      # n 70, s 9, D1 16, D2 32, [32, 64]
    p1, p2, idx, dist2, dout = (_t(i[k]) for k in ("points1", "points2", "idx", "dist2", "dout"))
    layers = [tuple(_t(a) for a in layer) for layer in i["layers"]]
    out, sm, si = _forward(L, p1, p2, idx, dist2, layers)
    with pytest.raises(L.AmpnetError, match="M = n_clouds"):       # one row has no batch statistics
        _forward(L, p1[:1, :1].contiguous(), p2[:1], idx[:1, :1].contiguous(), dist2[:1, :1].contiguous(), layers)
    with pytest.raises(L.AmpnetError, match="M = n_clouds"):
        _backward(L, p1[:1, :1].contiguous(), p2[:1], idx[:1, :1].contiguous(), dist2[:1, :1].contiguous(), layers, sm, si,
                  dout[:1, :1].contiguous())
    for m in (-0.1, 1.5, float("nan")):
        with pytest.raises(L.AmpnetError, match="momentum"):
            _forward(L, p1, p2, idx, dist2, layers, momentum=m)
    for need in (L.fp_train_forward_workspace_bytes, L.fp_train_backward_workspace_bytes):
        with pytest.raises(L.AmpnetError, match="exceed 16777216"):            # row counts are carried as floats: M past 2^24 is refused
            need(16, 32, 2, (1 << 23) + 1, [32, 64])
        assert need(16, 32, 1, 1 << 24, [32]) > 0                              # 2^24 rows themselves are accepted
    with pytest.raises(L.AmpnetError, match="workspace"):
        _forward(L, p1, p2, idx, dist2, layers, ws_short=1)
    with pytest.raises(L.AmpnetError, match="workspace"):
        _backward(L, p1, p2, idx, dist2, layers, sm, si, dout, ws_short=1)
    with pytest.raises(L.AmpnetError, match="save_mean"):
        _forward(L, p1, p2, idx, dist2, layers, save_mean=None)
    # the eval entry points' limit cases (tests/test_feature_propagation_gpu.py::test_fp_forward_refusals)
    dev = lambda ls: [tuple(_t(a) for a in layer) for layer in ls]
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _forward(L, p1, p2, idx, dist2, dev(R.make_layers(1, 48, [48])))
    with pytest.raises(L.AmpnetError, match="layers"):
        _forward(L, p1, p2, idx, dist2, dev(R.make_layers(1, 48, [32, 32, 32, 32])))
    wide1, wide2 = torch.zeros((2, 70, 257), device=DEV), torch.zeros((2, 9, 256), device=DEV)
    with pytest.raises(L.AmpnetError, match="512"):
        _forward(L, wide1, wide2, idx, dist2, dev(R.make_layers(1, 513, [32])))
    s48, s4, s513 = (torch.zeros(c, device=DEV) for c in (48, 128, 32))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _backward(L, p1, p2, idx, dist2, dev(R.make_layers(1, 48, [48])), s48, s48, torch.zeros((2, 70, 48), device=DEV))
    with pytest.raises(L.AmpnetError, match="layers"):
        _backward(L, p1, p2, idx, dist2, dev(R.make_layers(1, 48, [32, 32, 32, 32])), s4, s4, torch.zeros((2, 70, 32), device=DEV))
    with pytest.raises(L.AmpnetError, match="512"):
        _backward(L, wide1, wide2, idx, dist2, dev(R.make_layers(1, 513, [32])), s513, s513, torch.zeros((2, 70, 32), device=DEV))
    with pytest.raises(L.AmpnetError, match="workspace_bytes"):
        L.fp_train_forward_workspace_bytes(16, 32, 2, 70, [32, 40])
    with pytest.raises(L.AmpnetError, match="workspace_bytes"):
        L.fp_train_backward_workspace_bytes(16, 32, 2, 70, [32, 40])
    # nothing above touched the statistics of the one call that ran
    want = _case("tail_tile")[1]
    for l, layer in enumerate(layers):
        v, bar = want[f"running_mean{l}"]
        assert (np.abs(layer[4].cpu().numpy() - v) <= bar).all()
