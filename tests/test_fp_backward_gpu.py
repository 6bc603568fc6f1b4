"""The fused feature-propagation backward (include/ampnet_hip.h: ampnet_fp_backward_f32) against the float64 restatement
tests/fp_bwd_ref.py, which is fed the same neighbours and squared distances.  The bars are derived in fp_bwd_ref.fp_backward's docstring;
the worst error / bar ratio of every output of every case is printed."""
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
import fp_bwd_ref as R                             # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -1234.5
NAMES = [c[0] for c in R.CASES]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, reference) of a case, computed once and shared (nobody writes to them)."""
    i = R.case_inputs(sub("synthetic"), name)
    want, _ = R.fp_backward(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])
    return i, want


def _run(L, i, prefill=float("nan"), dout=None, ws_short=0, dp1="auto", layers=None, points1="auto", points2=None):
    """-> {name: numpy array}.  Every output lives in front of 64 guard floats, which the kernels must leave alone."""
    dev = "cuda"
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p1 = i["points1"] if isinstance(points1, str) else points1
    p2 = i["points2"] if points2 is None else points2
    layers = i["layers"] if layers is None else layers
    B, n, _ = i["idx"].shape
    bufs = {}

    def out(name, shape):
        numel = int(np.prod(shape))
        buf = torch.full((numel + 64,), prefill, dtype=torch.float32, device=dev)
        buf[numel:] = GUARD
        bufs[name] = buf
        return buf[:numel].view(*shape)

    res = {"dpoints2": out("dpoints2", p2.shape)}
    if isinstance(dp1, str):
        dp1 = None if p1 is None else out("dpoints1", p1.shape)
    if dp1 is not None:
        res["dpoints1"] = dp1
    grads = []
    for l, layer in enumerate(layers):
        grads.append(tuple(out(f"{k}{l}", layer[j].shape) for k, j in (("dW", 0), ("dbias", 1), ("dgamma", 1), ("dbeta", 1))))
        res.update({f"{k}{l}": g for k, g in zip(("dW", "dbias", "dgamma", "dbeta"), grads[-1])})
    D1 = 0 if p1 is None else p1.shape[2]
    try:
        need = L.fp_backward_workspace_bytes(D1, p2.shape[2], B, n, [layer[0].shape[0] for layer in layers])
    except L.AmpnetError:
        need = 1 << 20                                             # a refused shape: fp_backward_f32 has to say so itself
    ws = torch.full((need - ws_short,), 0xAB, dtype=torch.uint8, device=dev)
    L.fp_backward_f32(t(p1), t(p2), t(i["idx"]), t(i["dist2"]), [tuple(t(a) for a in layer) for layer in layers], [R.BN_EPS] * len(layers),
                      t(i["dout"] if dout is None else dout), dp1, res["dpoints2"], grads, ws)
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        assert (buf[-64:] == GUARD).all(), f"{name}: written past its end"
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", NAMES)
def test_fp_backward_within_the_derived_bar(name):
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
        ratios[k] = float((np.abs(got[k].astype(np.float64) - v) / np.maximum(bar, 1e-300)).max())
    print(f"fp_backward {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for c, u in enumerate(i["unpicked"]):
        assert (got["dpoints2"][c, u] == 0).all(), (name, c, u)    # nobody's neighbour: exact zeros, and written
    if name == "unpicked":
        assert all(len(u) >= 2 for u in i["unpicked"])
    if name == "negative_gamma":
        for k, v in got.items():
            assert (v != 0).mean() > 0.2, (k, float((v != 0).mean()))          # the ReLU did not wipe the case out
    assert not np.array_equal(got["dpoints2"][0], got["dpoints2"][1])
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


def test_fp_backward_refusals():
    """Every misuse is an AmpnetError that says what is wrong; shapes outside the forward's limits are refused the same way."""
    L = sub("_lib")
    i, _ = _case("tail_tile")                                      # n 70, s 9, D1 16, D2 32, [32, 64]
    with pytest.raises(L.AmpnetError, match="dout"):
        _run(L, i, dout=i["dout"][:, :, :32])
    with pytest.raises(L.AmpnetError, match="dout"):
        _run(L, i, dout=i["dout"][:, :69])
    with pytest.raises(L.AmpnetError, match="workspace"):
        _run(L, i, ws_short=1)
    with pytest.raises(L.AmpnetError, match="dpoints1"):
        _run(L, i, dp1=None)                                       # missing with D1 > 0
    j, _ = _case("three_layers")                                   # D1 = 0
    with pytest.raises(L.AmpnetError, match="dpoints1"):
        _run(L, j, dp1=torch.zeros((2, 96, 4), device="cuda"))     # given with D1 = 0
    # the forward's limit cases (tests/test_feature_propagation_gpu.py::test_fp_forward_refusals)
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, dict(i, dout=i["dout"][:, :, :48]), layers=R.make_layers(1, 48, [48]))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, dict(i, dout=np.zeros((2, 70, 288), np.float32)), layers=R.make_layers(1, 48, [32, 288]))
    wide1, wide2 = np.zeros((2, 70, 257), np.float32), np.zeros((2, 9, 256), np.float32)
    with pytest.raises(L.AmpnetError, match="512"):
        _run(L, dict(i, dout=i["dout"][:, :, :32]), layers=R.make_layers(1, 513, [32]), points1=wide1, points2=wide2)
    with pytest.raises(L.AmpnetError, match="layers"):
        _run(L, dict(i, dout=i["dout"][:, :, :32]), layers=R.make_layers(1, 48, [32, 32, 32, 32]))
    short = R.make_layers(1, 48, [32, 64])
    short[1] = (short[1][0][:-1],) + short[1][1:]                  # weight [63, 32]: one row short
    with pytest.raises(L.AmpnetError, match="fp_backward: layer 1 needs"):
        _run(L, i, layers=short)
    with pytest.raises(L.AmpnetError, match="workspace_bytes"):
        L.fp_backward_workspace_bytes(16, 32, 2, 70, [32, 40])
    assert L.fp_backward_workspace_bytes(256, 256, 2, 70, [32]) > 0                # cin_0 = 512 itself is accepted
