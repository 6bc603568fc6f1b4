"""The fused segmentation head (include/ampnet_hip.h: ampnet_seg_head_forward_f32, ampnet_seg_head_backward_f32) against the float64
restatement tests/seg_head_ref.py on its seeded cases.  The bars are derived in that module's docstring; the worst error / bar ratio of every
output of every case is printed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import seg_head_ref as R                           # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PRED_GUARD = -1234.5, -77


def _case(name):
    return R.reference(sub("synthetic"), name)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(shape, prefill, extra=64):
    """A tensor of `shape` in front of `extra` guard floats, which the kernels must leave alone -> (the view, the buffer)."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + extra,), prefill, dtype=torch.float32, device="cuda")
    buf[numel:] = GUARD
    return buf[:numel].view(*shape), buf


def _forward(L, i, want_preds=True, ld=None, prefill=float("nan")):
    """-> (logp [M, C], preds [M] or None) as numpy.  logp is prefilled with NaN and followed by a canary ROW (and more guard floats), preds
    by a canary element; ld > cin pads every input row with NaN columns the kernel must not read."""
    M, cin = i["x"].shape
    C = i["params"][7].shape[0]
    x = i["x"]
    if ld is not None:
        x = np.full((M, ld), np.nan, np.float32)
        x[:, :cin] = i["x"]
    logp, buf = _guarded((M, C), prefill, extra=C + 64)
    preds = torch.full((M + 1,), PRED_GUARD, dtype=torch.int64, device="cuda") if want_preds else None
    ws = torch.full((L.seg_head_forward_workspace_bytes(cin, i["params"][0].shape[0], C, M),), 0xAB, dtype=torch.uint8, device="cuda")
    L.seg_head_forward_f32(_t(x), [_t(p) for p in i["params"]], i["eps"], logp, None if preds is None else preds[:M], ws)
    torch.cuda.synchronize()
    assert (buf[M * C:] == GUARD).all(), "logp: the canary row after M was written"
    if preds is not None:
        assert int(preds[M]) == PRED_GUARD, "preds: written past M"
    return logp.cpu().numpy(), None if preds is None else preds[:M].cpu().numpy()


@pytest.mark.parametrize("name", R.NAMES)
def test_forward_within_the_derived_bar(name):
    L = sub("_lib")
    i, _, fwd = _case(name)
    logp, preds = _forward(L, i)
    assert np.isfinite(logp).all(), name                             # every element was written (the prefill is NaN)
    want, bar = fwd["logp"]
    ratio = float((np.abs(logp.astype(np.float64) - want) / bar).max())
    print(f"seg_head forward {name}: worst error / bar logp {ratio:.3f}")
    # preds: the lowest-index arg-max of the kernel's own log-probabilities, everywhere; the reference's where its arg-max cannot flip
    assert preds.min() >= 0 and preds.max() < logp.shape[1]
    assert np.array_equal(preds, logp.argmax(1)), name
    keep = R.admitted(fwd, i["params"])
    assert np.array_equal(preds[keep], fwd["pred"][keep]), name
    if name == "ties":
        z = fwd["z"][0]
        top = (z[:, 0] == z.max(1)) & keep
        assert top.sum() >= 8 and (preds[top] == 0).all()            # classes 0 and 1 tie exactly: the lower one
        assert np.array_equal(logp[:, 0], logp[:, 1])
    # the same bits without preds, from another prefill, under a bf16 precision scope and with padded input rows
    assert np.array_equal(_forward(L, i, want_preds=False, prefill=-7.0)[0], logp)
    with L.precision_scope("bf16"):
        assert np.array_equal(_forward(L, i)[0], logp)
    assert np.array_equal(_forward(L, i, ld=i["x"].shape[1] + 3)[0], logp)
    assert ratio <= 1.0, (name, ratio)


def _backward(L, i, dx_wanted=True, dlogp=None, prefill=float("nan")):
    """-> {name: numpy array}; every output is prefilled with NaN and lives in front of guard floats."""
    M, cin = i["x"].shape
    hidden, C = i["params"][0].shape[0], i["params"][7].shape[0]
    bufs, res = {}, {}
    for k, shape in (("dx", (M, cin)), ("dW1", (hidden, cin)), ("db1", (hidden,)), ("dgamma", (hidden,)), ("dbeta", (hidden,)),
                     ("dW2", (C, hidden)), ("db2", (C,))):
        if k != "dx" or dx_wanted:
            res[k], bufs[k] = _guarded(shape, prefill)
    ws = torch.full((L.seg_head_backward_workspace_bytes(cin, hidden, C, M),), 0xAB, dtype=torch.uint8, device="cuda")
    L.seg_head_backward_f32(_t(i["x"]), [_t(p) for p in i["params"]], i["eps"], _t(i["dlogp"] if dlogp is None else dlogp), res.get("dx"),
                            [res[k] for k in R.OUTPUTS[1:]], ws)
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        assert (buf[-64:] == GUARD).all(), f"{k}: written past its end"
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", R.NAMES)
def test_backward_within_the_derived_bar(name):
    L = sub("_lib")
    i, want, _ = _case(name)
    got = _backward(L, i)
    assert sorted(got) == sorted(R.OUTPUTS)
    ratios = {}
    for k in R.OUTPUTS:
        v, bar = want[k]
        assert got[k].shape == v.shape and np.isfinite(got[k]).all(), (name, k)
        ratios[k] = float((np.abs(got[k].astype(np.float64) - v) / np.maximum(bar, 1e-300)).max())
    print(f"seg_head backward {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    again = _backward(L, i, prefill=-7.0)
    for k in R.OUTPUTS:
        assert np.array_equal(got[k], again[k]), (name, k)             # bitwise the same on a second run
    no_dx = _backward(L, i, dx_wanted=False)
    assert sorted(no_dx) == sorted(R.OUTPUTS[1:])
    for k in R.OUTPUTS[1:]:
        assert np.array_equal(got[k], no_dx[k]), (name, k)             # dx = NULL changes nothing else
        r = float((np.abs(no_dx[k].astype(np.float64) - want[k][0]) / np.maximum(want[k][1], 1e-300)).max())
        assert r <= 1.0, (name, k, r)
    zeros = _backward(L, i, dlogp=np.zeros_like(i["dlogp"]))
    for k in R.OUTPUTS:
        assert (zeros[k] == 0).all(), (name, k)                       # a gradient of zeros gives exact zeros, and every one written
    if name == "negative_gamma":
        for k in R.OUTPUTS:
            assert (got[k] != 0).mean() > 0.2, (k, float((got[k] != 0).mean()))    # the ReLU did not wipe the case out
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


def test_refusals_reach_the_caller_as_errors():
    """Every misuse is an AmpnetError that says what is wrong, before anything is launched."""
    L = sub("_lib")
    i, _, _ = _case("negative_gamma")                                # M 70, cin 16, hidden 64, C 5
    x, params = _t(i["x"]), [_t(p) for p in i["params"]]
    logp, ws = torch.zeros((70, 5), device="cuda"), torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.AmpnetError, match="workspace"):
        L.seg_head_forward_f32(x, params, i["eps"], logp, None, ws[:511])
    with pytest.raises(L.AmpnetError, match="logp"):
        L.seg_head_forward_f32(x, params, i["eps"], logp[:, :4].contiguous(), None, ws)
    with pytest.raises(L.AmpnetError, match="preds"):
        L.seg_head_forward_f32(x, params, i["eps"], logp, torch.zeros(69, dtype=torch.int64, device="cuda"), ws)
    with pytest.raises(L.AmpnetError, match="ld >= cin"):
        L.seg_head_forward_f32(x[:, :15].contiguous(), params, i["eps"], logp, None, ws)
    with pytest.raises(L.AmpnetError, match="W2 and b2"):
        L.seg_head_forward_f32(x, params[:6] + [params[6][:, :63].contiguous(), params[7]], i["eps"], logp, None, ws)
    with pytest.raises(L.AmpnetError, match="n_classes=33"):
        L.seg_head_forward_f32(x, params[:6] + [torch.zeros((33, 64), device="cuda"), torch.zeros(33, device="cuda")], i["eps"],
                               torch.zeros((70, 33), device="cuda"), None, ws)
    grads = [torch.zeros_like(params[q]) for q in (0, 1, 1, 1, 6, 7)]
    big = torch.zeros(L.seg_head_backward_workspace_bytes(16, 64, 5, 70), dtype=torch.uint8, device="cuda")
    with pytest.raises(L.AmpnetError, match="workspace"):
        L.seg_head_backward_f32(x, params, i["eps"], _t(i["dlogp"]), None, grads, big[:-1])
    with pytest.raises(L.AmpnetError, match="dlogp"):
        L.seg_head_backward_f32(x, params, i["eps"], _t(i["dlogp"][:69]), None, grads, big)
    with pytest.raises(L.AmpnetError, match="dx"):
        L.seg_head_backward_f32(x, params, i["eps"], _t(i["dlogp"]), torch.zeros((70, 15), device="cuda"), grads, big)
    with pytest.raises(L.AmpnetError, match="grads"):
        L.seg_head_backward_f32(x, params, i["eps"], _t(i["dlogp"]), None, grads[:5], big)
