"""The yardstick of tests/test_fp_backward_gpu.py checked without a GPU: the float64 restatement tests/fp_bwd_ref.py against torch.autograd
on a float64 torch composition of the layer, and the ReLU margin of every seeded case of the GPU test."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp_bwd_ref as R                             # noqa: E402

NAMES = [c[0] for c in R.CASES]


def torch_grads(i):
    """The gradients of sum(out * dout) of the usual composition -- gather, inverse-distance weights, cat, conv1d, eval BatchNorm, ReLU --
    in float64 by torch.autograd, under the names of fp_bwd_ref.output_names()."""
    t = lambda a, g=False: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(g)
    p1 = None if i["points1"] is None else t(i["points1"], True)
    p2 = t(i["points2"], True)
    idx = torch.from_numpy(np.asarray(i["idx"], dtype=np.int64))
    B = idx.shape[0]
    r = 1.0 / (t(i["dist2"]) + float(np.float32(1e-8)))
    w = r / r.sum(-1, keepdim=True)
    x = (p2[torch.arange(B)[:, None, None], idx] * w[..., None]).sum(2)                    # [B, n, D2]
    if p1 is not None:
        x = torch.cat([p1, x], -1)
    x = x.transpose(1, 2)                                                                 # [B, cin, n]
    params = []
    for (W, b, gamma, beta, mean, var), e in zip(i["layers"], i["eps"]):
        W, b, gamma, beta = t(W, True), t(b, True), t(gamma, True), t(beta, True)
        params.append((W, b, gamma, beta))
        x = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.conv1d(x, W[:, :, None], b), t(mean), t(var), gamma, beta, False,
                                                      0.0, float(np.float32(e))))
    (x.transpose(1, 2) * t(i["dout"])).sum().backward()
    out = {"dpoints2": p2.grad}
    if p1 is not None:
        out["dpoints1"] = p1.grad
    for l, (W, b, gamma, beta) in enumerate(params):
        out.update({f"dW{l}": W.grad, f"dbias{l}": b.grad, f"dgamma{l}": gamma.grad, f"dbeta{l}": beta.grad})
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["negative_gamma", "three_layers", "unpicked"])
def test_the_restatement_agrees_with_torch_autograd(synth, name):
    i = R.case_inputs(synth, name)
    got, _ = R.fp_backward(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])
    want = torch_grads(i)
    assert sorted(got) == sorted(want) == sorted(R.output_names(len(i["layers"]), i["points1"] is not None))
    for k, (v, bar) in got.items():
        assert v.shape == want[k].shape == bar.shape, k
        assert np.abs(v - want[k]).max() <= 1e-10 * np.abs(want[k]).max(), k
        assert (bar >= 0).all() and np.isfinite(bar).all(), k
    for c, u in enumerate(i["unpicked"]):                    # nobody's neighbour: value 0 and bar 0, exactly
        assert (got["dpoints2"][0][c, u] == 0).all() and (got["dpoints2"][1][c, u] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_every_gpu_case_keeps_the_relu_margin(synth, name):
    i = R.case_inputs(synth, name)
    assert all(a.dtype == np.float32 for layer in i["layers"] for a in layer)
    _, worst = R.fp_backward(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])      # asserts the margin
    assert worst > R.RELU_MARGIN
    if name == "negative_gamma":
        g = [layer[2] for layer in i["layers"]]
        assert all((v < 0).any() and (v > 0).any() for v in g) and sum(int((v == 0).sum()) for v in g) == 1
    if name == "unpicked":
        assert all(len(u) >= 2 for u in i["unpicked"])
    k = min(3, i["points2"].shape[1])
    assert i["idx"].shape == i["dist2"].shape == (2, i["dout"].shape[1], k)


def test_the_margin_assertion_fires():
    """A ReLU input put on zero is refused, not compared."""
    layers = R.make_layers(3, 4, [32])
    layers[0][3][:] = 0.0
    layers[0][1][:] = layers[0][4]                            # b = mean, beta = 0 and a zero row: y = 0
    z = np.zeros((1, 2, 4), np.float32)
    with pytest.raises(AssertionError, match="ReLU"):
        R.fp_backward(None, z, np.zeros((1, 2, 1), np.int32), np.zeros((1, 2, 1), np.float32), layers, [R.BN_EPS], np.ones((1, 2, 32), np.float32))
