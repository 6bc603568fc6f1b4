"""The yardstick of tests/test_fp_train_gpu.py checked without a GPU: the float64 restatement tests/fp_train_ref.py against torch's float64
autograd over the usual composition with train-mode BatchNorm (conv bias present, momentum 0.1), the ReLU margin of every seeded case, and
two deliberate mistakes that the comparison has to catch."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp_train_ref as R                           # noqa: E402

NAMES = [c[0] for c in R.CASES]


def torch_train(i):
    """Outputs, updated running statistics, saved statistics and the gradients of sum(out * dout) of the usual composition -- gather,
    inverse-distance weights, cat, conv1d with bias, F.batch_norm(training=True), ReLU -- in float64, under fp_train_ref's names."""
    t = lambda a, g=False: torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(g)
    p1 = None if i["points1"] is None else t(i["points1"], True)
    p2 = t(i["points2"], True)
    idx = torch.from_numpy(np.asarray(i["idx"], dtype=np.int64))
    B = idx.shape[0]
    r = 1.0 / (t(i["dist2"]) + float(np.float32(1e-8)))
    w = r / r.sum(-1, keepdim=True)
    x = (p2[torch.arange(B)[:, None, None], idx] * w[..., None]).sum(2)
    if p1 is not None:
        x = torch.cat([p1, x], -1)
    x = x.transpose(1, 2)
    params, out = [], {}
    for l, ((W, b, gamma, beta, mean, var), e) in enumerate(zip(i["layers"], i["eps"])):
        W, b, gamma, beta, rm, rv = t(W, True), t(b, True), t(gamma, True), t(beta, True), t(mean), t(var)
        params.append((W, b, gamma, beta))
        z = torch.nn.functional.conv1d(x, W[:, :, None], b)
        with torch.no_grad():
            a = z - b[None, :, None]
            out[f"save_mean{l}"] = a.mean((0, 2))
            out[f"save_invstd{l}"] = 1.0 / torch.sqrt(a.var((0, 2), unbiased=False) + float(np.float32(e)))
        x = torch.relu(torch.nn.functional.batch_norm(z, rm, rv, gamma, beta, True, float(np.float32(R.MOMENTUM)), float(np.float32(e))))
        out[f"running_mean{l}"], out[f"running_var{l}"] = rm, rv
    out["out"] = x.transpose(1, 2).detach()
    (x.transpose(1, 2) * t(i["dout"])).sum().backward()
    out["dpoints2"] = p2.grad
    if p1 is not None:
        out["dpoints1"] = p1.grad
    for l, (W, b, gamma, beta) in enumerate(params):
        out.update({f"dW{l}": W.grad, f"dbias{l}": b.grad, f"dgamma{l}": gamma.grad, f"dbeta{l}": beta.grad})
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    import conftest
    return R.case_inputs(conftest.sub("synthetic"), name)


def _disagreements(got, want):
    """The outputs whose restated value is off torch's by more than 1e-9 relative (+ 1e-12 absolute: dbias is zero up to torch's own
    float64 rounding)."""
    return [k for k, (v, _) in got.items() if not np.abs(v - want[k]).max() <= 1e-9 * np.abs(want[k]).max() + 1e-12]


@pytest.mark.parametrize("name", NAMES)
def test_every_case_keeps_the_margin_and_agrees_with_torch(name):
    i = _inputs(name)
    assert all(a.dtype == np.float32 for layer in i["layers"] for a in layer)
    got, worst = R.fp_train(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"])      # asserts the margin
    assert worst > R.RELU_MARGIN
    want = torch_train(i)
    assert sorted(got) == sorted(want) == sorted(R.output_names(len(i["layers"]), i["points1"] is not None))
    for k, (v, bar) in got.items():
        assert v.shape == want[k].shape == bar.shape, k
        assert (bar >= 0).all() and np.isfinite(bar).all() and np.isfinite(v).all(), k
    assert _disagreements(got, want) == []
    for c, u in enumerate(i["unpicked"]):                    # nobody's neighbour: value 0 and bar 0, exactly
        assert (got["dpoints2"][0][c, u] == 0).all() and (got["dpoints2"][1][c, u] == 0).all()
    for l in range(len(i["layers"])):
        assert (got[f"dbias{l}"][0] == 0).all() and (got[f"dbias{l}"][1] == 0).all()
    if name == "negative_gamma":
        g = [layer[2] for layer in i["layers"]]
        assert all((v < 0).any() and (v > 0).any() for v in g) and sum(int((v == 0).sum()) for v in g) == 1
    if name == "unpicked":
        assert all(len(u) >= 2 for u in i["unpicked"])
    if name == "offset":
        mu, inv = got["save_mean0"][0], got["save_invstd0"][0]
        assert np.median(np.abs(mu) * inv) > 10.0            # |mu| an order of magnitude above the spread
    if name == "dead_channel":
        assert got["save_invstd0"][0][R.DEAD_ROW] == 1.0 / np.sqrt(np.float64(np.float32(R.BN_EPS)))
    if name == "many_tiles":
        assert i["idx"].shape[0] * ((i["idx"].shape[1] + 31) // 32) > 1024


@pytest.mark.parametrize("mutate, hit", [("biased", "running_var"), ("no_xhat", "dW")])
def test_the_comparison_with_torch_bites(mutate, hit):
    """The biased variance in running_var, or dz without its x^ dgamma / M term, does not pass."""
    i = _inputs("tail_tile")
    got, _ = R.fp_train(i["points1"], i["points2"], i["idx"], i["dist2"], i["layers"], i["eps"], i["dout"], mutate=mutate)
    bad = _disagreements(got, torch_train(i))
    assert any(k.startswith(hit) for k in bad), bad


def test_the_margin_assertion_fires():
    """A ReLU input put on zero is refused, not compared: gamma = 0 and beta = 0 give y = 0 in every row."""
    layers = R.make_layers(3, 4, [32])
    layers[0][2][:] = 0.0
    layers[0][3][:] = 0.0
    p2 = np.arange(8, dtype=np.float32).reshape(1, 2, 4)
    idx = np.arange(2, dtype=np.int32).reshape(1, 2, 1)
    with pytest.raises(AssertionError, match="ReLU"):
        R.fp_train(None, p2, idx, np.zeros((1, 2, 1), np.float32), layers, [R.BN_EPS], np.ones((1, 2, 32), np.float32))
