"""The yardsticks of tests/test_sa_train_gpu.py checked without a GPU: the float64 restatement tests/sa_train_ref.py against torch's
float64 autograd over the plain composition (gather, Conv2d with bias, BatchNorm2d in train mode with momentum 0.1, ReLU, the max with
its gradient routed to `arg`), the cases' own assertions, three deliberate mistakes that the comparison has to catch, and the layer-local
checker run on a float32 numpy emulation of the path: its cap on undecided ReLU inputs holds for every case, and it catches a mistake."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sa_train_ref as R                           # noqa: E402

NAMES = [c[0] for c in R.CASES]
LOCAL = [c[0] for c in R.LOCAL]


def torch_train(i, arg, arg_is_max=True):
    """Outputs, updated running statistics, saved statistics and the gradients of sum(out * dout) of the usual composition in float64,
    under sa_train_ref's names.  The max takes row `arg` of every (group, column): its value is the max's and its gradient goes there."""
    t = lambda a, g=False: torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(g)
    xyz, idx, cen = t(i["xyz"]), torch.from_numpy(i["group_idx"].astype(np.int64)), torch.from_numpy(i["centres"].astype(np.int64))
    feats = None if i["feats"] is None else t(i["feats"], True)
    B = xyz.shape[0]
    rows = torch.stack([xyz[c][idx[c]] - xyz[c][cen[c]][:, None, :] for c in range(B)])              # [B, s, nsample, 3]
    if feats is not None:
        rows = torch.cat([rows, torch.stack([feats[c][idx[c]] for c in range(B)])], -1)
    x = rows.permute(0, 3, 2, 1)                                                                     # [B, C, nsample, npoint]
    params, out = [], {}
    for l, ((W, b, gamma, beta, mean, var), e) in enumerate(zip(i["layers"], i["eps"])):
        W, b, gamma, beta, rm, rv = t(W, True), t(b, True), t(gamma, True), t(beta, True), t(mean), t(var)
        params.append((W, b, gamma, beta))
        z = torch.nn.functional.conv2d(x, W[:, :, None, None], b)
        with torch.no_grad():
            a = z - b[None, :, None, None]
            out[f"save_mean{l}"] = a.mean((0, 2, 3))
            out[f"save_invstd{l}"] = 1.0 / torch.sqrt(a.var((0, 2, 3), unbiased=False) + float(np.float32(e)))
        x = torch.relu(torch.nn.functional.batch_norm(z, rm, rv, gamma, beta, True, float(np.float32(R.MOMENTUM)), float(np.float32(e))))
        out[f"running_mean{l}"], out[f"running_var{l}"] = rm, rv
    x = x.permute(0, 3, 2, 1)                                                                        # [B, s, nsample, C]
    picked = torch.gather(x, 2, torch.from_numpy(arg.astype(np.int64))[:, :, None, :])[:, :, 0]
    assert not arg_is_max or (x.max(2).values - picked).abs().max() <= 1e-12             # (a repeated slot may round an ulp off its first member's row)
    out["out"] = picked.detach()
    (picked * t(i["dout"])).sum().backward()
    if feats is not None:
        out["dfeats"] = feats.grad
    for l, (W, b, gamma, beta) in enumerate(params):
        out.update({f"dW{l}": W.grad, f"dbias{l}": b.grad, f"dgamma{l}": gamma.grad, f"dbeta{l}": beta.grad})
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    import conftest
    return R.case_inputs(conftest.sub("synthetic"), name)


def _restated(i, mutate=None):
    tape, worst = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], mutate=mutate,
                                 margin=R.RELU_MARGIN if mutate is None else -1.0)          # (the betas were settled for the unmutated path)
    arg = R.float64_argmax(tape, i["group_idx"])
    R.check_argmax(arg, tape[-1], i["group_idx"])
    return R.sa_train(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape, mutate=mutate), arg, worst


def _disagreements(got, want, layers):
    """The outputs whose restated value is off torch's by more than 1e-9 relative + 1e-12 absolute.  dbias is zero up to torch's own
    float64 rounding of a cancelling sum whose every term carries the factor |gamma| invstd: its absolute bound is 1e-12 times the
    largest such factor of the layer (30 in no_feats, whose three input columns are small coordinate differences)."""
    def floor(k):
        if not k.startswith("dbias"):
            return 1e-12
        l = int(k[5:])
        return 1e-12 * max(1.0, float((np.abs(np.float64(layers[l][2])) * got[f"save_invstd{l}"][0]).max()))
    return [k for k, (v, _) in got.items() if not np.abs(v - want[k]).max() <= 1e-9 * np.abs(want[k]).max() + floor(k)]


@pytest.mark.parametrize("name", NAMES)
def test_every_case_keeps_the_margin_and_agrees_with_torch(name):
    i = _inputs(name)                                        # (the case's own assertions run inside: counts, repeated slots, unpicked)
    assert all(a.dtype == np.float32 for layer in i["layers"] for a in layer)
    got, arg, worst = _restated(i)                           # asserts the margin
    assert worst > R.RELU_MARGIN
    want = torch_train(i, arg)
    assert sorted(got) == sorted(want) == sorted(R.output_names(len(i["layers"]), i["feats"] is not None))
    for k, (v, bar) in got.items():
        assert v.shape == want[k].shape == bar.shape, k
        assert (bar >= 0).all() and np.isfinite(bar).all() and np.isfinite(v).all(), k
    assert _disagreements(got, want, i["layers"]) == []
    if i["feats"] is not None:
        for c, u in enumerate(i["unpicked"]):                # in no group: value 0 and bar 0, exactly
            assert (got["dfeats"][0][c, u] == 0).all() and (got["dfeats"][1][c, u] == 0).all()
    for l in range(len(i["layers"])):
        assert (got[f"dbias{l}"][0] == 0).all() and (got[f"dbias{l}"][1] == 0).all()
    if name == "negative_gamma":
        g = [layer[2] for layer in i["layers"]]
        assert all((v < 0).any() and (v > 0).any() for v in g) and sum(int((v == 0).sum()) for v in g) == 1
    if name == "dead_channel":
        assert got["save_invstd0"][0][i["dead_row"]] == 1.0 / np.sqrt(np.float64(np.float32(R.BN_EPS)))
    if name == "many_groups":
        assert i["group_idx"].shape[0] * i["group_idx"].shape[1] > 2048
    if name in ("tail_group", "two_tiles", "sparse_ball"):   # the repeated slots get a gradient of their own: dz is dense
        f = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])[0][-1]
        r = R.backward_layer(f, R.select_dout(arg, i["dout"], i["nsample"]), np.zeros_like(f["y"]))
        repeated = (np.arange(i["nsample"])[None, None, :] >= i["count"][:, :, None]).reshape(-1)
        assert repeated.any() and (r["dz"][repeated] != 0).mean() > 0.9


@pytest.mark.parametrize("mutate, case, hit", [("biased", "tail_group", "running_var"), ("no_xhat", "tail_group", "dW"),
                                               ("distinct", "sparse_ball", "save_mean")])
def test_the_comparison_with_torch_bites(mutate, case, hit):
    """The biased variance in running_var, dz without its x^ dgamma / M term, or statistics over the distinct members only (the repeated
    slots left out) do not pass."""
    i = _inputs(case)
    got, arg, _ = _restated(i, mutate)
    bad = _disagreements(got, torch_train(i, arg, arg_is_max=False), i["layers"])   # (arg: the mutated path's)
    assert any(k.startswith(hit) for k in bad), bad


def test_the_margin_assertion_fires():
    """A ReLU input put on zero is refused, not compared: gamma = 0 and beta = 0 give y = 0 in every row."""
    i = dict(_inputs("no_feats"))
    layers = [tuple(a.copy() for a in layer) for layer in i["layers"]]
    layers[0][2][:] = 0.0
    layers[0][3][:] = 0.0
    with pytest.raises(AssertionError, match="ReLU"):
        R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], layers, i["eps"])


@pytest.mark.parametrize("name", LOCAL)
def test_layer_local_checker_on_the_float32_emulation(name):
    """check_layers on a float32 numpy emulation of the path: at most 1e-3 of a layer's ReLU inputs are undecided (asserted inside), and
    every layer-local comparison holds."""
    i = _inputs(name)
    ratios = R.check_layers(i, R.emulate_f32(i))
    print(f"sa_train local (float32 emulation) {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    L = len(i["layers"])
    want = {"out", "dfeats"} | {f"{k}{l}" for l in range(L) for k in ("save_mean", "save_invstd", "running_mean", "running_var", "dW", "dgamma",
                                                                      "dbeta", "dz", "undecided")} | {f"x{l}" for l in range(1, L)}
    assert set(ratios) == want
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


def test_layer_local_checker_bites():
    """The checker refuses a dz without its x^ dgamma / M term, a dW of the wrong rows and statistics over the distinct members only."""
    i = _inputs("negative_gamma3")
    good = R.emulate_f32(i)
    bad = dict(good)
    f32 = np.float32
    M = good["x1"].shape[0]
    a = good["x1"][:, :i["layers"][1][0].shape[1]] @ i["layers"][1][0].T
    mu, inv = good["save_mean1"], good["save_invstd1"]
    bad["dz1"] = (good["dz1"] + i["layers"][1][2] * inv * (a - mu) * (good["dgamma1"] * inv / f32(M))).astype(f32)      # the term taken back out
    assert R.check_layers(i, bad)["dz1"] > 1.0
    bad = dict(good)
    bad["dW0"] = (good["dz0"][1:].T @ good["x0"][:-1]).astype(f32)
    assert R.check_layers(i, bad)["dW0"] > 1.0
    bad = dict(good)
    first = (np.arange(i["nsample"])[None, None, :] < i["count"][:, :, None]).reshape(-1)
    assert not first.all()
    a0 = good["x0"] @ i["layers"][0][0].T
    bad["save_mean0"] = a0[first].mean(0, dtype=f32)
    assert R.check_layers(i, bad)["save_mean0"] > 1.0
