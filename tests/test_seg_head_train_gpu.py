"""The train-mode segmentation head of the C ABI (include/ampnet_hip.h: ampnet_seg_head_train_forward_f32,
ampnet_seg_head_train_backward_f32) against the float64 restatement tests/seg_head_train_ref.py on its seeded cases.  The bars are derived in
that module's docstring; the worst error / bar ratio of every output of every case is printed.  A wrong keep bit moves a logit by about
|W2| |h| dscale, orders of magnitude above the bar (tests/test_seg_head_train_ref_cpu.py flips one), so the bars also pin the mask."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import seg_head_train_ref as R                     # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -1234.5
DEV = "cuda"
ALL = R.FORWARD + R.BACKWARD


def _case(name):
    return R.reference(sub("synthetic"), name)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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


def _run(L, i, prefill=float("nan"), want_dx=True, momentum=R.MOMENTUM):
    """Forward and backward of a case from its numpy inputs, fresh running statistics -> {seg_head_train_ref name: numpy array}."""
    x, dlogp = _t(i["x"]), _t(i["dlogp"])
    params = [_t(p) for p in i["params"]]
    M, cin = x.shape
    hidden, C = params[0].shape[0], params[6].shape[0]
    o = _Outs(prefill)
    res = {"logp": o.new("logp", (M, C)), "save_mean": o.new("save_mean", (hidden,)), "save_invstd": o.new("save_invstd", (hidden,))}
    ws = torch.full((L.seg_head_train_forward_workspace_bytes(cin, hidden, C, M),), 0xAB, dtype=torch.uint8, device=DEV)
    L.seg_head_train_forward_f32(x, params, i["eps"], momentum, i["p"], i["drop_seed"], res["logp"], res["save_mean"], res["save_invstd"], ws)
    res["running_mean"], res["running_var"] = params[4], params[5]
    if want_dx:
        res["dx"] = o.new("dx", (M, cin))
    names = ("dW1", "db1", "dgamma", "dbeta", "dW2", "db2")
    grads = [o.new(k, params[q].shape) for k, q in zip(names, (0, 1, 1, 1, 6, 7))]
    res.update(dict(zip(names, grads)))
    bws = torch.full((L.seg_head_train_backward_workspace_bytes(cin, hidden, C, M),), 0xAB, dtype=torch.uint8, device=DEV)
    # (the backward reads neither running statistic: hand it NaNs there)
    bparams = params[:4] + [torch.full_like(params[4], float("nan")), torch.full_like(params[5], float("nan"))] + params[6:]
    L.seg_head_train_backward_f32(x, bparams, i["eps"], i["p"], i["drop_seed"], res["save_mean"], res["save_invstd"], dlogp, res.get("dx"),
                                  grads, bws)
    o.check()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", R.NAMES)
def test_seg_head_train_within_the_derived_bar(name):
    L = sub("_lib")
    i, want, _ = _case(name)
    got = _run(L, i)                                               # every output starts as NaN: every element must be written
    assert sorted(got) == sorted(ALL)
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
    for k in ALL:
        v, bar = want[k]
        assert got[k].shape == v.shape, (name, k)
        err = np.abs(got[k].astype(np.float64) - v)
        ratios[k] = float(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0).max())     # (0 / 0: an exact value met exactly)
    print(f"seg_head_train {name}: worst error / bar " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    assert (got["db1"] == 0).all(), name                           # the bias has no effect on a batch-normalised output
    assert not np.array_equal(got["running_mean"], i["params"][4]) and not np.array_equal(got["running_var"], i["params"][5])
    if name == "negative_gamma":
        for k, v in got.items():
            assert k == "db1" or (v != 0).mean() > 0.2, (k, float((v != 0).mean()))       # the ReLU and the mask did not wipe the case out
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


@pytest.mark.parametrize("name", ["tail", "odd_cin"])
def test_dx_is_optional_and_changes_nothing_else(name):
    L = sub("_lib")
    i, _, _ = _case(name)
    full, lean = _run(L, i), _run(L, i, want_dx=False)
    assert "dx" not in lean
    for k in lean:
        assert np.array_equal(full[k], lean[k]), (name, k)


def _eval_bits(L, i):
    """The eval entry points on a case's inputs -> their outputs as numpy arrays."""
    x, dlogp = _t(i["x"]), _t(i["dlogp"])
    params = [_t(p) for p in i["params"]]
    M, cin = x.shape
    hidden, C = params[0].shape[0], params[6].shape[0]
    logp = torch.full((M, C), float("nan"), device=DEV)
    preds = torch.full((M,), -1, dtype=torch.int64, device=DEV)
    L.seg_head_forward_f32(x, params, i["eps"], logp, preds, torch.empty(L.seg_head_forward_workspace_bytes(cin, hidden, C, M), dtype=torch.uint8,
                                                                         device=DEV))
    dx = torch.full((M, cin), float("nan"), device=DEV)
    grads = [torch.full_like(params[q], float("nan")) for q in (0, 1, 1, 1, 6, 7)]
    L.seg_head_backward_f32(x, params, i["eps"], dlogp, dx, grads, torch.empty(L.seg_head_backward_workspace_bytes(cin, hidden, C, M),
                                                                              dtype=torch.uint8, device=DEV))
    return [t.cpu().numpy() for t in [logp, preds, dx] + grads]


@pytest.mark.parametrize("name", ["tail", "no_drop"])
def test_the_train_path_leaves_no_state_behind(name):
    """The eval entry points give the same bits before and after a train call on the same inputs."""
    L = sub("_lib")
    i, _, _ = _case(name)
    before = _eval_bits(L, i)
    _run(L, i)
    after = _eval_bits(L, i)
    for a, b in zip(before, after):
        assert np.isfinite(a.astype(np.float64)).all() and np.array_equal(a, b), name


def test_the_seed_selects_the_mask():
    L = sub("_lib")
    i, _, _ = _case("tail")
    a, b = _run(L, i), _run(L, dict(i, drop_seed=i["drop_seed"] + 1))
    assert not np.array_equal(a["logp"], b["logp"]) and not np.array_equal(a["dW2"], b["dW2"])
    for k in ("save_mean", "save_invstd", "running_mean", "running_var"):
        assert np.array_equal(a[k], b[k]), k                       # the statistics are taken in front of the dropout


def test_refusals_through_the_wrappers():
    L = sub("_lib")
    i, _, _ = _case("negative_gamma")                              # 70 rows, 16 -> 64 -> 5
    for bad, says in ((dict(p=1.0), "drop_p=1"), (dict(p=-0.5), "drop_p=-0.5"), (dict(p=float("nan")), "drop_p=")):
        with pytest.raises(L.AmpnetError, match=says):
            _run(L, dict(i, **bad))
    for m in (-0.1, 1.5, float("nan")):
        with pytest.raises(L.AmpnetError, match="momentum"):
            _run(L, i, momentum=m)
    with pytest.raises(L.AmpnetError, match="momentum=None"):
        _run(L, i, momentum=None)
    one = dict(i, x=i["x"][:1], dlogp=i["dlogp"][:1])
    with pytest.raises(L.AmpnetError, match=">= 2 rows"):
        _run(L, one)
    x, params = _t(i["x"]), [_t(p) for p in i["params"]]
    logp, sm, si = torch.zeros((70, 5), device=DEV), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    ws = torch.zeros(L.seg_head_train_forward_workspace_bytes(16, 64, 5, 70), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.AmpnetError, match="workspace"):
        L.seg_head_train_forward_f32(x, params, i["eps"], 0.1, 0.5, 1, logp, sm, si, ws[:-1])
    with pytest.raises(L.AmpnetError, match="save_mean"):
        L.seg_head_train_forward_f32(x, params, i["eps"], 0.1, 0.5, 1, logp, sm[:63].contiguous(), si, ws)
    with pytest.raises(L.AmpnetError, match="save_mean is None"):
        L.seg_head_train_forward_f32(x, params, i["eps"], 0.1, 0.5, 1, logp, None, si, ws)
    grads = [torch.zeros_like(params[q]) for q in (0, 1, 1, 1, 6, 7)]
    bws = torch.zeros(L.seg_head_train_backward_workspace_bytes(16, 64, 5, 70), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.AmpnetError, match="workspace"):
        L.seg_head_train_backward_f32(x, params, i["eps"], 0.5, 1, sm, si, _t(i["dlogp"]), None, grads, bws[:-1])
    with pytest.raises(L.AmpnetError, match="dlogp"):
        L.seg_head_train_backward_f32(x, params, i["eps"], 0.5, 1, sm, si, _t(i["dlogp"][:69]), None, grads, bws)
    with pytest.raises(L.AmpnetError, match="grads"):
        L.seg_head_train_backward_f32(x, params, i["eps"], 0.5, 1, sm, si, _t(i["dlogp"]), None, grads[:5], bws)
    assert torch.equal(params[4], _t(i["params"][4]))              # nothing above touched the statistics
