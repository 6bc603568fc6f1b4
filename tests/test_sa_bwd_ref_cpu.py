"""The yardstick of the set-abstraction backward test checked without a GPU: tests/sa_bwd_ref.py, fed its own float64 argmax, against
torch float64 autograd of the composition (gather, 1x1 conv, eval BatchNorm, ReLU, max); every seeded case settles; check_argmax refuses
a wrong row."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import sa_bwd_ref as R                             # noqa: E402


def _torch_grads(i):
    """float64 autograd of the composition on case inputs i -> {name: numpy}."""
    d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    xyz, idx, cen = d(i["xyz"]), torch.from_numpy(i["group_idx"].astype(np.int64)), torch.from_numpy(i["centres"].astype(np.int64))
    feats = None if i["feats"] is None else d(i["feats"]).requires_grad_(True)
    B = xyz.shape[0]
    rows = torch.stack([xyz[c][idx[c]] - xyz[c][cen[c]][:, None, :] for c in range(B)])
    if feats is not None:
        rows = torch.cat([rows, torch.stack([feats[c][idx[c]] for c in range(B)])], -1)
    params, x = [], rows
    for layer, e in zip(i["layers"], i["eps"]):
        W, b, gamma, beta = (d(t).requires_grad_(True) for t in layer[:4])
        mean, var = d(layer[4]), d(layer[5])
        params.append((W, b, gamma, beta))
        z = x @ W.T + b
        x = torch.relu((z - mean) / torch.sqrt(var + float(np.float32(e))) * gamma + beta)
    out = x.max(2).values                           # ties are bit-identical repeated slots of one source point: any split sums the same
    (out * d(i["dout"])).sum().backward()
    res = {} if feats is None else {"dfeats": feats.grad.numpy()}
    for l, p in enumerate(params):
        res.update({f"{k}{l}": t.grad.numpy() for k, t in zip(("dW", "dbias", "dgamma", "dbeta"), p)})
    return res


@pytest.mark.parametrize("name", ["tail_group", "no_feats", "sparse_ball"])
def test_restatement_agrees_with_float64_autograd(name):
    i = R.case_inputs(sub("synthetic"), name)
    tape, worst = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    assert worst > R.RELU_MARGIN
    arg = R.float64_argmax(tape, i["group_idx"])
    R.check_argmax(arg, tape, i["group_idx"])
    got = R.sa_backward(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"], i["dout"], arg, tape)
    want = _torch_grads(i)
    assert sorted(got) == sorted(want) == sorted(R.output_names(len(i["layers"]), i["feats"] is not None))
    for k, (v, bar) in got.items():
        assert v.shape == want[k].shape and bar.shape == v.shape and (bar >= 0).all(), k
        assert np.abs(v - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
        assert np.abs(want[k]).max() > 0, k
    if i["feats"] is not None:
        for c, u in enumerate(i["unpicked"]):
            assert (got["dfeats"][0][c, u] == 0).all() and (got["dfeats"][1][c, u] == 0).all()


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_every_case_settles(name):
    i = R.case_inputs(sub("synthetic"), name)       # (settle_betas and the case's own assertions run inside)
    _, worst = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    assert worst > R.RELU_MARGIN


def test_check_argmax_rejects_a_wrong_row():
    i = R.case_inputs(sub("synthetic"), "tail_group")
    tape, _ = R.forward_tape(i["xyz"], i["centres"], i["group_idx"], i["feats"], i["layers"], i["eps"])
    arg = R.float64_argmax(tape, i["group_idx"])
    R.check_argmax(arg, tape, i["group_idx"])
    B, s, nsample = i["group_idx"].shape
    v = np.maximum(tape[-1][5], 0.0).reshape(B, s, nsample, -1)
    # a row that is far from the maximum
    g, c = np.unravel_index(np.argmax((v.max(2) - v.min(2)).reshape(-1)), (B * s, v.shape[-1]))
    bad = arg.copy().reshape(B * s, -1)
    bad[g, c] = v.reshape(B * s, nsample, -1)[g, :, c].argmin()
    with pytest.raises(AssertionError, match="not a maximum"):
        R.check_argmax(bad.reshape(arg.shape), tape, i["group_idx"])
    # a repeated slot of the winner: the same value, but not the first occurrence
    cnt = i["count"].reshape(-1)
    g = int(np.argmax(cnt < nsample))
    assert cnt[g] < nsample
    first_member = np.flatnonzero(arg.reshape(B * s, -1)[g] == 0)
    assert len(first_member), "no column of this group is won by the repeated member"
    dup = arg.copy().reshape(B * s, -1)
    dup[g, first_member[0]] = cnt[g]                # the first repeated slot holds member 0 again
    with pytest.raises(AssertionError, match="first occurrence"):
        R.check_argmax(dup.reshape(arg.shape), tape, i["group_idx"])
    out_of_range = arg.copy()
    out_of_range[0, 0, 0] = nsample
    with pytest.raises(AssertionError, match="nsample"):
        R.check_argmax(out_of_range, tape, i["group_idx"])
