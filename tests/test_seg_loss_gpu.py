"""The loss kernel behind the segmentation head on the GPU (csrc/seg_loss.hip: ampnet_seg_nll_forward_f32, ampnet_seg_nll_backward_f32)
against the float64 restatement of tests/seg_loss_ref.py, with the bars derived there: sums 1e-12 relative, loss 1 float32 ulp, dlogp 2
float32 ulp and exact zeros, predictions and counts exact, two runs the same bits.

confusion_device (ampnet_confusion_i64) is built for at most 8 classes, a limit this feature leaves alone: the counts are compared with
it at C = 2 and C = 5, and at C = 32 with the reference alone (which every case is compared with)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import seg_loss_ref as R                           # noqa: E402

pytestmark = pytest.mark.gpu

CONFUSION_MAX_CLASSES = 8


def _forward(L, logp, target, w):
    M, C = logp.shape
    dev = logp.device
    sums = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    preds = torch.full((M,), -7, dtype=torch.int64, device=dev)
    counts = torch.full((C * C + 1,), -7, dtype=torch.int64, device=dev)             # (the entry point zero-fills it)
    ws = torch.empty(L.seg_nll_forward_workspace_bytes(M), dtype=torch.uint8, device=dev)
    L.seg_nll_forward_f32(logp, target, w, sums, loss, preds, counts, ws)
    return sums, loss, preds, counts


def _backward(L, target, w, sums, M, C):
    g = torch.tensor([float(R.GRAD)], dtype=torch.float32, device=target.device)
    dlogp = torch.full((M, C), float("nan"), dtype=torch.float32, device=target.device)      # the kernel writes every element
    L.seg_nll_backward_f32(target, w, sums, g, dlogp)
    return dlogp


def _ulps(got32, ref64):
    """|got - ref| in float32 ulps of the reference value."""
    ref32 = np.asarray(ref64).astype(np.float32)
    return np.abs(np.asarray(got32, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", R.CLASSES)
@pytest.mark.parametrize("M", R.ROWS)
def test_kernels_against_the_float64_reference(M, C, weighted):
    L = sub("_lib")
    logp_h, target_h, w_h, ref = R.case(M, C, weighted)
    logp, target = torch.tensor(logp_h, device="cuda"), torch.tensor(target_h, device="cuda")      # (copies: the shared case stays read-only)
    w = None if w_h is None else torch.tensor(w_h, device="cuda")
    sums, loss, preds, counts = _forward(L, logp, target, w)
    sums_h, loss_h = sums.cpu().numpy(), float(loss.cpu()[0])
    rel = np.abs(sums_h - ref["sums"]) / ref["sums"]
    loss_ulps = float(_ulps(np.float32(loss_h), ref["loss"]))
    print(f"seg_nll M={M} C={C} weighted={weighted}: sums relative error {rel[0]:.2e} {rel[1]:.2e}, loss {loss_ulps:.2f} ulp")
    assert (rel <= 1e-12).all(), rel
    assert abs(loss_h - float(np.float32(ref["loss"]))) <= float(np.spacing(np.float32(abs(ref["loss"])))), (loss_h, ref["loss"])
    assert loss_h == float(np.float32(sums_h[0] / sums_h[1]))                        # loss IS (float)(sums[0] / sums[1])
    assert np.array_equal(preds.cpu().numpy(), ref["preds"])
    assert np.array_equal(counts.cpu().numpy(), ref["counts"])
    if C <= CONFUSION_MAX_CLASSES:
        conf = sub("utils.get_metrics").confusion_device(preds, target, C)
        assert torch.equal(counts, conf)
    # backward
    dlogp = _backward(L, target, w, sums, M, C)
    d_h = dlogp.cpu().numpy()
    want = R.nll_backward(target_h, w_h, ref["sums"][1], R.GRAD, C)
    hit = want != 0
    assert hit.sum() == ref["live"].sum()
    assert (d_h[~hit] == 0).all()                                                    # off-target and ignored rows: exact zeros
    worst = float(_ulps(d_h[hit], want[hit]).max())
    print(f"seg_nll M={M} C={C} weighted={weighted}: dlogp worst {worst:.2f} ulp")
    assert worst <= 2.0, worst
    # two runs: the same bits
    again = _forward(L, logp, target, w)
    for a, b in zip((sums, loss, preds, counts), again):
        assert torch.equal(a, b)
    assert torch.equal(dlogp, _backward(L, target, w, again[0], M, C))
    # preds and counts are optional
    sums2 = torch.empty_like(sums)
    loss2 = torch.empty_like(loss)
    L.seg_nll_forward_f32(logp, target, w, sums2, loss2, None, None,
                          torch.empty(L.seg_nll_forward_workspace_bytes(M), dtype=torch.uint8, device=logp.device))
    assert torch.equal(sums2, sums) and torch.equal(loss2, loss)


def test_every_row_ignored_is_nan_and_a_zero_gradient():
    L = sub("_lib")
    logp_h, _, w_h, _ = R.case(257, 5, True)
    logp, w = torch.tensor(logp_h, device="cuda"), torch.tensor(w_h, device="cuda")
    target = torch.full((257,), -1, dtype=torch.int64, device="cuda")
    sums, loss, preds, counts = _forward(L, logp, target, w)
    assert (sums == 0).all() and math.isnan(float(loss.cpu()[0]))
    assert np.array_equal(preds.cpu().numpy(), R.nll(logp_h, target.cpu().numpy(), w_h)["preds"])       # ignored rows still get a prediction
    assert int(counts[25]) == 257 and int(counts[:25].sum()) == 0
    assert (_backward(L, target, w, sums, 257, 5) == 0).all()


def test_refusals_come_before_any_launch():
    L = sub("_lib")
    logp = torch.zeros((4, 5), device="cuda")
    target = torch.zeros(4, dtype=torch.int64, device="cuda")
    sums, loss = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(1, device="cuda")
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.AmpnetError, match="classes must be in"):
        L.seg_nll_forward_f32(torch.zeros((4, 33), device="cuda"), target, None, sums, loss, None, None, ws)
    with pytest.raises(L.AmpnetError, match="workspace"):
        L.seg_nll_forward_f32(logp, target, None, sums, loss, None, None, ws[:8])
    with pytest.raises(L.AmpnetError, match="class_w"):
        L.seg_nll_forward_f32(logp, target, torch.ones(4, device="cuda"), sums, loss, None, None, ws)
    with pytest.raises(L.AmpnetError, match="target"):
        L.seg_nll_forward_f32(logp, target.int(), None, sums, loss, None, None, ws)
    with pytest.raises(L.AmpnetError, match="needs target"):
        L.seg_nll_backward_f32(target[:3], None, sums, loss, torch.empty((4, 5), device="cuda"))


def test_seg_nll_loss_builds_a_graph_to_a_leaf():
    """The public function: the gradient of 3 * loss reaches a leaf log_probs of shape [B, N, C] through autograd._SegNllFn, equal to the
    kernel's own backward; preds and counts carry no graph; without grad nothing does."""
    U = sub("pointNet.model.pointnet2_utils")
    L = sub("_lib")
    logp_h, target_h, w_h, ref = R.case(4099, 5, True)
    logp_h, target_h = logp_h[:4096].reshape(2, 2048, 5), target_h[:4096].reshape(2, 2048)
    leaf = torch.tensor(logp_h, device="cuda").requires_grad_(True)
    target, w = torch.tensor(target_h, device="cuda"), torch.tensor(w_h, device="cuda")
    loss, preds, counts = U.seg_nll_loss(leaf, target, w, want_preds=True, want_counts=True)
    assert loss.dim() == 0 and loss.requires_grad and preds.shape == (2, 2048) and not preds.requires_grad and not counts.requires_grad
    (3.0 * loss).backward()
    flat_ref = R.nll(logp_h.reshape(-1, 5), target_h.reshape(-1), w_h)
    want = R.nll_backward(target_h.reshape(-1), w_h, flat_ref["sums"][1], 3.0, 5)
    got = leaf.grad.cpu().numpy().reshape(-1, 5)
    hit = want != 0
    assert (got[~hit] == 0).all() and float(_ulps(got[hit], want[hit]).max()) <= 2.0
    assert np.array_equal(preds.cpu().numpy().reshape(-1), flat_ref["preds"]) and np.array_equal(counts.cpu().numpy(), flat_ref["counts"])
    assert abs(float(loss.detach().cpu()) - float(np.float32(flat_ref["loss"]))) <= float(np.spacing(np.float32(flat_ref["loss"])))
    # defaults: neither predictions nor counts; no graph without grad mode or without a tensor that asks for one
    plain, p, c = U.seg_nll_loss(leaf.detach(), target, w)
    assert p is None and c is None and not plain.requires_grad and torch.equal(plain, loss.detach())
    with torch.no_grad():
        assert not U.seg_nll_loss(leaf, target)[0].requires_grad
    unweighted, p2, _ = U.seg_nll_loss(leaf, target, None, want_preds=True)
    assert unweighted.requires_grad and torch.equal(p2, preds)
    with pytest.raises(L.AmpnetError, match="int64 target"):
        U.seg_nll_loss(leaf, target.int())
