"""PointNetSegHead and pointnet_2_seg on the GPU: the module against the C ABI (bit for bit) and against torch (a strict state_dict
exchange, autograd of the float32 composition, loosely), the graph rules, and the model end to end."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_finetune_util as PU                     # noqa: E402
import seg_head_ref as R                           # noqa: E402

pytestmark = pytest.mark.gpu

B, N = 2, 35                                       # 70 rows: the `tail` case of seg_head_ref (128 -> 128 -> 5, betas settled) as two clouds


def _torch_head(cin, hidden, classes):
    m = torch.nn.Module()
    m.conv1, m.bn1, m.drop1, m.conv2 = (torch.nn.Conv1d(cin, hidden, 1), torch.nn.BatchNorm1d(hidden), torch.nn.Dropout(0.5),
                                        torch.nn.Conv1d(hidden, classes, 1))
    m.forward = lambda p: torch.log_softmax(m.conv2(m.drop1(torch.relu(m.bn1(m.conv1(p))))), dim=1).permute(0, 2, 1)
    return m.cuda().eval()


def _head(grad, synth):
    """(a PointNetSegHead with the `tail` case's parameters, its input [B, 128, N], the case)."""
    U = sub("pointNet.model.pointnet2_utils")
    i, _, _ = R.reference(synth, "tail")
    head = U.PointNetSegHead(128, 128, 5, grad=grad).eval()
    W1, b1, gamma, beta, mean, var, W2, b2 = (torch.from_numpy(p) for p in i["params"])
    head.load_state_dict({"conv1.weight": W1[:, :, None], "conv1.bias": b1, "bn1.weight": gamma, "bn1.bias": beta, "bn1.running_mean": mean,
                          "bn1.running_var": var, "bn1.num_batches_tracked": torch.tensor(3), "conv2.weight": W2[:, :, None], "conv2.bias": b2})
    points = torch.from_numpy(i["x"]).cuda().reshape(B, N, 128).transpose(1, 2).contiguous()
    return head, points, i


def test_module_forward_is_the_c_abi_bit_for_bit(synth):
    L = sub("_lib")
    head, points, i = _head(False, synth)
    out = head(points)
    assert out.shape == (B, N, 5) and out.dtype == torch.float32 and not out.requires_grad and out.grad_fn is None
    logp = torch.empty((B * N, 5), device="cuda")
    preds = torch.empty((B * N,), dtype=torch.int64, device="cuda")
    ws = torch.empty(L.seg_head_forward_workspace_bytes(128, 128, 5, B * N), dtype=torch.uint8, device="cuda")
    L.seg_head_forward_f32(torch.from_numpy(i["x"]).cuda(), [torch.from_numpy(p).cuda() for p in i["params"]], head.bn1.eps, logp, preds, ws)
    assert torch.equal(out.reshape(B * N, 5), logp)
    pred = head.predict(points)
    assert pred.shape == (B, N) and pred.dtype == torch.int64
    assert torch.equal(pred.reshape(-1), preds)
    assert np.array_equal(pred.cpu().numpy(), out.cpu().numpy().argmax(-1))
    assert torch.allclose(out.exp().sum(-1), torch.ones((B, N), device="cuda"), atol=1e-5)
    with pytest.raises(sub("_lib").AmpnetError, match="points"):
        head(points[:, :127].contiguous())
    with pytest.raises(sub("_lib").AmpnetError, match="GPU"):
        head(points.cpu())


def test_no_graph_unless_asked_and_train_mode_raises(synth):
    plain, points, _ = _head(False, synth)
    twin, _, _ = _head(True, synth)
    req = points.clone().requires_grad_(True)
    assert plain(req).grad_fn is None                                # grad=False: no graph, ever
    out = twin(req)
    assert out.requires_grad and torch.equal(out.detach(), plain(points))
    with torch.no_grad():
        assert not twin(req).requires_grad                           # grad mode off
    for p in twin.parameters():
        p.requires_grad_(False)
    assert not twin(points).requires_grad                            # nothing requires grad
    assert twin(req).requires_grad                                   # the input does
    assert not twin.predict(req).requires_grad
    with pytest.raises(NotImplementedError, match="eval mode"):
        twin.train()(points)
    with pytest.raises(NotImplementedError, match="eval mode"):
        plain.train().predict(points)
    assert torch.equal(plain.eval()(points), out.detach())            # back in eval mode: as before


def test_gradients_against_torch_autograd(synth):
    """The float32 torch composition on the same tensors, loosely (rtol 1e-3 of each gradient's scale: torch sums in other orders); the
    tight check is tests/test_seg_head_gpu.py."""
    head, points, i = _head(True, synth)
    ref = _torch_head(128, 128, 5)
    ref.load_state_dict(head.state_dict(), strict=True)              # our state into a torch head, strictly ...
    back = sub("pointNet.model.pointnet2_utils").PointNetSegHead(128, 128, 5).eval()
    back.load_state_dict(ref.state_dict(), strict=True)              # ... and a torch head's state into ours
    assert list(back.state_dict()) == list(ref.state_dict())
    assert all(torch.equal(v, head.state_dict()[k]) for k, v in back.state_dict().items())
    assert torch.equal(back(points), head(points).detach())
    g = torch.from_numpy(i["dlogp"]).cuda().reshape(B, N, 5)
    a, b = points.clone().requires_grad_(True), points.clone().requires_grad_(True)
    out, want = head(a), ref.forward(b)
    assert torch.allclose(out, want, rtol=1e-3, atol=1e-4)
    (out * g).sum().backward()
    (want * g).sum().backward()
    pairs = [("points", a.grad, b.grad)] + [(k, p.grad, dict(ref.named_parameters())[k].grad) for k, p in head.named_parameters()]
    assert sorted(k for k, _, _ in pairs[1:]) == sorted(["conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "conv2.weight", "conv2.bias"])
    for k, got, exp in pairs:
        assert got is not None and got.shape == exp.shape, k
        err, scale = float((got - exp).abs().max()), float(exp.abs().max())
        print(f"seg_head module gradient {k}: max |difference| / max |torch| = {err / scale:.2e}")
        assert err <= 1e-3 * scale, (k, err, scale)
    for k, v in head.named_buffers():
        assert torch.equal(v, back.state_dict()[k]), k                # running statistics and the counter: untouched


def test_one_sgd_step_changes_the_output(synth):
    head, points, i = _head(True, synth)
    target = torch.from_numpy(sub("synthetic").randint(77, (B * N,), 0, 5)).cuda()
    opt = torch.optim.SGD(head.parameters(), lr=0.01)
    before = head(points)
    loss = F.nll_loss(before.reshape(-1, 5), target)
    loss.backward()
    opt.step()
    after = head(points)
    assert not torch.equal(after.detach(), before.detach())
    assert float(F.nll_loss(after.detach().reshape(-1, 5), target)) < float(loss.detach())


def _seg_model(synth, state=None, **kwargs):
    """pointnet_2_seg(5) in eval mode at the reduced sizes of pn2_finetune_util.model (128 / 32 / 8 centres), seeded."""
    A = sub("pointNet.model.pointnetAtt")
    net = A.pointnet_2_seg(5, **kwargs).eval()
    for sa, npoint, radius in ((net.sa1, 128, 0.2), (net.sa2, 32, 0.4), (net.sa3, 8, 0.8)):
        sa.npoint, sa.radius = npoint, radius
    PU.randomise(net, 8)
    if state is not None:
        res = net.load_state_dict(state, strict=False)
        assert not res.unexpected_keys and sorted({k.split(".")[0] for k in res.missing_keys}) == ["bn1", "conv2"], res
    return net


def _model_input(synth, n=256):
    x = np.concatenate([synth.clouds(55, 2, n), synth.uniform(56, (2, n, 6), -1.0, 1.0)], -1)          # [2, n, 9]
    return torch.from_numpy(x).cuda().transpose(1, 2).contiguous()                                    # [2, 9, n]


def test_pointnet_2_seg_forward(synth):
    x = _model_input(synth)
    backbone = PU.model()
    seg = _seg_model(synth, state=backbone.state_dict())             # a pointnet_2 checkpoint: exactly bn1.* and conv2.* are missing
    log_probs, l0 = seg(x)
    assert log_probs.shape == (2, 256, 5) and l0.shape == (2, 128, 256)
    assert not log_probs.requires_grad and not l0.requires_grad
    assert torch.isfinite(log_probs).all() and torch.allclose(log_probs.exp().sum(-1), torch.ones((2, 256), device="cuda"), atol=1e-5)
    _, l0_backbone = backbone(x)
    assert torch.equal(l0, l0_backbone)                              # the same backbone state: the same bits
    head = sub("pointNet.model.pointnet2_utils").PointNetSegHead(128, 128, 5).eval()
    head.load_state_dict({k: v for k, v in seg.state_dict().items() if k.split(".")[0] in ("conv1", "bn1", "conv2")}, strict=True)
    assert torch.equal(head(l0), log_probs)                          # the model's head is the module
    pred = seg.predict(x)
    assert pred.shape == (2, 256) and pred.dtype == torch.int64
    assert np.array_equal(pred.cpu().numpy(), log_probs.cpu().numpy().argmax(-1))
    with pytest.raises(NotImplementedError, match="eval mode"):
        seg.train()(x)
    assert not seg._head.training


def test_pointnet_2_seg_nll_loss_reaches_every_parameter(synth):
    x = _model_input(synth)
    seg = _seg_model(synth, decoder_grad=True, encoder_grad=True)
    target = torch.from_numpy(sub("synthetic").randint(78, (2 * 256,), 0, 5)).cuda()
    buffers = {k: v.clone() for k, v in seg.named_buffers()}
    log_probs, l0 = seg(x)
    assert log_probs.requires_grad and l0.requires_grad
    F.nll_loss(log_probs.reshape(-1, 5), target.reshape(-1)).backward()
    names = [k for k, _ in seg.named_parameters()]
    assert {k.split(".")[0] for k in names} == {"sa1", "sa2", "sa3", "fp3", "fp2", "fp1", "conv1", "bn1", "conv2"}
    for k, p in seg.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert torch.isfinite(p.grad).all() and (p.grad != 0).any(), k
    for k, v in seg.named_buffers():
        assert torch.equal(v, buffers[k]), k
