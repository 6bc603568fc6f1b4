"""PointNetSegHead(batch_stats=True) and pointnet_2_seg(head_batch_stats=True) in train mode on the GPU: the module against a torch head
that is fed the same mask (built from the module's seed), the seed convention, the strict state_dict exchange, and the model trained from
scratch for a few steps.  The arithmetic itself is checked tightly in tests/test_seg_head_train_gpu.py."""
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
import seg_head_train_ref as R                     # noqa: E402

pytestmark = pytest.mark.gpu

B, N = 2, 35                                       # 70 rows: the `tail` case of seg_head_train_ref (128 -> 128 -> 5) as two clouds
FLAGS = dict(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True, head_batch_stats=True)


class _TorchHead(torch.nn.Module):
    """The usual PointNet++ head with the dropout's mask handed in: mask [B, hidden, N], keep * dscale."""

    def __init__(self, cin, hidden, classes):
        super().__init__()
        self.conv1, self.bn1, self.drop1, self.conv2 = (torch.nn.Conv1d(cin, hidden, 1), torch.nn.BatchNorm1d(hidden), torch.nn.Dropout(0.5),
                                                        torch.nn.Conv1d(hidden, classes, 1))

    def forward(self, p, mask):
        return torch.log_softmax(self.conv2(torch.relu(self.bn1(self.conv1(p))) * mask), dim=1).permute(0, 2, 1)


def _head(synth, **kwargs):
    """(a PointNetSegHead with the `tail` case's parameters, its input [B, 128, N], the case)."""
    U = sub("pointNet.model.pointnet2_utils")
    i, _, _ = R.reference(synth, "tail")
    head = U.PointNetSegHead(128, 128, 5, **kwargs)
    W1, b1, gamma, beta, mean, var, W2, b2 = (torch.from_numpy(p) for p in i["params"])
    head.load_state_dict({"conv1.weight": W1[:, :, None], "conv1.bias": b1, "bn1.weight": gamma, "bn1.bias": beta, "bn1.running_mean": mean,
                          "bn1.running_var": var, "bn1.num_batches_tracked": torch.tensor(3), "conv2.weight": W2[:, :, None], "conv2.bias": b2})
    points = torch.from_numpy(i["x"]).cuda().reshape(B, N, 128).transpose(1, 2).contiguous()
    return head, points, i


def _mask(seed, p, rows, hidden):
    """keep * dscale of a call with that seed as [B, hidden, N]: the module's rows are the flat [B * N, hidden] list."""
    m = R.keep_mask(seed, rows, hidden, p).astype(np.float32) * np.float32(R.drop_scale(p))
    return torch.from_numpy(m).cuda().reshape(B, rows // B, hidden).transpose(1, 2).contiguous()


def test_defaults_still_refuse_train_mode(synth):
    head, points, _ = _head(synth, grad=True)
    with pytest.raises(NotImplementedError, match="eval mode"):
        head.train()(points)
    A = sub("pointNet.model.pointnetAtt")
    seg = A.pointnet_2_seg(5, decoder_grad=True, decoder_batch_stats=True).train()
    assert not seg._head.training and seg.fp1.training
    with pytest.raises(ValueError, match="head_batch_stats=True needs decoder_batch_stats=True"):
        A.pointnet_2_seg(5, decoder_grad=True, head_batch_stats=True)
    trainable, _, _ = _head(synth, grad=True, batch_stats=True)
    with pytest.raises(NotImplementedError, match="predict is an eval operation"):
        trainable.train().predict(points)


def test_train_mode_against_a_torch_head_fed_the_same_mask(synth):
    """The float32 torch composition on the same tensors and the same mask, loosely (1e-3 of each tensor's scale: torch sums in other
    orders), the convention of tests/test_seg_head_module_gpu.py."""
    head, points, i = _head(synth, grad=True, batch_stats=True)
    ref = _TorchHead(128, 128, 5).cuda()
    ref.load_state_dict(head.state_dict(), strict=True)              # our state into a torch head, strictly
    head.train(), ref.train()
    mask = _mask(head.seed, head.drop1.p, B * N, 128)                # _step is 0: the first call's seed is `seed` itself
    g = torch.from_numpy(i["dlogp"]).cuda().reshape(B, N, 5)
    a, b = points.clone().requires_grad_(True), points.clone().requires_grad_(True)
    out, want = head(a), ref(b, mask)
    assert out.shape == (B, N, 5) and out.requires_grad and head._step == 1
    err, scale = float((out - want).detach().abs().max()), float(want.detach().abs().max())
    print(f"seg_head train module output: max |difference| / max |torch| = {err / scale:.2e}")
    assert err <= 1e-3 * scale
    (out * g).sum().backward()
    (want * g).sum().backward()
    pairs = [("points", a.grad, b.grad)] + [(k, p.grad, dict(ref.named_parameters())[k].grad) for k, p in head.named_parameters()]
    assert sorted(k for k, _, _ in pairs[1:]) == sorted(["conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "conv2.weight", "conv2.bias"])
    for k, got, exp in pairs:
        assert got is not None and got.shape == exp.shape, k
        if k == "conv1.bias":                                        # exact zeros here, a cancelling float32 sum in torch
            assert (got == 0).all() and float(exp.abs().max()) <= 1e-3 * float(b.grad.abs().max()), k
            continue
        err, scale = float((got - exp).abs().max()), float(exp.abs().max())
        print(f"seg_head train module gradient {k}: max |difference| / max |torch| = {err / scale:.2e}")
        assert err <= 1e-3 * scale, (k, err, scale)
    assert torch.allclose(head.bn1.running_mean, ref.bn1.running_mean) and torch.allclose(head.bn1.running_var, ref.bn1.running_var)
    assert not torch.equal(head.bn1.running_mean, torch.from_numpy(i["params"][4]).cuda())
    assert int(head.bn1.num_batches_tracked) == 4 == int(ref.bn1.num_batches_tracked)
    # the exchange stays strict after training, in both directions
    back = sub("pointNet.model.pointnet2_utils").PointNetSegHead(128, 128, 5)
    back.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(head.state_dict(), strict=True)
    assert list(head.state_dict()) == list(ref.state_dict())


def test_seeds_follow_the_house_convention(synth):
    one, points, _ = _head(synth, batch_stats=True)
    two, _, _ = _head(synth, batch_stats=True)
    one.train(), two.train()
    a1, b1 = one(points), two(points)
    assert a1.grad_fn is None and torch.equal(a1, b1)                # equal seed and step: equal bits
    assert int(one.bn1.num_batches_tracked) == 4                     # counted without a graph too
    a2 = one(points)
    assert one._step == 2 and not torch.equal(a1, a2)                # the next call draws another mask
    two.seed, two._step = one.seed, 1
    two.bn1.load_state_dict({k: v.clone() for k, v in one.bn1.state_dict().items()})
    one._step = 1
    assert torch.equal(one(points), two(points))                     # a user reproduces a call from seed and step
    step = one._step
    one.eval()
    e1, e2 = one(points), one(points)
    assert one._step == step and torch.equal(e1, e2)                 # eval mode: no dropout, no step
    with torch.no_grad():
        one.drop1.p = 0.0
        one.train()
        d1, d2 = one(points), one(points)
    assert torch.equal(d1, d2)                                       # p = 0: the identity, whatever the seed


def _seg_model(**kwargs):
    """pointnet_2_seg(5) in eval mode at the reduced sizes of pn2_finetune_util.model (128 / 32 / 8 centres), seeded."""
    A = sub("pointNet.model.pointnetAtt")
    net = A.pointnet_2_seg(5, **kwargs).eval()
    for sa, npoint, radius in ((net.sa1, 128, 0.2), (net.sa2, 32, 0.4), (net.sa3, 8, 0.8)):
        sa.npoint, sa.radius = npoint, radius
    PU.randomise(net, 8)
    return net


def test_pointnet_2_seg_trains_from_scratch(synth):
    x = np.concatenate([synth.clouds(55, 2, 256), synth.uniform(56, (2, 256, 6), -1.0, 1.0)], -1)          # [2, 256, 9]
    x = torch.from_numpy(x).cuda().transpose(1, 2).contiguous()
    target = torch.from_numpy(synth.randint(78, (2 * 256,), 0, 5)).cuda()
    seg = _seg_model(**FLAGS)
    with torch.no_grad():
        before = float(F.nll_loss(seg(x)[0].reshape(-1, 5), target))
    mean0 = seg.bn1.running_mean.clone()
    assert seg.train() is seg and seg._head.training and seg.bn1.training and seg.drop1.training and seg.sa1.training
    opt = torch.optim.SGD(seg.parameters(), lr=0.1)
    for step in range(5):
        opt.zero_grad()
        log_probs, _ = seg(x)
        assert log_probs.requires_grad
        F.nll_loss(log_probs.reshape(-1, 5), target).backward()
        if step == 0:
            for k, p in seg.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all(), k
                # (a conv bias in front of a batch-statistics BatchNorm has no effect on the output: exact zeros, by the kernels' contract)
                conv_bias = k == "conv1.bias" or ("mlp_convs" in k and k.endswith("bias"))
                assert (p.grad == 0).all() if conv_bias else (p.grad != 0).any(), k
        opt.step()
    assert seg._head._step == 5 and int(seg.bn1.num_batches_tracked) == 3 + 5
    assert not torch.equal(seg.bn1.running_mean, mean0)
    seg.eval()
    assert not seg._head.training
    with torch.no_grad():
        trained = seg(x)[0]
    after = float(F.nll_loss(trained.reshape(-1, 5), target))
    print(f"pointnet_2_seg from scratch: eval nll_loss {before:.4f} -> {after:.4f} after five SGD steps")
    assert after < before
    plain = _seg_model()
    plain.load_state_dict(seg.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(plain(x)[0], trained)                     # the trained state in a default model: the same bits
