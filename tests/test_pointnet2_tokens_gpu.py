"""pointnet_2 as a window encoder on the GPU: forward_tokens / forward_tokens_ragged put the fused token (pointnet2_utils.token_pool:
conv1 and the segmented max as one kernel, tests/test_token_pool_gpu.py) behind the backbone's rows.  Held here: the rows are the
backbone's bits, the token is token_pool's bits on them and within the layer bar of the float64 conv1 + max, the ragged call is cloud by
cloud the uniform call, the graph rules are _backbone's, the token's gradient is wired into the backbone exactly as a hand-fed dx is, and
pointnet_2.forward and pointnet_2_seg are as they were."""
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
import token_pool_ref as R                         # noqa: E402
from pn2_finetune_util import randomise            # noqa: E402
from pw_probe import err_ratio                     # noqa: E402

pytestmark = pytest.mark.gpu
Q, N = 2, 1024
RAGGED = [1024, 1500, 1024]


def _M():
    return sub("pointNet.model.pointnetAtt")


def _token_pool(*a, **k):
    return sub("pointNet.model.pointnet2_utils").token_pool(*a, **k)


def _net(cls="pointnet_2", train=False, **kwargs):
    net = getattr(_M(), cls)(5, **kwargs).eval()
    randomise(net, 8)
    return net.train(train)


def _points(n_list, seed=55):
    synth = sub("synthetic")
    total = sum(n_list)
    x = np.concatenate([synth.clouds(seed, 1, total)[0], synth.uniform(seed + 1, (total, 6), -1.0, 1.0)], -1)     # [total, 9]
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def _default_run():
    """The default model on Q clouds of N points: computed once, shared."""
    net = _net()
    points = _points([N] * Q).view(Q, N, 9)
    with torch.no_grad():
        tokens, l0_rows = net.forward_tokens(points)
    return net, points, tokens, l0_rows


def test_forward_tokens_is_the_backbones_rows_and_the_fused_token_on_them():
    net, points, tokens, l0_rows = _default_run()
    assert tuple(tokens.shape) == (Q, 128) and tuple(l0_rows.shape) == (Q, N, 128)
    with torch.no_grad():
        assert torch.equal(l0_rows, net._backbone(points, rows=True)[0])
        t, arg = _token_pool(l0_rows, net.conv1.weight, net.conv1.bias, want_arg=True)
    assert torch.equal(tokens, t)
    rows = l0_rows.reshape(-1, 128).cpu().numpy()
    W, b = net.conv1.weight.detach().reshape(128, 128).cpu().numpy(), net.conv1.bias.detach().cpu().numpy()
    out64, _, bar_out = R.forward(rows, [N] * Q, W, b)
    worst = err_ratio(tokens.cpu().numpy(), out64, bar_out)
    print(f"forward_tokens: worst error / bar = {worst:.4f}")
    assert worst <= 1.0
    R.check_arg(arg.cpu().numpy(), rows, [N] * Q, W, b)


def test_forward_is_bitwise_the_torch_conv1_and_amax():
    net, points, tokens, l0_rows = _default_run()
    with torch.no_grad():
        gf, l0_points = net(points.transpose(1, 2).contiguous())
        assert torch.equal(gf, net.conv1(l0_points).amax(2))
        assert torch.equal(l0_points, l0_rows.transpose(1, 2))
    # the fused token is the same quantity in another summation order: inside twice the layer bar of each other
    rows = l0_rows.reshape(-1, 128).cpu().numpy()
    W, b = net.conv1.weight.detach().reshape(128, 128).cpu().numpy(), net.conv1.bias.detach().cpu().numpy()
    _, _, bar_out = R.forward(rows, [N] * Q, W, b)
    assert (np.abs(gf.cpu().numpy().astype(np.float64) - tokens.cpu().numpy()) <= 2 * bar_out).all()


def test_forward_tokens_ragged_is_forward_tokens_cloud_by_cloud():
    net = _default_run()[0]
    rows = _points(RAGGED, seed=77)
    with torch.no_grad():
        tokens, l0 = net.forward_tokens_ragged(rows, RAGGED)
        assert tuple(tokens.shape) == (len(RAGGED), 128) and tuple(l0.shape) == (sum(RAGGED), 128)
        off = R.offsets(RAGGED)
        for q, n in enumerate(RAGGED):
            t1, l1 = net.forward_tokens(rows[off[q]:off[q + 1]].reshape(1, n, 9).contiguous())
            assert torch.equal(tokens[q], t1[0]), f"cloud {q}"
            assert torch.equal(l0[off[q]:off[q + 1]], l1[0]), f"cloud {q}"
        net2, points, want_t, want_l = _default_run()
        t, l = net.forward_tokens_ragged(points.reshape(-1, 9), [N] * Q)                  # an equal-size layout
        assert torch.equal(t, want_t) and torch.equal(l, want_l.reshape(-1, 128))
    L = sub("_lib")
    with pytest.raises(L.AmpnetError, match="every cloud needs at least sa1.npoint=1024 points, cloud 1 has 1000"):
        net.forward_tokens_ragged(rows[:2024].contiguous(), [1024, 1000])


def test_default_model_the_backbone_is_frozen_and_conv1_alone_gets_a_graph():
    net, points, want_t, want_l = _default_run()
    p = points.clone().requires_grad_(True)
    tokens, l0_rows = net.forward_tokens(p)                      # grad mode on, the input asks for a gradient
    assert not l0_rows.requires_grad                             # no graph on the rows: the backbone is frozen, the input too
    assert torch.equal(tokens.detach(), want_t) and torch.equal(l0_rows, want_l)
    assert tokens.requires_grad                                  # conv1 is a torch parameter: torch's own rule
    net.zero_grad(set_to_none=True)
    tokens.sum().backward()
    assert p.grad is None
    with_grad = sorted(n for n, q in net.named_parameters() if q.grad is not None)
    assert with_grad == ["conv1.bias", "conv1.weight"], with_grad
    net.zero_grad(set_to_none=True)
    with torch.no_grad():
        assert not net.forward_tokens(p)[0].requires_grad


@pytest.mark.parametrize("train", [False, True], ids=["eval_finetune", "train_batch_stats"])
def test_the_tokens_gradient_reaches_the_backbone_as_a_hand_fed_dx_does(train):
    flags = dict(decoder_grad=True, encoder_grad=True)
    if train:
        flags.update(decoder_batch_stats=True, encoder_batch_stats=True)
    net = _net(train=train, **flags)
    points = _points([N] * Q).view(Q, N, 9)
    g = torch.from_numpy(sub("synthetic").uniform(91, (Q, 128), -1.0, 1.0)).cuda()
    watched = [n for n, _ in net.named_parameters() if n.split(".")[0] in ("sa1", "fp1")]

    tokens, l0_rows = net.forward_tokens(points)
    assert tokens.requires_grad and l0_rows.requires_grad
    (tokens * g).sum().backward()
    first = {n: q.grad.clone() for n, q in net.named_parameters() if q.grad is not None}
    for n in watched + ["conv1.weight", "conv1.bias"]:
        assert n in first and torch.isfinite(first[n]).all(), n
        # (under batch statistics a block's conv bias cancels in its BatchNorm: that gradient is exactly zero, as torch's is)
        assert (first[n] != 0).any() != (train and "mlp_convs" in n and n.endswith("bias")), n

    # the dx token_pool's backward gives for the same dout on the detached rows, and the float64 restatement of conv1's gradients
    rows_d = l0_rows.detach().clone().requires_grad_(True)
    W, b = net.conv1.weight.detach().clone().requires_grad_(True), net.conv1.bias.detach().clone().requires_grad_(True)
    t2, arg = _token_pool(rows_d, W, b, want_arg=True)
    assert torch.equal(t2.detach(), tokens.detach())
    (t2 * g).sum().backward()
    assert torch.equal(W.grad, first["conv1.weight"]) and torch.equal(b.grad, first["conv1.bias"])
    ref = R.backward(rows_d.detach().reshape(-1, 128).cpu().numpy(), [N] * Q, W.detach().reshape(128, 128).cpu().numpy(), arg.cpu().numpy(),
                     g.cpu().numpy())
    for name, got in (("dW", first["conv1.weight"].reshape(128, 128)), ("db", first["conv1.bias"])):
        worst = err_ratio(got.cpu().numpy(), *ref[name])
        print(f"forward_tokens {'train' if train else 'eval'} conv1 {name}: worst error / bar = {worst:.4f}")
        assert worst <= 1.0

    # wiring, bit for bit: a second identical forward, the same dx fed to l0_rows by hand
    net.zero_grad(set_to_none=True)
    _, l0_again = net.forward_tokens(points)
    assert torch.equal(l0_again.detach(), l0_rows.detach())
    l0_again.backward(rows_d.grad)
    for n in watched:
        assert torch.equal(net.get_parameter(n).grad, first[n]), n
    assert net.conv1.weight.grad is None


def test_pointnet_2_seg_has_no_token():
    net = _net("pointnet_2_seg")
    for call in (lambda: net.forward_tokens(_points([N]).view(1, N, 9)), lambda: net.forward_tokens_ragged(_points([N]), [N])):
        with pytest.raises(NotImplementedError, match="conv1 is the first layer of the segmentation head"):
            call()


def test_bf16_blocks_keep_an_exact_fp32_token():
    net = _net(precision="bf16")
    points = _default_run()[1]
    with torch.no_grad():
        tokens, l0_rows = net.forward_tokens(points)
        assert tuple(l0_rows.shape) == (Q, N, 128) and torch.isfinite(tokens).all()
        assert torch.equal(tokens, _token_pool(l0_rows, net.conv1.weight, net.conv1.bias))
        assert not torch.equal(l0_rows, _default_run()[3])       # (the blocks did run in bf16)
