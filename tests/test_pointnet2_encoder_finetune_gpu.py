"""Encoder fine-tuning of pointnet_2: PointNetSetAbstraction(grad=True) and pointnet_2(decoder_grad=True, encoder_grad=True) through
torch.autograd (autograd._SaFn -> ampnet_sa_backward_f32).  The defaults keep returning graph-free tensors with the same bits; train mode
still raises.  What ties the kernel to float64 is tests/test_sa_backward_gpu.py; here the module's gradients are the kernel's, bit for bit."""
import gc
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
from pn2_finetune_util import B, N, model as _net, model_input as _input, randomise as _randomise     # noqa: E402

pytestmark = pytest.mark.gpu

SA_BLOCKS = ("sa1", "sa2", "sa3")
TRAINABLE = SA_BLOCKS + ("fp3", "fp2", "fp1", "conv1")


def _model(decoder_grad, encoder_grad, state=None):
    return _net(state, decoder_grad=decoder_grad, encoder_grad=encoder_grad)


def _sa_pair(synth, n=96, D=13):
    """(plain block, grad=True twin with the same state, xyz [2, 3, n], points [2, D, n])"""
    M = sub("pointNet.model.pointnet2_utils")
    sa = M.PointNetSetAbstraction(12, 0.5, 20, 3 + D, [32, 64], False).eval()
    _randomise(sa, 4)
    twin = M.PointNetSetAbstraction(12, 0.5, 20, 3 + D, [32, 64], False, grad=True).eval()
    twin.load_state_dict(sa.state_dict())
    xyz = torch.from_numpy(synth.clouds(61, 2, n)).cuda().transpose(1, 2).contiguous()
    points = torch.from_numpy(synth.uniform(62, (2, D, n), -1.0, 1.0)).cuda()
    return sa, twin, xyz, points


def test_defaults_are_unchanged(synth):
    sa, twin, xyz, points = _sa_pair(synth)
    (nx, out), (nx_g, out_g) = sa(xyz, points), twin(xyz, points)
    assert not out.requires_grad and out.grad_fn is None and out_g.requires_grad and not nx_g.requires_grad
    assert torch.equal(out, out_g.detach()) and torch.equal(nx, nx_g) and (out > 0).any()
    with torch.no_grad():
        assert not twin(xyz, points)[1].requires_grad                 # grad mode off: no graph with grad=True either
    points.requires_grad_(True)
    assert not sa(xyz, points)[1].requires_grad                       # grad=False: no graph, whatever the input asks
    x = _input(synth)
    model = _model(True, False)
    glob, l0 = model(x)
    glob_g, l0_g = _model(True, True, model.state_dict())(x)
    assert torch.equal(l0.detach(), l0_g.detach()) and torch.equal(glob.detach(), glob_g.detach())
    plain = _model(False, False, model.state_dict())
    glob_p, l0_p = plain(x)
    assert not l0_p.requires_grad and torch.equal(l0_p, l0_g.detach())
    assert not plain.encoder_grad and not plain.sa1.grad


def test_grad_in_train_mode_still_raises(synth):
    _, twin, xyz, points = _sa_pair(synth)
    twin.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        twin(xyz, points)
    with pytest.raises(NotImplementedError, match="eval mode"):
        _model(True, True).train()(_input(synth))


def test_encoder_grad_needs_decoder_grad():
    M = sub("pointNet.model.pointnetAtt")
    with pytest.raises(ValueError, match="decoder_grad"):
        M.pointnet_2(5, decoder_grad=False, encoder_grad=True)


def test_module_gradients_are_the_kernels(synth):
    """points.grad and every parameter's .grad of a stand-alone PointNetSetAbstraction(grad=True) are bitwise what a direct
    _lib.sa_backward_f32 call gives on the same rows and the same dout."""
    L, U = sub("_lib"), sub("utils.utils")
    _, twin, xyz, points = _sa_pair(synth)
    points.requires_grad_(True)
    _, out = twin(xyz, points)                                        # [2, 64, 12]
    g = torch.Generator().manual_seed(5)
    r = (torch.rand(out.shape, generator=g) - 0.5).cuda()
    (out * r).sum().backward()
    assert points.grad is not None and points.grad.shape == points.shape
    # the same call by hand
    x = xyz.transpose(1, 2).contiguous()
    feats = points.detach().transpose(1, 2).contiguous()
    centres = U.fps_indices(x, twin.npoint)
    group_idx = U.ball_query(x, centres, twin.radius, twin.nsample)
    layers = [(conv.weight.detach().reshape(conv.weight.shape[0], -1).contiguous(), conv.bias.detach(), bn.weight.detach(), bn.bias.detach(),
               bn.running_mean, bn.running_var) for conv, bn in zip(twin.mlp_convs, twin.mlp_bns)]
    dout = r.transpose(1, 2).contiguous()                            # [2, 12, 64]
    dfeats = torch.full_like(feats, float("nan"))
    grads = [tuple(torch.full_like(t, float("nan")) for t in layer[:4]) for layer in layers]
    need = L.sa_backward_workspace_bytes(feats.shape[2], 2, twin.npoint, twin.nsample, [32, 64])
    L.sa_backward_f32(x, centres.contiguous(), group_idx, feats, layers, [bn.eps for bn in twin.mlp_bns], dout, dfeats, grads,
                      torch.empty(need, dtype=torch.uint8, device="cuda"))
    assert torch.equal(points.grad.transpose(1, 2), dfeats) and (dfeats != 0).any()
    for (conv, bn), gl in zip(zip(twin.mlp_convs, twin.mlp_bns), grads):
        assert conv.weight.grad.shape == conv.weight.shape           # [out, in, 1, 1]
        for p, t in zip((conv.weight, conv.bias, bn.weight, bn.bias), gl):
            assert torch.equal(p.grad.reshape(t.shape), t) and torch.isfinite(t).all() and (t != 0).any()
    # only what needs a gradient gets one
    points.grad = None
    for p in twin.mlp_bns.parameters():
        p.requires_grad_(False)
        p.grad = None
    (twin(xyz, points.detach())[1] * r).sum().backward()
    assert points.grad is None and all(p.grad is None for p in twin.mlp_bns.parameters())


def test_backward_through_the_whole_backbone(synth):
    x = _input(synth).requires_grad_(True)
    model = _model(True, True)
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    g = torch.Generator().manual_seed(11)
    r, q = torch.rand((B, 128, N), generator=g).cuda() - 0.5, torch.rand((B, 128), generator=g).cuda() - 0.5
    glob, l0 = model(x)
    ((l0 * r).sum() + (glob * q).sum()).backward()
    for name, p in model.named_parameters():
        assert name.startswith(tuple(t + "." for t in TRAINABLE)), name
        assert p.grad is not None and p.grad.shape == p.shape, name
        assert torch.isfinite(p.grad).all() and (p.grad != 0).any(), name
    for k, v in model.named_buffers():
        assert torch.equal(v, buffers[k]), k                          # running statistics and num_batches_tracked: bit-unchanged
    assert x.grad is None                                             # the input gets no gradient


def test_three_sgd_steps_on_the_encoder_lower_the_loss(synth):
    x = _input(synth)
    model = _model(True, True)
    g = torch.Generator().manual_seed(12)
    target, target_g = torch.rand((B, 128, N), generator=g).cuda(), torch.rand((B, 128), generator=g).cuda()
    trainable = [p for n, p in model.named_parameters() if n.startswith(SA_BLOCKS)]
    opt, losses = None, []
    for _ in range(4):
        glob, l0 = model(x)
        loss = ((l0 - target) ** 2).mean() + ((glob - target_g) ** 2).mean()
        losses.append(float(loss.detach()))
        model.zero_grad()
        loss.backward()
        if opt is None:
            # The encoder sits behind three decoder blocks and a mean over B 128 N elements: its gradient is small, and a step that
            # moves the float32 loss at all needs a rate to match.  The rate is fixed once, from the first gradient, so that the first
            # step lowers the loss by 0.1 % to first order (lr |g|^2 = 0.001 loss: 1e4 float32 ulps of it); plain SGD from there on.
            g2 = float(sum((p.grad.double() ** 2).sum() for p in trainable))
            assert g2 > 0
            opt = torch.optim.SGD(trainable, lr=1e-3 * losses[0] / g2)
            print(f"|g|^2 of sa1..sa3 = {g2:.3e}, lr = {1e-3 * losses[0] / g2:.3e}")
        opt.step()
    print("losses over three SGD steps on sa1..sa3:", losses)
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2], losses


def test_a_forward_without_backward_frees_its_saved_tensors(synth):
    x = _input(synth)
    model = _model(True, True)

    def settle():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    out = model(x)                                                    # first call: the blocks allocate their workspaces
    del out
    base = settle()
    out = model(x)
    assert out[1].requires_grad and torch.cuda.memory_allocated() > base
    del out
    assert settle() == base
