"""Decoder fine-tuning of pointnet_2: PointNetFeaturePropagation(grad=True) and pointnet_2(decoder_grad=True) through torch.autograd
(autograd._FpFn -> ampnet_fp_backward_f32).  The defaults keep returning graph-free tensors with the same bits; train mode still raises."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import fp_bwd_ref as R                             # noqa: E402

pytestmark = pytest.mark.gpu

B, N = 2, 512
FP_BLOCKS = ("fp3", "fp2", "fp1")


def _randomise(mod, seed):
    """Seeded values for every parameter and BatchNorm buffer (as tests/test_pointnet2_model_gpu.py does)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in mod.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var") or ("mlp_bns" in k and k.endswith("weight")):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * (0.6 if v.dim() == 1 else 2.0 / v.shape[1] ** 0.5)
    mod.load_state_dict(sd)


def _model(decoder_grad, state=None):
    """pointnet_2 in eval mode at the reduced sizes of test_pointnet_2_eval_forward_block_by_block (128 / 32 / 8 centres)."""
    M = sub("pointNet.model.pointnetAtt")
    model = M.pointnet_2(5, decoder_grad=decoder_grad).eval()
    for sa, npoint, radius in ((model.sa1, 128, 0.2), (model.sa2, 32, 0.4), (model.sa3, 8, 0.8)):
        sa.npoint, sa.radius = npoint, radius
    if state is None:
        _randomise(model, 8)
    else:
        model.load_state_dict(state)
    return model


def _input(synth):
    x = np.concatenate([synth.clouds(55, B, N), synth.uniform(56, (B, N, 6), -1.0, 1.0)], -1)        # [B, N, 9]
    return torch.from_numpy(x).cuda().transpose(1, 2).contiguous()                                  # [B, 9, N]


def test_defaults_are_unchanged(synth):
    M = sub("pointNet.model.pointnet2_utils")
    fp = M.PointNetFeaturePropagation(48, [32]).eval()
    _randomise(fp, 3)
    twin = M.PointNetFeaturePropagation(48, [32], grad=True).eval()
    twin.load_state_dict(fp.state_dict())
    xyz1 = torch.from_numpy(synth.clouds(54, 1, 64)).cuda().transpose(1, 2).contiguous()
    xyz2 = xyz1[:, :, :8].contiguous()
    p1 = torch.from_numpy(synth.uniform(57, (1, 16, 64), -1.0, 1.0)).cuda()
    p2 = torch.from_numpy(synth.uniform(58, (1, 32, 8), -1.0, 1.0)).cuda()
    out, out_g = fp(xyz1, xyz2, p1, p2), twin(xyz1, xyz2, p1, p2)
    assert not out.requires_grad and out.grad_fn is None and out_g.requires_grad
    assert torch.equal(out, out_g.detach()) and (out > 0).any()
    with torch.no_grad():
        assert not twin(xyz1, xyz2, p1, p2).requires_grad             # grad mode off: no graph with grad=True either
    x = _input(synth)
    model = _model(False)
    glob, l0 = model(x)
    assert not l0.requires_grad and glob.requires_grad == any(p.requires_grad for p in model.conv1.parameters())
    glob_g, l0_g = _model(True, model.state_dict())(x)
    assert l0_g.requires_grad and glob_g.requires_grad
    assert torch.equal(l0, l0_g.detach()) and torch.equal(glob.detach(), glob_g.detach())


def test_grad_in_train_mode_still_raises(synth):
    M = sub("pointNet.model.pointnet2_utils")
    fp = M.PointNetFeaturePropagation(48, [32], grad=True)
    assert fp.training
    xyz1 = torch.from_numpy(synth.clouds(54, 1, 64)).cuda().transpose(1, 2).contiguous()
    with pytest.raises(NotImplementedError, match="eval mode"):
        fp(xyz1, xyz1[:, :, :8].contiguous(), torch.zeros((1, 16, 64), device="cuda"), torch.zeros((1, 32, 8), device="cuda"))
    with pytest.raises(NotImplementedError, match="eval mode"):
        _model(True).train()(_input(synth))


def _layers_np(block):
    return [tuple(t.detach().cpu().numpy().reshape(t.shape[0], -1) if q == 0 else t.detach().cpu().numpy() for q, t in enumerate(
        (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var))) for conv, bn in zip(block.mlp_convs, block.mlp_bns)]


def test_decoder_backward_through_the_model(synth):
    """loss.backward() reaches every decoder parameter and no encoder parameter, leaves every buffer alone, and fp2's gradients -- its
    parameters' and the one it hands to fp3 -- are the restatement's on fp2's own inputs and the dout autograd delivered to it."""
    x = _input(synth)
    model = _model(True)
    # fp2's inputs do not depend on fp2: take them from a first pass and move fp2's betas off its ReLU inputs' bars (fp_bwd_ref.settle_betas)
    seen = {}
    inner = model.fp2._forward_rows

    def spy(x1, x2, p1, p2):
        out = inner(x1, x2, p1, p2)
        seen.update(x1=x1, x2=x2, p1=p1, p2=p2, out=out)
        if out.requires_grad:
            out.register_hook(lambda g: seen.__setitem__("dout", g.detach().clone()))
            p2.register_hook(lambda g: seen.__setitem__("dp2", g.detach().clone()))
        return out

    model.fp2._forward_rows = spy
    with torch.no_grad():
        model(x)
    U = sub("utils.utils")
    idx, dist2 = (t.cpu().numpy() for t in U.three_nn(seen["x1"], seen["x2"]))
    p1_np, p2_np = seen["p1"].cpu().numpy(), seen["p2"].cpu().numpy()
    layers = _layers_np(model.fp2)
    eps = [bn.eps for bn in model.fp2.mlp_bns]
    R.settle_betas(p1_np, p2_np, idx, dist2, layers, eps)
    with torch.no_grad():
        for bn, layer in zip(model.fp2.mlp_bns, layers):
            bn.bias.copy_(torch.from_numpy(layer[3]))
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    g = torch.Generator().manual_seed(11)
    r, q = torch.rand((B, 128, N), generator=g).cuda() - 0.5, torch.rand((B, 128), generator=g).cuda() - 0.5
    glob, l0 = model(x)
    ((l0 * r).sum() + (glob * q).sum()).backward()
    for name, p in model.named_parameters():
        if name.startswith(("sa1.", "sa2.", "sa3.")):
            assert p.grad is None, name
        else:
            assert name.startswith(FP_BLOCKS + ("conv1.",)), name
            assert p.grad is not None and p.grad.shape == p.shape, name
            assert torch.isfinite(p.grad).all() and (p.grad != 0).any(), name
    for k, v in model.named_buffers():
        assert torch.equal(v, buffers[k]), k                          # running statistics and num_batches_tracked: bit-unchanged
    assert np.array_equal(seen["p2"].detach().cpu().numpy(), p2_np) and seen["dout"].shape == (B, 128, 128)
    want, _ = R.fp_backward(p1_np, p2_np, idx, dist2, layers, eps, seen["dout"].cpu().numpy())
    got = {"dpoints2": seen["dp2"]}
    for l, (conv, bn) in enumerate(zip(model.fp2.mlp_convs, model.fp2.mlp_bns)):
        got.update({f"dW{l}": conv.weight.grad.reshape(conv.weight.shape[0], -1), f"dbias{l}": conv.bias.grad, f"dgamma{l}": bn.weight.grad,
                    f"dbeta{l}": bn.bias.grad})
    ratios = {k: float((np.abs(v.cpu().numpy().astype(np.float64) - want[k][0]) / np.maximum(want[k][1], 1e-300)).max()) for k, v in got.items()}
    print("fp2 inside pointnet_2: worst error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_three_sgd_steps_lower_the_loss(synth):
    x = _input(synth)
    model = _model(True)
    g = torch.Generator().manual_seed(12)
    target, target_g = torch.rand((B, 128, N), generator=g).cuda(), torch.rand((B, 128), generator=g).cuda()
    trainable = [p for n, p in model.named_parameters() if n.startswith(FP_BLOCKS + ("conv1.",))]
    opt = torch.optim.SGD(trainable, lr=1e-2)
    losses = []
    for _ in range(4):
        glob, l0 = model(x)
        loss = ((l0 - target) ** 2).mean() + ((glob - target_g) ** 2).mean()
        losses.append(float(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print("losses over three SGD steps:", losses)
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2], losses


def test_a_forward_without_backward_frees_its_saved_tensors(synth):
    x = _input(synth)
    model = _model(True)

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
