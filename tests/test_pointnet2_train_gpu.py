"""Train-mode BatchNorm in the encoder of pointnet_2: PointNetSetAbstraction(batch_stats=True) and
pointnet_2(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True) through torch.autograd
(autograd._SaTrainFn -> ampnet_sa_train_forward_f32 / ampnet_sa_train_backward_f32).  The module and the model must hand the C ABI's
results on bit for bit; the arithmetic itself is checked in tests/test_sa_train_gpu.py."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import pn2_finetune_util as T                      # noqa: E402

pytestmark = pytest.mark.gpu

FP_BLOCKS = ("fp3", "fp2", "fp1")
SA_BLOCKS = ("sa1", "sa2", "sa3")
ALL = dict(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True)


def _block_inputs(synth, scale=1.0):
    """The tail_group form (n 70, 9 centres, nsample 20, D 6), channel-major as the module takes it; the features require grad."""
    xyz = torch.from_numpy(synth.clouds(71, 2, 70)).cuda().transpose(1, 2).contiguous()
    points = (torch.from_numpy(synth.uniform(72, (2, 6, 70), -1.0, 1.0)).cuda() * scale).requires_grad_(True)
    centres = (torch.arange(9, dtype=torch.int32, device="cuda") * 7 + 1).repeat(2, 1).contiguous()
    return xyz, points, centres


def _block(state=None, **kwargs):
    M = sub("pointNet.model.pointnet2_utils")
    sa = M.PointNetSetAbstraction(9, 0.35, 20, 9, [32, 64], False, **kwargs)
    if state is None:
        T.randomise(sa, 6)
    else:
        sa.load_state_dict(state)
    return sa


def _direct(block_state, mlp_len, eps, radius, nsample, x, centres, feats, dout, want_dfeats=True):
    """The C ABI on point-major rows with copies of a block's state -> (out, updated layers, {gradient name: tensor})."""
    L, A, U = sub("_lib"), sub("autograd"), sub("utils.utils")
    group_idx = U.ball_query(x, centres, radius, nsample)
    layers = [tuple(block_state[f"{k}.{l}.{q}"].detach().clone().reshape(block_state[f"{k}.{l}.{q}"].shape[0], -1) if (k, q) == ("mlp_convs", "weight")
                    else block_state[f"{k}.{l}.{q}"].detach().clone()
                    for k, q in (("mlp_convs", "weight"), ("mlp_convs", "bias"), ("mlp_bns", "weight"), ("mlp_bns", "bias"),
                                 ("mlp_bns", "running_mean"), ("mlp_bns", "running_var"))) for l in range(mlp_len)]
    out, sm, si = A.sa_train_forward(x, centres, group_idx, feats, layers, eps, 0.1)
    if dout is None:
        return out, layers, {}
    dfeats = torch.empty_like(feats) if want_dfeats else None
    grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in layers]
    need = L.sa_train_backward_workspace_bytes(feats.shape[2], x.shape[0], centres.shape[1], nsample, [g[0].shape[0] for g in grads])
    L.sa_train_backward_f32(x, centres, group_idx, feats, layers, eps, sm, si, dout.contiguous(), dfeats, grads,
                            torch.empty(need, dtype=torch.uint8, device="cuda"))
    return out, layers, dict(dfeats=dfeats, grads=grads)


def _rows(t):
    return t.detach().transpose(1, 2).contiguous()


def _assert_block_grads(sa, points, want):
    assert torch.equal(points.grad, want["dfeats"].transpose(1, 2))
    for l, (conv, bn) in enumerate(zip(sa.mlp_convs, sa.mlp_bns)):
        dW, dbias, dgamma, dbeta = want["grads"][l]
        assert conv.weight.grad.shape == conv.weight.shape and conv.weight.grad.dim() == 4          # [out, in, 1, 1]
        assert torch.equal(conv.weight.grad.reshape(dW.shape), dW), l
        assert torch.equal(conv.bias.grad, torch.zeros_like(conv.bias)) and (dbias == 0).all(), l
        assert torch.equal(bn.weight.grad, dgamma) and torch.equal(bn.bias.grad, dbeta), l
        assert (dW != 0).any() and (dgamma != 0).any() and (dbeta != 0).any()


def test_batch_stats_block_in_eval_mode_is_the_default_block(synth):
    xyz, points, centres = _block_inputs(synth)
    plain = _block().eval()
    flagged = _block(plain.state_dict(), batch_stats=True).eval()
    buffers = {k: v.clone() for k, v in flagged.named_buffers()}
    with torch.no_grad():
        want_xyz, want = plain(xyz, points, centres)
        got_xyz, got = flagged(xyz, points, centres)
    assert torch.equal(want, got) and torch.equal(want_xyz, got_xyz)
    graphed = _block(plain.state_dict(), batch_stats=True, grad=True).eval()
    _, out = graphed(xyz, points, centres)
    assert out.requires_grad and torch.equal(out.detach(), want)
    for mod in (flagged, graphed):
        for k, v in mod.named_buffers():
            assert torch.equal(v, buffers[k]), k


def test_block_in_train_mode_hands_on_the_c_abi(synth):
    xyz, points, centres = _block_inputs(synth)
    sa = _block(batch_stats=True, grad=True)
    assert sa.training
    state = {k: v.clone() for k, v in sa.state_dict().items()}
    eps = [bn.eps for bn in sa.mlp_bns]
    r = torch.from_numpy(synth.uniform(74, (2, 64, 9), -1.0, 1.0)).cuda()
    new_xyz, out = sa(xyz, points, centres)
    assert out.requires_grad and out.shape == (2, 64, 9) and not new_xyz.requires_grad
    (out * r).sum().backward()
    want_out, layers, want = _direct(state, 2, eps, 0.35, 20, _rows(xyz), centres, _rows(points), _rows(r))
    assert torch.equal(out.detach(), want_out.transpose(1, 2))
    _assert_block_grads(sa, points, want)
    for l, bn in enumerate(sa.mlp_bns):                               # updated once, as the C ABI updates them
        assert torch.equal(bn.running_mean, layers[l][4]) and torch.equal(bn.running_var, layers[l][5])
        assert not torch.equal(bn.running_mean, state[f"mlp_bns.{l}.running_mean"])
        assert int(bn.num_batches_tracked) == int(state[f"mlp_bns.{l}.num_batches_tracked"]) + 1
    assert sorted(sa.state_dict()) == sorted(_block().state_dict())   # momentum is no state_dict key
    # two forwards, then the FIRST one's backward: its own saved statistics, whatever the second forward did to the buffers
    xyzb, pointsb, _ = _block_inputs(synth)
    twin = _block(state, batch_stats=True, grad=True)
    _, first = twin(xyzb, pointsb, centres)
    _, other, _ = _block_inputs(synth, scale=3.0)
    twin(xyzb, other, centres)
    (first * r).sum().backward()
    _assert_block_grads(twin, pointsb, want)
    assert all(int(bn.num_batches_tracked) == int(state[f"mlp_bns.{l}.num_batches_tracked"]) + 2 for l, bn in enumerate(twin.mlp_bns))
    assert not torch.equal(twin.mlp_bns[0].running_mean, sa.mlp_bns[0].running_mean)
    # no graph under no_grad, or with grad=False: the statistics still move, as torch's do
    for mod, ctx in ((_block(state, batch_stats=True, grad=True), torch.no_grad()), (_block(state, batch_stats=True), torch.enable_grad())):
        with ctx:
            _, quiet = mod(xyz, points, centres)
        assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, out.detach())
        for l, bn in enumerate(mod.mlp_bns):
            assert torch.equal(bn.running_mean, layers[l][4]) and torch.equal(bn.running_var, layers[l][5])
            assert int(bn.num_batches_tracked) == int(state[f"mlp_bns.{l}.num_batches_tracked"]) + 1
    none = _block(state, batch_stats=True, grad=True)
    none.mlp_bns[0].momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        none(xyz, points, centres)


def test_default_block_in_train_mode_still_raises(synth):
    xyz, points, centres = _block_inputs(synth)
    for kwargs in ({}, dict(grad=True)):
        blk = _block(**kwargs)
        assert blk.training
        with pytest.raises(NotImplementedError, match="eval mode"):
            blk(xyz, points, centres)
        with pytest.raises(NotImplementedError, match="eval mode"):
            blk._forward_rows(_rows(xyz), _rows(points), centres)


def test_the_flag_needs_encoder_grad_and_decoder_batch_stats():
    M = sub("pointNet.model.pointnetAtt")
    for kwargs in (dict(encoder_batch_stats=True), dict(decoder_grad=True, encoder_batch_stats=True),
                   dict(decoder_grad=True, encoder_grad=True, encoder_batch_stats=True),
                   dict(decoder_grad=True, decoder_batch_stats=True, encoder_batch_stats=True)):
        with pytest.raises(ValueError, match="encoder_batch_stats"):
            M.pointnet_2(5, **kwargs)
    # decoder_batch_stats alone still keeps the encoder in eval mode
    model = T.model(decoder_grad=True, encoder_grad=True, decoder_batch_stats=True).train()
    assert all(not getattr(model, n).training for n in SA_BLOCKS) and all(getattr(model, n).training for n in FP_BLOCKS)


def _loss(model, x, r, q):
    glob, l0 = model(x)
    return (l0 * r).sum() + (glob * q).sum()


def _targets(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((T.B, 128, T.N), generator=g).cuda() - 0.5, torch.rand((T.B, 128), generator=g).cuda() - 0.5


def test_one_training_step_of_the_whole_model(synth):
    x = T.model_input(synth)
    model = T.model(**ALL)
    assert model.train() is model and all(m.training for m in model.modules())
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    state = {k: v.clone() for k, v in model.sa2.state_dict().items()}
    seen = {}
    inner = model.sa2._train_rows

    def spy(xr, centres, group_idx, feats):
        out = inner(xr, centres, group_idx, feats)
        seen.update(x=xr.detach(), centres=centres, feats=feats.detach(), out=out.detach())
        out.register_hook(lambda g: seen.__setitem__("dout", g.detach().clone()))
        return out

    model.sa2._train_rows = spy
    r, q = _targets(11)
    _loss(model, x, r, q).backward()
    for k, v in model.named_buffers():                                # every BatchNorm buffer of all six blocks moves
        assert k.startswith(SA_BLOCKS + FP_BLOCKS) and not torch.equal(v, buffers[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(buffers[k]) + 1, k
    for name, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), name
        if "mlp_convs" in name and name.endswith("bias"):
            assert (p.grad == 0).all(), name                          # no effect on a batch-normalised output: exact zeros
        else:
            assert (p.grad != 0).any(), name
    # sa2 inside the model is the C ABI on the same inputs (l1_points also feeds fp2's skip input, so its own .grad is a sum and is not
    # compared here; the block test above compares dfeats)
    out, layers, want = _direct(state, 3, [bn.eps for bn in model.sa2.mlp_bns], model.sa2.radius, model.sa2.nsample, seen["x"], seen["centres"],
                                seen["feats"], seen["dout"])
    assert torch.equal(out, seen["out"])
    for l, (conv, bn) in enumerate(zip(model.sa2.mlp_convs, model.sa2.mlp_bns)):
        dW, dbias, dgamma, dbeta = want["grads"][l]
        assert torch.equal(conv.weight.grad.reshape(dW.shape), dW) and torch.equal(conv.bias.grad, dbias) and (dbias == 0).all(), l
        assert torch.equal(bn.weight.grad, dgamma) and torch.equal(bn.bias.grad, dbeta) and (dgamma != 0).any(), l
        assert torch.equal(bn.running_mean, layers[l][4]) and torch.equal(bn.running_var, layers[l][5]), l
    assert (want["dfeats"] != 0).any()
    assert model.eval() is model and not any(m.training for m in model.modules())
    model.train()
    model.sa1.eval()
    with pytest.raises(NotImplementedError, match="model's mode"):
        model(x)


def test_sgd_on_a_fixed_batch_is_reproducible_and_eval_follows_the_state(synth):
    x = T.model_input(synth)
    g = torch.Generator().manual_seed(12)
    target, target_g = torch.rand((T.B, 128, T.N), generator=g).cuda(), torch.rand((T.B, 128), generator=g).cuda()

    def run(state):
        model = T.model(state, **ALL).train()
        opt = torch.optim.SGD(model.parameters(), lr=1e-2)
        losses = []
        for _ in range(4):
            glob, l0 = model(x)
            loss = ((l0 - target) ** 2).mean() + ((glob - target_g) ** 2).mean()
            losses.append(float(loss.detach()))
            opt.zero_grad()
            loss.backward()
            opt.step()
        return model, losses

    start = {k: v.clone() for k, v in T.model().state_dict().items()}
    model, losses = run(start)
    _, again = run(start)
    print("losses over four train-mode SGD steps of the whole backbone:", losses)
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses == again
    assert not torch.equal(model.sa1.mlp_convs[0].weight.detach(), start["sa1.mlp_convs.0.weight"])
    with torch.no_grad():
        glob, l0 = model.eval()(x)
        glob_d, l0_d = T.model(model.state_dict())(x)                 # a default pointnet_2 with the trained state
    assert torch.equal(glob, glob_d) and torch.equal(l0, l0_d)
