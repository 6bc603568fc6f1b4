"""Train-mode BatchNorm in the decoder of pointnet_2: PointNetFeaturePropagation(batch_stats=True) and
pointnet_2(decoder_grad=True, decoder_batch_stats=True) through torch.autograd (autograd._FpTrainFn -> ampnet_fp_train_forward_f32 /
ampnet_fp_train_backward_f32).  The module and the model must hand the C ABI's results on bit for bit; the arithmetic itself is checked in
tests/test_fp_train_gpu.py."""
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


def _block_inputs(synth, scale=1.0):
    """The tail_tile form (n 70, s 9, D1 16, D2 32), channel-major as the module takes it; the leaves require grad."""
    xyz1 = torch.from_numpy(synth.clouds(61, 2, 70)).cuda().transpose(1, 2).contiguous()
    xyz2 = xyz1[:, :, 1::8][:, :, :9].contiguous()
    p1 = (torch.from_numpy(synth.uniform(62, (2, 16, 70), -1.0, 1.0)).cuda() * scale).requires_grad_(True)
    p2 = (torch.from_numpy(synth.uniform(63, (2, 32, 9), -1.0, 1.0)).cuda() * scale).requires_grad_(True)
    return xyz1, xyz2, p1, p2


def _block(state=None, **kwargs):
    M = sub("pointNet.model.pointnet2_utils")
    fp = M.PointNetFeaturePropagation(48, [32, 64], **kwargs)
    if state is None:
        T.randomise(fp, 5)
    else:
        fp.load_state_dict(state)
    return fp


def _direct(block_state, mlp_len, eps, x1, x2, p1, p2, dout):
    """The C ABI on point-major rows with copies of a block's state -> (out, updated layers, {gradient name: tensor})."""
    L, A, U = sub("_lib"), sub("autograd"), sub("utils.utils")
    idx, dist2 = U.three_nn(x1, x2)
    layers = [tuple(block_state[f"{k}.{l}.{q}"].detach().clone().reshape(block_state[f"{k}.{l}.{q}"].shape[0], -1) if (k, q) == ("mlp_convs", "weight")
                    else block_state[f"{k}.{l}.{q}"].detach().clone()
                    for k, q in (("mlp_convs", "weight"), ("mlp_convs", "bias"), ("mlp_bns", "weight"), ("mlp_bns", "bias"),
                                 ("mlp_bns", "running_mean"), ("mlp_bns", "running_var"))) for l in range(mlp_len)]
    out, sm, si = A.fp_train_forward(p1, p2, idx, dist2, layers, eps, 0.1)
    if dout is None:
        return out, layers, {}
    dp1 = None if p1 is None else torch.empty_like(p1)
    dp2 = torch.empty_like(p2)
    grads = [tuple(torch.empty_like(t) for t in layer[:4]) for layer in layers]
    need = L.fp_train_backward_workspace_bytes(0 if p1 is None else p1.shape[2], p2.shape[2], p2.shape[0], idx.shape[1], [g[0].shape[0] for g in grads])
    L.fp_train_backward_f32(p1, p2, idx, dist2, layers, eps, sm, si, dout.contiguous(), dp1, dp2, grads,
                            torch.empty(need, dtype=torch.uint8, device="cuda"))
    return out, layers, dict(dp1=dp1, dp2=dp2, grads=grads)


def _rows(t):
    return t.detach().transpose(1, 2).contiguous()


def _assert_block_grads(fp, got_p1, got_p2, want):
    assert torch.equal(got_p1.grad, want["dp1"].transpose(1, 2)) and torch.equal(got_p2.grad, want["dp2"].transpose(1, 2))
    for l, (conv, bn) in enumerate(zip(fp.mlp_convs, fp.mlp_bns)):
        dW, dbias, dgamma, dbeta = want["grads"][l]
        assert conv.weight.grad.shape == conv.weight.shape and conv.weight.grad.dim() == 3          # [out, in, 1]
        assert torch.equal(conv.weight.grad.reshape(dW.shape), dW), l
        assert torch.equal(conv.bias.grad, torch.zeros_like(conv.bias)) and (dbias == 0).all(), l
        assert torch.equal(bn.weight.grad, dgamma) and torch.equal(bn.bias.grad, dbeta), l
        assert (dW != 0).any() and (dgamma != 0).any() and (dbeta != 0).any()


def test_batch_stats_block_in_eval_mode_is_the_default_block(synth):
    xyz1, xyz2, p1, p2 = _block_inputs(synth)
    plain = _block().eval()
    flagged = _block(plain.state_dict(), batch_stats=True).eval()
    buffers = {k: v.clone() for k, v in flagged.named_buffers()}
    with torch.no_grad():
        assert torch.equal(plain(xyz1, xyz2, p1, p2), flagged(xyz1, xyz2, p1, p2))
    graphed = _block(plain.state_dict(), batch_stats=True, grad=True).eval()
    out = graphed(xyz1, xyz2, p1, p2)
    assert out.requires_grad and torch.equal(out.detach(), plain(xyz1, xyz2, p1, p2))
    for mod in (flagged, graphed):
        for k, v in mod.named_buffers():
            assert torch.equal(v, buffers[k]), k


def test_block_in_train_mode_hands_on_the_c_abi(synth):
    xyz1, xyz2, p1, p2 = _block_inputs(synth)
    fp = _block(batch_stats=True, grad=True)
    assert fp.training
    state = {k: v.clone() for k, v in fp.state_dict().items()}
    eps = [bn.eps for bn in fp.mlp_bns]
    r = torch.from_numpy(synth.uniform(64, (2, 64, 70), -1.0, 1.0)).cuda()
    out = fp(xyz1, xyz2, p1, p2)
    assert out.requires_grad and out.shape == (2, 64, 70)
    (out * r).sum().backward()
    want_out, layers, want = _direct(state, 2, eps, _rows(xyz1), _rows(xyz2), _rows(p1), _rows(p2), _rows(r))
    assert torch.equal(out.detach(), want_out.transpose(1, 2))
    _assert_block_grads(fp, p1, p2, want)
    for l, bn in enumerate(fp.mlp_bns):                               # updated once, as the C ABI updates them
        assert torch.equal(bn.running_mean, layers[l][4]) and torch.equal(bn.running_var, layers[l][5])
        assert not torch.equal(bn.running_mean, state[f"mlp_bns.{l}.running_mean"])
        assert int(bn.num_batches_tracked) == int(state[f"mlp_bns.{l}.num_batches_tracked"]) + 1
    assert sorted(fp.state_dict()) == sorted(_block().state_dict())   # momentum is no state_dict key
    # two forwards, then the FIRST one's backward: its own saved statistics, whatever the second forward did to the buffers
    xyz1b, xyz2b, p1b, p2b = _block_inputs(synth)
    twin = _block(state, batch_stats=True, grad=True)
    first = twin(xyz1b, xyz2b, p1b, p2b)
    _, _, q1, q2 = _block_inputs(synth, scale=3.0)
    twin(xyz1b, xyz2b, q1, q2)
    (first * r).sum().backward()
    _assert_block_grads(twin, p1b, p2b, want)
    assert all(int(bn.num_batches_tracked) == int(state[f"mlp_bns.{l}.num_batches_tracked"]) + 2 for l, bn in enumerate(twin.mlp_bns))
    assert not torch.equal(twin.mlp_bns[0].running_mean, fp.mlp_bns[0].running_mean)
    # no graph under no_grad, or with grad=False: the statistics still move, as torch's do
    for mod, ctx in ((_block(state, batch_stats=True, grad=True), torch.no_grad()), (_block(state, batch_stats=True), torch.enable_grad())):
        with ctx:
            quiet = mod(xyz1, xyz2, p1, p2)
        assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, out.detach())
        for l, bn in enumerate(mod.mlp_bns):
            assert torch.equal(bn.running_mean, layers[l][4]) and torch.equal(bn.running_var, layers[l][5])
            assert int(bn.num_batches_tracked) == int(state[f"mlp_bns.{l}.num_batches_tracked"]) + 1
    none = _block(state, batch_stats=True, grad=True)
    none.mlp_bns[0].momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        none(xyz1, xyz2, p1, p2)
    with pytest.raises(NotImplementedError, match="eval mode"):
        _block(state, grad=True)(xyz1, xyz2, p1, p2)                  # without the flag train mode raises as before


def _loss(model, x, r, q):
    glob, l0 = model(x)
    return (l0 * r).sum() + (glob * q).sum()


def _targets(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((T.B, 128, T.N), generator=g).cuda() - 0.5, torch.rand((T.B, 128), generator=g).cuda() - 0.5


@pytest.mark.parametrize("encoder_grad", [False, True])
def test_one_training_step_of_the_model(synth, encoder_grad):
    x = T.model_input(synth)
    model = T.model(decoder_grad=True, encoder_grad=encoder_grad, decoder_batch_stats=True)
    assert model.train() is model and model.training
    assert all(not getattr(model, n).training for n in SA_BLOCKS) and all(getattr(model, n).training for n in FP_BLOCKS)
    assert model.conv1.training
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    r, q = _targets(11)
    _loss(model, x, r, q).backward()
    for k, v in model.named_buffers():
        if k.startswith(SA_BLOCKS):
            assert torch.equal(v, buffers[k]), k                      # the encoder's statistics stay frozen, bit for bit
        else:
            assert k.startswith(FP_BLOCKS) and not torch.equal(v, buffers[k]), k
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(buffers[k]) + 1, k
    for name, p in model.named_parameters():
        if name.startswith(SA_BLOCKS) and not encoder_grad:
            assert p.grad is None, name
        else:
            assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), name
    if encoder_grad:
        assert all(any((p.grad != 0).any() for p in getattr(model, n).parameters()) for n in SA_BLOCKS)
    assert model.eval() is model and not any(m.training for m in model.modules())
    model.train()
    model.fp2.eval()
    with pytest.raises(NotImplementedError, match="model's mode"):
        model(x)
    model.train()
    model.sa1.train()
    with pytest.raises(NotImplementedError, match="train mode"):
        model(x)


def test_fp2_inside_the_training_model_is_the_c_abi(synth):
    x = T.model_input(synth)
    model = T.model(decoder_grad=True, decoder_batch_stats=True).train()
    seen = {}
    inner = model.fp2._forward_rows
    state = {k: v.clone() for k, v in model.fp2.state_dict().items()}

    def spy(x1, x2, p1, p2):
        out = inner(x1, x2, p1, p2)
        seen.update(x1=x1.detach(), x2=x2.detach(), p1=p1.detach(), p2=p2.detach(), out=out.detach())
        out.register_hook(lambda g: seen.__setitem__("dout", g.detach().clone()))
        p2.register_hook(lambda g: seen.__setitem__("dp2", g.detach().clone()))
        return out

    model.fp2._forward_rows = spy
    r, q = _targets(13)
    _loss(model, x, r, q).backward()
    out, layers, want = _direct(state, 2, [bn.eps for bn in model.fp2.mlp_bns], seen["x1"], seen["x2"], seen["p1"], seen["p2"], seen["dout"])
    assert torch.equal(out, seen["out"]) and torch.equal(want["dp2"], seen["dp2"])
    for l, (conv, bn) in enumerate(zip(model.fp2.mlp_convs, model.fp2.mlp_bns)):
        dW, dbias, dgamma, dbeta = want["grads"][l]
        assert torch.equal(conv.weight.grad.reshape(dW.shape), dW) and torch.equal(conv.bias.grad, dbias) and (dbias == 0).all(), l
        assert torch.equal(bn.weight.grad, dgamma) and torch.equal(bn.bias.grad, dbeta) and (dgamma != 0).any(), l
        assert torch.equal(bn.running_mean, layers[l][4]) and torch.equal(bn.running_var, layers[l][5]), l


def test_sgd_on_a_fixed_batch_is_reproducible_and_eval_follows_the_state(synth):
    x = T.model_input(synth)
    g = torch.Generator().manual_seed(12)
    target, target_g = torch.rand((T.B, 128, T.N), generator=g).cuda(), torch.rand((T.B, 128), generator=g).cuda()

    def run(state):
        model = T.model(state, decoder_grad=True, decoder_batch_stats=True).train()
        opt = torch.optim.SGD([p for n, p in model.named_parameters() if n.startswith(FP_BLOCKS + ("conv1.",))], lr=1e-2)
        losses = []
        for _ in range(5):
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
    print("losses over five train-mode SGD steps:", losses)
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses == again
    with torch.no_grad():
        glob, l0 = model.eval()(x)
        glob_d, l0_d = T.model(model.state_dict())(x)                 # a default pointnet_2 with the trained state
    assert torch.equal(glob, glob_d) and torch.equal(l0, l0_d)


def test_the_flag_needs_decoder_grad():
    M = sub("pointNet.model.pointnetAtt")
    with pytest.raises(ValueError, match="decoder_grad"):
        M.pointnet_2(5, decoder_batch_stats=True)
    with pytest.raises(ValueError, match="decoder_grad"):
        M.pointnet_2(5, encoder_grad=True, decoder_batch_stats=True)
