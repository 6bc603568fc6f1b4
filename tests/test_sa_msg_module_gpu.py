"""PointNetSetAbstractionMsg on the GPU: the state_dict of the usual implementation, shapes, the eval forward against K single-scale
blocks (bit for bit) and against a plain torch composition in the usual [features, relative xyz] row order, autograd through grad=True,
train-mode BatchNorm through batch_stats=True, what it refuses -- and a PointNetSetAbstraction block beside it, which keeps its bits."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402

pytestmark = pytest.mark.gpu

B, N, D, S = 2, 70, 6, 9
RADII, NSAMPLES, MLPS = [0.3, 0.6, 0.45], [20, 48, 32], [[32, 64], [32, 32, 64], [32]]
C_OUT = 64 + 64 + 32


def _randomise(mod, seed):
    """Seeded values for every parameter and BatchNorm buffer (fresh running statistics would make bn_eval almost the identity)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in mod.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var") or (k.split(".")[0] in ("mlp_bns", "bn_blocks") and k.endswith("weight")):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * (0.6 if v.dim() == 1 else 2.0 / v.shape[1] ** 0.5)
    mod.load_state_dict(sd)
    return sd


def _inputs(synth, seed=41, d=D):
    xyz = torch.from_numpy(synth.clouds(seed, B, N)).cuda().transpose(1, 2).contiguous()                    # [B, 3, N]
    points = torch.from_numpy(synth.uniform(seed + 1, (B, N, d), -1.0, 1.0)).cuda().transpose(1, 2).contiguous() if d else None
    return xyz, points


def _msg(M, **kw):
    return M.PointNetSetAbstractionMsg(S, RADII, NSAMPLES, D, MLPS, **kw)


def _usual(msg, xyz, points, params, buffers, training):
    """The usual MSG block in plain float32 torch on this module's centres and groups: gather, cat([features, relative xyz]) in THAT
    order, per layer 1x1 conv, batch norm and relu, max over the group, cat over the branches.  params / buffers: name -> tensor."""
    U = sub("utils.utils")
    x = xyz.transpose(1, 2).contiguous()
    cent = U.fps_indices(x, msg.npoint)
    new = U.gather_rows(x, cent)
    b_idx = torch.arange(x.shape[0], device=x.device)[:, None, None]
    outs = []
    for i, (radius, nsample) in enumerate(zip(msg.radius_list, msg.nsample_list)):
        gi = U.ball_query(x, cent, radius, nsample).long()
        h = x[b_idx, gi] - new[:, :, None, :]                                       # [B, S, nsample, 3]
        if points is not None:
            h = torch.cat([points.transpose(1, 2)[b_idx, gi], h], -1)               # features first
        h = h.permute(0, 3, 2, 1)                                                   # [B, C, nsample, S]
        for j, bn in enumerate(msg.bn_blocks[i]):
            h = F.conv2d(h, params[f"conv_blocks.{i}.{j}.weight"], params[f"conv_blocks.{i}.{j}.bias"])
            h = F.batch_norm(h, buffers[f"bn_blocks.{i}.{j}.running_mean"], buffers[f"bn_blocks.{i}.{j}.running_var"],
                             params[f"bn_blocks.{i}.{j}.weight"], params[f"bn_blocks.{i}.{j}.bias"], training, bn.momentum, bn.eps)
            h = torch.relu(h)
        outs.append(h.amax(2))                                                      # [B, C, S]
    return torch.cat(outs, 1)


def _clones(msg):
    return ({k: v.detach().clone().requires_grad_(True) for k, v in msg.named_parameters()},
            {k: v.detach().clone() for k, v in msg.named_buffers()})


def test_state_dict_keys_and_round_trip():
    M = sub("pointNet.model.pointnet2_utils")
    msg = _msg(M)
    assert msg.npoint == S and msg.radius_list == RADII and msg.nsample_list == NSAMPLES
    usual = torch.nn.ModuleDict({"conv_blocks": torch.nn.ModuleList(), "bn_blocks": torch.nn.ModuleList()})
    for mlp in MLPS:
        convs, bns, last = torch.nn.ModuleList(), torch.nn.ModuleList(), D + 3
        for c in mlp:
            convs.append(torch.nn.Conv2d(last, c, 1))
            bns.append(torch.nn.BatchNorm2d(c))
            last = c
        usual["conv_blocks"].append(convs)
        usual["bn_blocks"].append(bns)
    want = {k: tuple(v.shape) for k, v in usual.state_dict().items()}
    assert want["conv_blocks.1.0.weight"] == (32, D + 3, 1, 1) and want["bn_blocks.1.2.num_batches_tracked"] == ()
    assert {k: tuple(v.shape) for k, v in msg.state_dict().items()} == want
    src = _randomise(_msg(M), 5)
    msg.load_state_dict({k: v.cpu() for k, v in src.items()})                        # strict: every key is there, none is extra
    for k, v in msg.state_dict().items():
        assert torch.equal(v.cpu(), src[k].cpu()), k
    usual.load_state_dict({k: v.cpu() for k, v in msg.state_dict().items()})         # and a torch model takes them back
    msg.load_state_dict(usual.state_dict())


def test_eval_forward(synth):
    M, U = sub("pointNet.model.pointnet2_utils"), sub("utils.utils")
    msg = _msg(M).eval()
    _randomise(msg, 7)
    xyz, points = _inputs(synth)
    new_xyz, new_points = msg(xyz, points)
    assert new_xyz.shape == (B, 3, S) and new_points.shape == (B, C_OUT, S)
    assert new_xyz.dtype == torch.float32 and new_points.dtype == torch.float32 and not new_points.requires_grad
    assert torch.isfinite(new_points).all() and (new_points > 0).any()
    x = xyz.transpose(1, 2).contiguous()
    cent = U.fps_indices(x, S)
    assert torch.equal(new_xyz, U.gather_rows(x, cent).transpose(1, 2))
    # centres= is honoured
    other = torch.stack([torch.arange(S, dtype=torch.int32) * 7 + c for c in range(B)]).cuda()
    o_xyz, o_points = msg(xyz, points, centres=other)
    assert torch.equal(o_xyz, U.gather_rows(x, other).transpose(1, 2)) and not torch.equal(o_points, new_points)
    assert torch.equal(msg(xyz, points, centres=cent)[1], new_points)
    # K single-scale blocks loaded with the rotated layer-0 weights: bit for bit
    off, sd = 0, msg.state_dict()
    for i, (radius, nsample, mlp) in enumerate(zip(RADII, NSAMPLES, MLPS)):
        sa = M.PointNetSetAbstraction(S, radius, nsample, D + 3, mlp, False).eval()
        part = {k.replace(f"conv_blocks.{i}.", "mlp_convs.").replace(f"bn_blocks.{i}.", "mlp_bns."): v
                for k, v in sd.items() if k.split(".")[1] == str(i)}
        w = part["mlp_convs.0.weight"]
        part["mlp_convs.0.weight"] = torch.cat([w[:, D:], w[:, :D]], 1)
        sa.load_state_dict(part)
        assert torch.equal(sa(xyz, points)[1], new_points[:, off:off + mlp[-1]]), i
        off += mlp[-1]
    # the usual block in plain float32 torch, features first: pins the column order
    params, buffers = _clones(msg)
    with torch.no_grad():
        want = _usual(msg, xyz, points, params, buffers, False)
    assert torch.allclose(new_points, want, rtol=1e-4, atol=1e-5)
    # no point features: the row is the relative xyz alone
    bare = M.PointNetSetAbstractionMsg(S, RADII[:2], NSAMPLES[:2], 0, MLPS[:2]).eval()
    _randomise(bare, 8)
    with torch.no_grad():
        want = _usual(bare, xyz, None, *_clones(bare), False)
    got = bare(xyz, None)[1]
    assert got.shape == (B, 128, S) and torch.allclose(got, want, rtol=1e-4, atol=1e-5)


def test_autograd_and_one_sgd_step(synth):
    M = sub("pointNet.model.pointnet2_utils")
    msg = _msg(M, grad=True).eval()
    _randomise(msg, 9)
    xyz, points = _inputs(synth)
    points.requires_grad_(True)
    with torch.no_grad():
        fused = msg(xyz, points)[1]
        assert not fused.requires_grad                                               # no_grad: no graph
    plain = _msg(M).eval()
    plain.load_state_dict(msg.state_dict())
    assert not plain(xyz, points)[1].requires_grad                                   # grad=False: no graph, ever
    new_xyz, before = msg(xyz, points)
    assert before.requires_grad and not new_xyz.requires_grad
    assert torch.equal(before.detach(), fused) and torch.equal(fused, plain(xyz, points)[1])
    weight = torch.from_numpy(synth.uniform(43, (B, C_OUT, S), -1.0, 1.0)).cuda()
    (before * weight).sum().backward()
    first = [points.grad.clone()] + [p.grad.clone() for p in msg.parameters()]
    for name, p in msg.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all() and (p.grad != 0).any(), name
    # torch's own autograd of the usual composition: layer 0's weight gradient is in the checkpoint's column order
    params, buffers = _clones(msg)
    pr = points.detach().clone().requires_grad_(True)
    (_usual(msg, xyz, pr, params, buffers, False) * weight).sum().backward()
    assert torch.allclose(points.grad, pr.grad, rtol=1e-3, atol=1e-4)
    for name, p in msg.named_parameters():
        assert torch.allclose(p.grad, params[name].grad, rtol=1e-3, atol=1e-4), name
    # a second backward: the same bits (K = 3 gradients to `points` are summed)
    points.grad = None
    msg.zero_grad(set_to_none=True)
    (msg(xyz, points)[1] * weight).sum().backward()
    for a, b in zip(first, [points.grad] + [p.grad for p in msg.parameters()]):
        assert torch.equal(a, b)
    torch.optim.SGD(msg.parameters(), lr=0.05).step()
    with torch.no_grad():
        after = msg(xyz, points)[1]
    assert not torch.equal(after, before.detach())                                   # one SGD step changes the output


def test_train_mode_batch_statistics(synth):
    M = sub("pointNet.model.pointnet2_utils")
    msg = _msg(M, grad=True, batch_stats=True)
    _randomise(msg, 10)
    assert msg.training
    xyz, points = _inputs(synth)
    points.requires_grad_(True)
    params, buffers = _clones(msg)
    start = {k: v.clone() for k, v in msg.named_buffers()}
    out = msg(xyz, points)[1]
    weight = torch.from_numpy(synth.uniform(44, (B, C_OUT, S), -1.0, 1.0)).cuda()
    (out * weight).sum().backward()
    pr = points.detach().clone().requires_grad_(True)
    want = _usual(msg, xyz, pr, params, buffers, True)                               # updates `buffers` as torch does
    (want * weight).sum().backward()
    assert torch.allclose(out, want, rtol=1e-4, atol=1e-5)
    assert torch.allclose(points.grad, pr.grad, rtol=1e-3, atol=1e-4)
    for name, p in msg.named_parameters():
        if name.startswith("conv_blocks") and name.endswith("bias"):
            assert (p.grad == 0).all(), name                                         # no effect on a batch-normalised output
        assert torch.allclose(p.grad, params[name].grad, rtol=1e-3, atol=1e-4), name
    for name, v in msg.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(v) == int(start[name]) + 1, name
        else:
            assert not torch.equal(v, start[name]), name                             # every branch's running statistics moved
            assert torch.allclose(v, buffers[name], rtol=1e-4, atol=1e-5), name
    with torch.no_grad():
        msg(xyz, points)                                                             # no graph: the statistics move all the same
    assert all(int(v) == int(start[k]) + 2 for k, v in msg.named_buffers() if k.endswith("num_batches_tracked"))
    # .eval() afterwards is the eval forward of the trained state
    msg.eval()
    fresh = _msg(M).eval()
    fresh.load_state_dict(msg.state_dict())
    assert torch.equal(msg(xyz, points)[1].detach(), fresh(xyz, points)[1])
    msg.bn_blocks[1][0].momentum = 0.2
    with pytest.raises(NotImplementedError, match="one float momentum"):
        msg.train()(xyz, points)


def test_refusals(synth):
    M, L = sub("pointNet.model.pointnet2_utils"), sub("_lib")
    xyz, points = _inputs(synth)
    msg = _msg(M)
    assert msg.training
    with pytest.raises(NotImplementedError, match="eval mode"):
        msg(xyz, points)                                                             # .train() raises without batch_stats
    msg.eval()
    with pytest.raises(NotImplementedError, match="one length"):
        M.PointNetSetAbstractionMsg(S, [0.1, 0.2], [8, 8, 8], D, [[32], [32]])
    with pytest.raises(NotImplementedError, match="one length"):
        M.PointNetSetAbstractionMsg(S, [0.1, 0.2], [8, 8], D, [[32]])
    with pytest.raises(NotImplementedError, match=f"1..{L.SA_MSG_MAX_SCALES}"):
        M.PointNetSetAbstractionMsg(S, [0.1] * 5, [8] * 5, D, [[32]] * 5)
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        M.PointNetSetAbstractionMsg(S, [0.1, 0.2], [8, 8], D, [[32], [32, 48]])
    with pytest.raises(NotImplementedError, match="nsample <= 64"):
        M.PointNetSetAbstractionMsg(S, [0.1, 0.2], [8, 65], D, [[32], [32]])
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        M.PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], 0, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])     # a stock MSG layer
    with pytest.raises(L.AmpnetError, match="points"):
        msg(xyz, points[:, :D - 1].contiguous())                                     # in_channel = 6 needs 6 feature rows
    with pytest.raises(L.AmpnetError, match="points"):
        msg(xyz, None)
    with pytest.raises(Exception):
        msg(xyz.cpu(), points.cpu())                                                 # no CPU path
    with pytest.raises(L.AmpnetError, match="centres"):
        msg(xyz, points, centres=torch.zeros((B, S + 1), dtype=torch.int32, device="cuda"))


def test_single_scale_block_beside_it_keeps_its_bits(synth):
    """PointNetSetAbstraction is untouched: its output is ampnet_sa_forward_f32 on its own centres and groups, bit for bit."""
    M, L, U = sub("pointNet.model.pointnet2_utils"), sub("_lib"), sub("utils.utils")
    msg = _msg(M).eval()
    sa = M.PointNetSetAbstraction(16, 0.3, 32, D + 3, [32, 64], False).eval()
    _randomise(sa, 9)
    xyz, points = _inputs(synth)
    msg(xyz, points)
    new_xyz, new_points = sa(xyz, points)
    x, feats = xyz.transpose(1, 2).contiguous(), points.transpose(1, 2).contiguous()
    cent = U.fps_indices(x, 16)
    gi = U.ball_query(x, cent, 0.3, 32)
    out = torch.full((B, 16, 64), float("nan"), device="cuda")
    L.sa_forward_f32(x, cent, gi, feats, M._mlp_tensors(sa), [bn.eps for bn in sa.mlp_bns], out,
                     torch.empty(L.SA_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda"))
    assert torch.equal(out.transpose(1, 2), new_points) and new_points.shape == (B, 64, 16)
    assert torch.equal(new_xyz, U.gather_rows(x, cent).transpose(1, 2))
