"""PointNetSetAbstraction(..., group_all=True) on the GPU: shapes, the state_dict, the eval forward against the C ABI, autograd through
grad=True, what it refuses -- and a group_all=False block beside it, which must give the bits it always gave."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402

pytestmark = pytest.mark.gpu

B, N, D = 2, 70, 9


def _randomise(mod, seed):
    """Seeded values for every parameter and BatchNorm buffer (fresh running statistics would make bn_eval almost the identity)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in mod.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var") or (k.startswith("mlp_bns") and k.endswith("weight")):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * (0.6 if v.dim() == 1 else 2.0 / v.shape[1] ** 0.5)
    mod.load_state_dict(sd)
    return sd


def _inputs(synth, seed=41):
    xyz = torch.from_numpy(synth.clouds(seed, B, N)).cuda().transpose(1, 2).contiguous()                    # [B, 3, N]
    points = torch.from_numpy(synth.uniform(seed + 1, (B, N, D), -1.0, 1.0)).cuda().transpose(1, 2).contiguous()
    return xyz, points


def _layers(sa):
    M = sub("pointNet.model.pointnet2_utils")
    return M._mlp_tensors(sa), [bn.eps for bn in sa.mlp_bns]


def test_group_all_forward_shapes_and_values(synth):
    M, L = sub("pointNet.model.pointnet2_utils"), sub("_lib")
    sa = M.PointNetSetAbstraction(None, None, None, D + 3, [32, 32, 64], True).eval()
    assert sa.group_all is True
    _randomise(sa, 7)
    xyz, points = _inputs(synth)
    new_xyz, new_points = sa(xyz, points)
    assert new_xyz.shape == (B, 3, 1) and new_points.shape == (B, 64, 1)
    assert new_xyz.dtype == torch.float32 and (new_xyz == 0).all() and not new_points.requires_grad
    x, feats = xyz.transpose(1, 2).contiguous(), points.transpose(1, 2).contiguous()
    rows_xyz, rows = sa._forward_rows(x, feats)
    assert rows_xyz.shape == (B, 1, 3) and (rows_xyz == 0).all() and rows.shape == (B, 1, 64)
    assert torch.equal(rows[:, 0], new_points[:, :, 0])
    layers, eps = _layers(sa)
    out = torch.full((B, 64), float("nan"), device="cuda")
    ws = torch.empty(L.sa_all_forward_workspace_bytes(D, B, N, [32, 32, 64]), dtype=torch.uint8, device="cuda")
    L.sa_all_forward_f32(x, feats, layers, eps, out, ws)
    assert torch.equal(out, new_points[:, :, 0]) and (out > 0).any()
    # the plain float32 composition, loosely: the bars are the kernel tests' business
    h = torch.cat([x, feats], -1)
    for (w, b, g, beta, mean, var), e in zip(layers, eps):
        h = torch.relu((h @ w.T + b - mean) / torch.sqrt(var + e) * g + beta)
    assert torch.allclose(h.amax(1), out, rtol=1e-4, atol=1e-5)
    none = M.PointNetSetAbstraction(None, None, None, 3, [32], True).eval()      # in_channel = 3: no point features
    assert none(xyz, None)[1].shape == (B, 32, 1)
    one = none(xyz[:, :, :1].contiguous(), None)                                 # a cloud of one point
    assert one[1].shape == (B, 32, 1) and torch.isfinite(one[1]).all()


def test_group_all_state_dict_keys_and_round_trip():
    M = sub("pointNet.model.pointnet2_utils")
    sa = M.PointNetSetAbstraction(None, None, None, 12, [32, 64], True)
    want = {}
    for i, (cin, cout) in enumerate([(12, 32), (32, 64)]):
        want[f"mlp_convs.{i}.weight"] = (cout, cin, 1, 1)
        want[f"mlp_convs.{i}.bias"] = (cout,)
        for k in ("weight", "bias", "running_mean", "running_var"):
            want[f"mlp_bns.{i}.{k}"] = (cout,)
        want[f"mlp_bns.{i}.num_batches_tracked"] = ()
    assert {k: tuple(v.shape) for k, v in sa.state_dict().items()} == want
    usual = torch.nn.ModuleDict({"mlp_convs": torch.nn.ModuleList([torch.nn.Conv2d(12, 32, 1), torch.nn.Conv2d(32, 64, 1)]),
                                 "mlp_bns": torch.nn.ModuleList([torch.nn.BatchNorm2d(32), torch.nn.BatchNorm2d(64)])})
    assert {k: tuple(v.shape) for k, v in usual.state_dict().items()} == want
    src = _randomise(M.PointNetSetAbstraction(None, None, None, 12, [32, 64], True), 5)
    sa.load_state_dict({k: v.cpu() for k, v in src.items()})                     # strict: every key is there, none is extra
    for k, v in sa.state_dict().items():
        assert torch.equal(v.cpu(), src[k].cpu()), k
    usual.load_state_dict({k: v.cpu() for k, v in sa.state_dict().items()})      # and a torch model takes them back


def test_group_all_autograd_and_one_sgd_step(synth):
    M = sub("pointNet.model.pointnet2_utils")
    sa = M.PointNetSetAbstraction(None, None, None, D + 3, [32, 64], True, grad=True).eval()
    _randomise(sa, 8)
    xyz, points = _inputs(synth)
    points.requires_grad_(True)
    with torch.no_grad():
        assert not sa(xyz, points)[1].requires_grad                              # no_grad: no graph
    plain = M.PointNetSetAbstraction(None, None, None, D + 3, [32, 64], True).eval()
    plain.load_state_dict(sa.state_dict())
    assert not plain(xyz, points)[1].requires_grad                               # grad=False: no graph, ever
    new_xyz, before = sa(xyz, points)
    assert before.requires_grad and not new_xyz.requires_grad and torch.equal(before.detach(), plain(xyz, points)[1])
    weight = torch.from_numpy(synth.uniform(43, (B, 64, 1), -1.0, 1.0)).cuda()
    (before * weight).sum().backward()
    assert points.grad.shape == points.shape and torch.isfinite(points.grad).all()
    touched = (points.grad != 0).any(1)                                          # [B, N]: only rows that won a channel carry a gradient
    assert touched.any() and (touched.sum(1) <= 64).all() and not touched.all()
    for name, p in sa.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.shape == p.shape, name
        assert (p.grad != 0).any(), name
    # against torch's own autograd of the float32 composition, loosely (ties between rows are not expected in seeded inputs)
    ref = [t.detach().clone().requires_grad_(True) for t in sa.parameters()]
    pr = points.detach().clone().requires_grad_(True)
    h = torch.cat([xyz.transpose(1, 2), pr.transpose(1, 2)], -1)
    for l, bn in enumerate(sa.mlp_bns):
        w, b, g, beta = ref[2 * l], ref[2 * l + 1], ref[4 + 2 * l], ref[4 + 2 * l + 1]
        h = torch.relu((h @ w.reshape(w.shape[0], -1).T + b - bn.running_mean) / torch.sqrt(bn.running_var + bn.eps) * g + beta)
    (h.amax(1)[:, :, None] * weight).sum().backward()
    names = [n for n, _ in sa.named_parameters()]
    assert names == ["mlp_convs.0.weight", "mlp_convs.0.bias", "mlp_convs.1.weight", "mlp_convs.1.bias", "mlp_bns.0.weight", "mlp_bns.0.bias",
                     "mlp_bns.1.weight", "mlp_bns.1.bias"]
    assert torch.allclose(points.grad, pr.grad, rtol=1e-3, atol=1e-5)
    for (n, p), r in zip(sa.named_parameters(), ref):
        assert torch.allclose(p.grad, r.grad, rtol=1e-3, atol=1e-4), n
    torch.optim.SGD(sa.parameters(), lr=0.05).step()
    with torch.no_grad():
        after = sa(xyz, points)[1]
    assert not torch.equal(after, before.detach())                               # one SGD step changes the output
    # parameters frozen, the input still gets its gradient
    for p in sa.parameters():
        p.requires_grad_(False)
    points.grad = None
    sa(xyz, points)[1].sum().backward()
    assert points.grad is not None and (points.grad != 0).any()


def test_group_all_refusals(synth):
    M, L = sub("pointNet.model.pointnet2_utils"), sub("_lib")
    xyz, points = _inputs(synth)
    sa = M.PointNetSetAbstraction(None, None, None, D + 3, [32], True)
    assert sa.training
    with pytest.raises(NotImplementedError, match="eval mode"):
        sa(xyz, points)                                                          # .train() raises as for any block without batch_stats
    sa.eval()
    with pytest.raises(L.AmpnetError, match="group_all"):
        sa(xyz, points, centres=torch.zeros((B, 1), dtype=torch.int32, device="cuda"))
    with pytest.raises(NotImplementedError, match="group_all.*train mode"):
        M.PointNetSetAbstraction(None, None, None, D + 3, [32], True, batch_stats=True)
    with pytest.raises(NotImplementedError, match="group_all"):
        M.PointNetSetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True)
    with pytest.raises(Exception):
        sa(xyz, None)                                                            # in_channel = 12 needs 9 feature rows
    with pytest.raises(Exception):
        sa(xyz.cpu(), points.cpu())                                              # no CPU path


def test_ball_query_block_beside_it_keeps_its_bits(synth):
    """group_all=False is untouched: the block's output is ampnet_sa_forward_f32 on its own centres and groups, bit for bit."""
    M, L, U = sub("pointNet.model.pointnet2_utils"), sub("_lib"), sub("utils.utils")
    glob = M.PointNetSetAbstraction(None, None, None, D + 3, [32, 64], True).eval()
    sa = M.PointNetSetAbstraction(16, 0.3, 32, D + 3, [32, 64], False).eval()
    assert sa.group_all is False and (sa.npoint, sa.radius, sa.nsample) == (16, 0.3, 32)
    _randomise(sa, 9)
    glob.load_state_dict(sa.state_dict())
    xyz, points = _inputs(synth)
    glob(xyz, points)
    new_xyz, new_points = sa(xyz, points)
    x, feats = xyz.transpose(1, 2).contiguous(), points.transpose(1, 2).contiguous()
    cent = U.fps_indices(x, 16)
    gi = U.ball_query(x, cent, 0.3, 32)
    layers, eps = _layers(sa)
    out = torch.full((B, 16, 64), float("nan"), device="cuda")
    L.sa_forward_f32(x, cent, gi, feats, layers, eps, out, torch.empty(L.SA_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda"))
    assert torch.equal(out.transpose(1, 2), new_points) and new_points.shape == (B, 64, 16)
    assert torch.equal(new_xyz, U.gather_rows(x, cent).transpose(1, 2))
    with pytest.raises(NotImplementedError, match="nsample <= 64"):
        M.PointNetSetAbstraction(16, 0.3, 65, D + 3, [32], False)                # the same message as before
