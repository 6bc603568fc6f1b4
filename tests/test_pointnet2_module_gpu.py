"""pointNet/model/pointnet2_utils.py::PointNetSetAbstraction: the usual PointNet++ constructor and state_dict keys, an eval forward
against the restatements of tests/sa_ref.py, a three-layer chain, and the limits that raise."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import sa_ref                                      # noqa: E402

pytestmark = pytest.mark.gpu


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


def test_state_dict_keys_shapes_and_round_trip():
    M = sub("pointNet.model.pointnet2_utils")
    sa = M.PointNetSetAbstraction(64, 0.2, 32, 9 + 3, [32, 32, 64], False)
    want = {}
    for i, (cin, cout) in enumerate([(12, 32), (32, 32), (32, 64)]):
        want[f"mlp_convs.{i}.weight"] = (cout, cin, 1, 1)
        want[f"mlp_convs.{i}.bias"] = (cout,)
        for k in ("weight", "bias", "running_mean", "running_var"):
            want[f"mlp_bns.{i}.{k}"] = (cout,)
        want[f"mlp_bns.{i}.num_batches_tracked"] = ()
    sd = sa.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(v.is_cuda for v in sd.values())
    # the same keys and shapes as the torch layers the usual implementation holds in its two ModuleLists
    usual = torch.nn.ModuleDict({"mlp_convs": torch.nn.ModuleList([torch.nn.Conv2d(a, b, 1) for a, b in [(12, 32), (32, 32), (32, 64)]]),
                                 "mlp_bns": torch.nn.ModuleList([torch.nn.BatchNorm2d(b) for b in (32, 32, 64)])})
    assert {k: tuple(v.shape) for k, v in usual.state_dict().items()} == want
    src = _randomise(M.PointNetSetAbstraction(64, 0.2, 32, 12, [32, 32, 64], False), 5)
    sa.load_state_dict({k: v.cpu() for k, v in src.items()})                     # strict: every key is there, none is extra
    for k, v in sa.state_dict().items():
        assert torch.equal(v.cpu(), src[k].cpu()), k
    usual.load_state_dict({k: v.cpu() for k, v in sa.state_dict().items()})      # and a torch model takes them back


def test_eval_forward_matches_the_restatement(synth):
    M = sub("pointNet.model.pointnet2_utils")
    U = sub("utils.utils")
    B, N, npoint, radius, nsample = 2, 512, 64, 0.2, 32
    sa = M.PointNetSetAbstraction(npoint, radius, nsample, 9 + 3, [32, 32, 64], False).eval()
    sd = _randomise(sa, 6)
    pc = synth.clouds(21, B, N)
    pts = synth.uniform(22, (B, N, 9), -1.0, 1.0)
    xyz = torch.from_numpy(pc).cuda().transpose(1, 2).contiguous()               # [B, 3, N]
    points = torch.from_numpy(pts).cuda().transpose(1, 2).contiguous()           # [B, 9, N]
    new_xyz, new_points = sa(xyz, points)
    assert new_xyz.shape == (B, 3, npoint) and new_points.shape == (B, 64, npoint)
    cent = U.fps_indices(torch.from_numpy(pc).cuda(), npoint)                    # the module's centres: the project's FPS, seed = point 0
    assert (cent[:, 0] == 0).all()
    given = sa(xyz, points, centres=cent)
    assert torch.equal(given[0], new_xyz) and torch.equal(given[1], new_points)
    cent = cent.cpu().numpy()
    got_idx = U.ball_query(torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda(), radius, nsample).cpu().numpy()
    layers = [tuple(sd[k].cpu().numpy().reshape(sd[k].shape[0], -1) if k.endswith("convs.%d.weight" % i) else sd[k].cpu().numpy()
                    for k in (f"mlp_convs.{i}.weight", f"mlp_convs.{i}.bias", f"mlp_bns.{i}.weight", f"mlp_bns.{i}.bias",
                              f"mlp_bns.{i}.running_mean", f"mlp_bns.{i}.running_var")) for i in range(3)]
    worst = 0.0
    for c in range(B):
        idx, cnt = sa_ref.ball_query(pc[c], cent[c], radius, nsample)
        assert np.array_equal(got_idx[c], idx)                                   # the groups match exactly
        assert (cnt < nsample).any() and (cnt > 1).any()                         # padded groups, and groups of more than the centre
        assert np.array_equal(new_xyz[c].cpu().numpy(), pc[c][cent[c]].T)
        want, bar = sa_ref.sa_forward(pc[c], cent[c], idx, pts[c], layers, [1e-5] * 3)
        worst = max(worst, float(np.max(np.abs(new_points[c].cpu().numpy().T.astype(np.float64) - want) / np.maximum(bar, 1e-300))))
    print(f"PointNetSetAbstraction eval forward: worst error / bar = {worst:.3f}")
    assert worst <= 1.0, worst
    other = torch.from_numpy(np.stack([np.arange(npoint) * 7 % N] * B).astype(np.int32)).cuda()      # other centres, other result
    o_xyz, o_points = sa(xyz, points, centres=other)
    assert np.array_equal(o_xyz[0].cpu().numpy(), pc[0][other[0].cpu().numpy()].T) and not torch.equal(o_points, new_points)


def test_three_layer_chain_shapes(synth):
    M = sub("pointNet.model.pointnet2_utils")
    B, N = 2, 512
    sa1 = M.PointNetSetAbstraction(128, 0.2, 32, 9 + 3, [32, 32, 64], False).eval()
    sa2 = M.PointNetSetAbstraction(32, 0.4, 32, 64 + 3, [64, 64, 128], False).eval()
    sa3 = M.PointNetSetAbstraction(8, 0.8, 32, 128 + 3, [128, 128, 256], False).eval()
    for i, m in enumerate((sa1, sa2, sa3)):
        _randomise(m, 30 + i)
    xyz = torch.from_numpy(synth.clouds(23, B, N)).cuda().transpose(1, 2).contiguous()
    points = torch.from_numpy(synth.uniform(24, (B, N, 9), -1.0, 1.0)).cuda().transpose(1, 2).contiguous()
    x1, p1 = sa1(xyz, points)
    x2, p2 = sa2(x1, p1)
    x3, p3 = sa3(x2, p2)
    assert (x1.shape, p1.shape) == ((B, 3, 128), (B, 64, 128))
    assert (x2.shape, p2.shape) == ((B, 3, 32), (B, 128, 32))
    assert (x3.shape, p3.shape) == ((B, 3, 8), (B, 256, 8))
    for t in (x1, p1, x2, p2, x3, p3):
        assert torch.isfinite(t).all()
    assert (p3 > 0).any()
    none = M.PointNetSetAbstraction(16, 0.5, 8, 3, [32], False).eval()           # in_channel = 3: no point features
    assert none(xyz, None)[1].shape == (B, 32, 16)


def test_limits_raise(synth):
    M = sub("pointNet.model.pointnet2_utils")
    with pytest.raises(NotImplementedError, match="group_all"):
        M.PointNetSetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True)
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        M.PointNetSetAbstraction(16, 0.2, 32, 12, [32, 48], False)
    sa = M.PointNetSetAbstraction(16, 0.2, 32, 12, [32], False)
    assert sa.training
    xyz = torch.from_numpy(synth.clouds(25, 1, 64)).cuda().transpose(1, 2).contiguous()
    points = torch.zeros((1, 9, 64), device="cuda")
    with pytest.raises(NotImplementedError, match="eval mode"):
        sa(xyz, points)
    sa.eval()
    assert sa(xyz, points)[1].shape == (1, 32, 16)
    with pytest.raises(Exception):
        sa(xyz, None)                                                            # in_channel = 12 needs 9 feature rows
    with pytest.raises(Exception):
        sa(xyz.cpu(), points.cpu())                                              # no CPU path
