"""pointNet/model/pointnet2_utils.py::PointNetFeaturePropagation and pointNet/model/pointnetAtt.py::pointnet_2: the usual constructors and
state_dict keys, eval forwards against the restatements of tests/sa_ref.py and tests/fp_ref.py, and the limits that raise."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import sub                           # noqa: E402
import fp_ref                                      # noqa: E402
import sa_ref                                      # noqa: E402

pytestmark = pytest.mark.gpu


def _randomise(mod, seed):
    """Seeded values for every parameter and BatchNorm buffer (fresh running statistics would make bn_eval almost the identity)."""
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
    return sd


def _layers(sd, prefix, n):
    """The six numpy arrays per layer of the block `prefix` of a state dict, weight as [cout, cin]."""
    out = []
    for i in range(n):
        w = sd[f"{prefix}mlp_convs.{i}.weight"].cpu().numpy()
        out.append((w.reshape(w.shape[0], -1),) + tuple(sd[prefix + k].cpu().numpy() for k in (
            f"mlp_convs.{i}.bias", f"mlp_bns.{i}.weight", f"mlp_bns.{i}.bias", f"mlp_bns.{i}.running_mean", f"mlp_bns.{i}.running_var")))
    return out


def _usual_block(conv, bn, cin, mlp):
    """The two ModuleLists of torch layers the usual implementation's blocks hold."""
    return torch.nn.ModuleDict({"mlp_convs": torch.nn.ModuleList([conv(a, b, 1) for a, b in zip([cin] + mlp[:-1], mlp)]),
                                "mlp_bns": torch.nn.ModuleList([bn(b) for b in mlp])})


def _rows(t):
    """[B, C, N] GPU -> [B, N, C] numpy."""
    return np.ascontiguousarray(t.detach().cpu().numpy().transpose(0, 2, 1))


def test_fp_state_dict_keys_shapes_and_round_trip():
    M = sub("pointNet.model.pointnet2_utils")
    fp = M.PointNetFeaturePropagation(384, [256, 256])
    want = {}
    for i, (cin, cout) in enumerate([(384, 256), (256, 256)]):
        want[f"mlp_convs.{i}.weight"] = (cout, cin, 1)
        want[f"mlp_convs.{i}.bias"] = (cout,)
        for k in ("weight", "bias", "running_mean", "running_var"):
            want[f"mlp_bns.{i}.{k}"] = (cout,)
        want[f"mlp_bns.{i}.num_batches_tracked"] = ()
    sd = fp.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(v.is_cuda for v in sd.values())
    usual = _usual_block(torch.nn.Conv1d, torch.nn.BatchNorm1d, 384, [256, 256])
    assert {k: tuple(v.shape) for k, v in usual.state_dict().items()} == want
    src = _randomise(M.PointNetFeaturePropagation(384, [256, 256]), 5)
    fp.load_state_dict({k: v.cpu() for k, v in src.items()})                     # strict: every key is there, none is extra
    for k, v in fp.state_dict().items():
        assert torch.equal(v.cpu(), src[k].cpu()), k
    usual.load_state_dict({k: v.cpu() for k, v in fp.state_dict().items()})      # and a torch model takes them back
    fp.load_state_dict(usual.state_dict())


def test_fp_eval_forward_matches_the_restatement(synth):
    M = sub("pointNet.model.pointnet2_utils")
    U = sub("utils.utils")
    B, N, S, D1, D2 = 2, 200, 24, 16, 32
    fp = M.PointNetFeaturePropagation(D1 + D2, [64, 32]).eval()
    sd = _randomise(fp, 6)
    fine = synth.clouds(51, B, N)
    coarse = np.ascontiguousarray(fine[:, np.arange(S) * 8 + 3])                 # sampled from the fine points, as a set abstraction does
    p1, p2 = synth.uniform(52, (B, N, D1), -1.0, 1.0), synth.uniform(53, (B, S, D2), -1.0, 1.0)
    cm = lambda a: torch.from_numpy(a).cuda().transpose(1, 2).contiguous()       # channel-major, the module's interface
    got_idx, got_d = (t.cpu().numpy() for t in U.three_nn(torch.from_numpy(fine).cuda(), torch.from_numpy(coarse).cuda()))
    out = fp(cm(fine), cm(coarse), cm(p1), cm(p2))
    assert out.shape == (B, 32, N)
    layers = _layers(sd, "", 2)
    none = M.PointNetFeaturePropagation(D2, [32]).eval()                          # in_channel = D2: points1 = None
    sd_none = _randomise(none, 7)
    out_none = none(cm(fine), cm(coarse), None, cm(p2))
    assert out_none.shape == (B, 32, N)
    worst = worst_none = 0.0
    for c in range(B):
        idx, d2 = fp_ref.three_nn(fine[c], coarse[c])
        assert got_idx[c].tobytes() == idx.tobytes() and got_d[c].tobytes() == d2.tobytes()       # the neighbours match bit for bit
        assert (d2[:, 0] == 0).sum() == S
        want, bar = fp_ref.fp_forward(p1[c], p2[c], idx, d2, layers, [1e-5] * 2)
        worst = max(worst, float(np.max(np.abs(_rows(out)[c].astype(np.float64) - want) / np.maximum(bar, 1e-300))))
        want, bar = fp_ref.fp_forward(None, p2[c], idx, d2, _layers(sd_none, "", 1), [1e-5])
        worst_none = max(worst_none, float(np.max(np.abs(_rows(out_none)[c].astype(np.float64) - want) / np.maximum(bar, 1e-300))))
    print(f"PointNetFeaturePropagation eval forward: worst error / bar = {worst:.3f}, with points1=None {worst_none:.3f}")
    assert worst <= 1.0 and worst_none <= 1.0, (worst, worst_none)


def test_fp_limits_raise(synth):
    M, L = sub("pointNet.model.pointnet2_utils"), sub("_lib")
    for in_channel, mlp in ((48, [48]), (48, [32, 288]), (513, [32]), (0, [32]), (48, [32, 32, 32, 32]), (48, [])):
        with pytest.raises(NotImplementedError, match="multiples of 32"):
            M.PointNetFeaturePropagation(in_channel, mlp)
    fp = M.PointNetFeaturePropagation(48, [32])
    assert fp.training
    xyz1 = torch.from_numpy(synth.clouds(54, 1, 64)).cuda().transpose(1, 2).contiguous()
    xyz2 = xyz1[:, :, :8].contiguous()
    p1, p2 = torch.zeros((1, 16, 64), device="cuda"), torch.zeros((1, 32, 8), device="cuda")
    with pytest.raises(NotImplementedError, match="eval mode"):
        fp(xyz1, xyz2, p1, p2)
    fp.eval()
    assert fp(xyz1, xyz2, p1, p2).shape == (1, 32, 64)
    with pytest.raises(L.AmpnetError):
        fp(xyz1, xyz2, None, p2)                                                 # in_channel = 48 needs 16 rows of points1
    with pytest.raises(L.AmpnetError):
        fp(xyz1, xyz2, p1[:, :15], p2)
    with pytest.raises(L.AmpnetError):
        fp(xyz1, xyz2, p1, p2[:, :, :7])                                         # points2 of another S
    with pytest.raises(L.AmpnetError):
        fp(xyz1, xyz2[:1, :2], p1, p2)
    with pytest.raises(L.AmpnetError):
        fp(xyz1.cpu(), xyz2.cpu(), p1.cpu(), p2.cpu())                           # no CPU path
    with pytest.raises(L.AmpnetError):
        fp(xyz1, xyz2, p1, p2.cpu())


def test_pointnet_2_state_dict_is_the_reference_class_on_torch_layers():
    M = sub("pointNet.model.pointnetAtt")
    model = M.pointnet_2(5)
    c2, b2, c1, b1 = torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.Conv1d, torch.nn.BatchNorm1d
    usual = torch.nn.ModuleDict({"sa1": _usual_block(c2, b2, 9 + 3, [32, 32, 64]), "sa2": _usual_block(c2, b2, 64 + 3, [64, 64, 128]),
                                 "sa3": _usual_block(c2, b2, 128 + 3, [128, 128, 256]), "fp3": _usual_block(c1, b1, 384, [256, 256]),
                                 "fp2": _usual_block(c1, b1, 320, [256, 128]), "fp1": _usual_block(c1, b1, 128, [128, 128, 128]),
                                 "conv1": torch.nn.Conv1d(128, 128, 1)})
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes(model) == shapes(usual) and len(shapes(model)) == 16 * 7 + 2
    assert (model.sa1.npoint, model.sa1.radius, model.sa1.nsample) == (1024, 0.1, 32)
    assert (model.sa2.npoint, model.sa2.radius, model.sa3.npoint, model.sa3.radius) == (256, 0.2, 64, 0.4)
    model.load_state_dict(usual.state_dict())                                    # strict, both ways
    usual.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})


def test_pointnet_2_eval_forward_block_by_block(synth):
    """The reference's sizes with fewer centres and larger balls (B = 2, N = 512; 128 / 32 / 8 centres), every block against its
    restatement on the block's OWN inputs as the chain produced them, so each bar is that of one block."""
    M = sub("pointNet.model.pointnetAtt")
    U = sub("utils.utils")
    B, N = 2, 512
    model = M.pointnet_2(5).eval()
    for sa, npoint, radius in ((model.sa1, 128, 0.2), (model.sa2, 32, 0.4), (model.sa3, 8, 0.8)):
        sa.npoint, sa.radius = npoint, radius
    sd = _randomise(model, 8)
    x_np = np.concatenate([synth.clouds(55, B, N), synth.uniform(56, (B, N, 6), -1.0, 1.0)], -1)        # [B, N, 9]
    x = torch.from_numpy(x_np).cuda().transpose(1, 2).contiguous()                                    # [B, 9, N]
    glob, l0_points = model(x)
    assert glob.shape == (B, 128) and l0_points.shape == (B, 128, N)
    assert torch.isfinite(glob).all() and torch.isfinite(l0_points).all() and (l0_points > 0).any()
    assert torch.equal(glob, model.conv1(l0_points).amax(2))
    assert not torch.equal(l0_points[0], l0_points[1])
    # the same chain through the blocks' public, channel-major interface: the layout kept between the blocks inside the model changes nothing
    l0_xyz = x[:, :3, :].contiguous()
    l1_xyz, l1_p = model.sa1(l0_xyz, x)
    l2_xyz, l2_p = model.sa2(l1_xyz, l1_p)
    l3_xyz, l3_p = model.sa3(l2_xyz, l2_p)
    f2 = model.fp3(l2_xyz, l3_xyz, l2_p, l3_p)
    f1 = model.fp2(l1_xyz, l2_xyz, l1_p, f2)
    f0 = model.fp1(l0_xyz, l1_xyz, None, f1)
    assert (l1_p.shape, l2_p.shape, l3_p.shape) == ((B, 64, 128), (B, 128, 32), (B, 256, 8))
    assert (f2.shape, f1.shape) == ((B, 256, 32), (B, 128, 128))
    assert torch.equal(f0, l0_points)
    ratios = {}
    # set abstractions: the model's centres are the project's FPS from point 0, its groups the ball query's
    for name, sa, xyz_in, p_in, xyz_out, p_out in (("sa1", model.sa1, l0_xyz, x, l1_xyz, l1_p), ("sa2", model.sa2, l1_xyz, l1_p, l2_xyz, l2_p),
                                                   ("sa3", model.sa3, l2_xyz, l2_p, l3_xyz, l3_p)):
        pts, feats = _rows(xyz_in), _rows(p_in)
        cent = U.fps_indices(torch.from_numpy(pts).cuda(), sa.npoint)
        grp = U.ball_query(torch.from_numpy(pts).cuda(), cent, sa.radius, sa.nsample).cpu().numpy()
        cent = cent.cpu().numpy()
        worst = 0.0
        for c in range(B):
            idx, _ = sa_ref.ball_query(pts[c], cent[c], sa.radius, sa.nsample)
            assert np.array_equal(grp[c], idx), name
            assert np.array_equal(_rows(xyz_out)[c], pts[c][cent[c]]), name
            want, bar = sa_ref.sa_forward(pts[c], cent[c], idx, feats[c], _layers(sd, name + ".", 3), [1e-5] * 3)
            worst = max(worst, float(np.max(np.abs(_rows(p_out)[c].astype(np.float64) - want) / np.maximum(bar, 1e-300))))
        ratios[name] = worst
    # feature propagations: the neighbours bit for bit, then the fused layer
    for name, n_layers, xyz1, xyz2, p1, p2, out in (("fp3", 2, l2_xyz, l3_xyz, l2_p, l3_p, f2), ("fp2", 2, l1_xyz, l2_xyz, l1_p, f2, f1),
                                                    ("fp1", 3, l0_xyz, l1_xyz, None, f1, l0_points)):
        fine, coarse = _rows(xyz1), _rows(xyz2)
        got_idx, got_d = (t.cpu().numpy() for t in U.three_nn(torch.from_numpy(fine).cuda(), torch.from_numpy(coarse).cuda()))
        worst = 0.0
        for c in range(B):
            idx, d2 = fp_ref.three_nn(fine[c], coarse[c])
            assert got_idx[c].tobytes() == idx.tobytes() and got_d[c].tobytes() == d2.tobytes(), name
            assert (d2[:, 0] == 0).sum() >= coarse.shape[1], name                # every coarse point is one of the fine points
            want, bar = fp_ref.fp_forward(None if p1 is None else _rows(p1)[c], _rows(p2)[c], idx, d2, _layers(sd, name + ".", n_layers),
                                          [1e-5] * n_layers)
            worst = max(worst, float(np.max(np.abs(_rows(out)[c].astype(np.float64) - want) / np.maximum(bar, 1e-300))))
        ratios[name] = worst
    print("pointnet_2 eval forward, worst error / bar per block: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def test_pointnet_2_train_mode_raises(synth):
    M = sub("pointNet.model.pointnetAtt")
    model = M.pointnet_2(5)
    assert model.training
    x = torch.zeros((1, 9, 64), device="cuda")
    with pytest.raises(NotImplementedError, match="pointnet_2"):
        model(x)
    model.eval()
    model.fp1.train()
    with pytest.raises(NotImplementedError, match="pointnet_2"):
        model(x)
    with pytest.raises(sub("_lib").AmpnetError):
        model.eval()(x.cpu())
