"""The PointNet++ bindings on the GPU: every `*_f32` wrapper of _lib refuses a non-contiguous tensor, a wrong rank and a wrong dtype in
Python, by its own name and the argument's (the kernels take bare pointers and no strides: what a wrapper lets through is read wrongly
without any error), and each of the five autograd paths routes a gradient to the tensor that asked for one and to no other.  Values are
not at stake here: the float64 parity tests of every entry point are."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import sub                           # noqa: E402
import pn2_bindings_util as U                      # noqa: E402

pytestmark = pytest.mark.gpu

BROKEN = {
    "non-contiguous": lambda t: t.repeat_interleave(2, dim=-1)[..., ::2],       # the same shape and values on every other element
    "rank": lambda t: t.unsqueeze(0),
    "dtype": lambda t: t.to(torch.float64 if t.dtype == torch.float32 else torch.int64),
}


@pytest.mark.parametrize("name", U.WRAPPERS)
def test_strict_tensor_arguments(name):
    L = sub("_lib")
    good = U.valid_args(L, name, "cuda")
    U.call(L, name, good)                                          # the arguments below are valid but for the one that is broken
    torch.cuda.synchronize()
    for arg in U.TENSOR_ARGS[name]:
        for kind, breaks in BROKEN.items():
            bad = breaks(good[arg])
            assert kind != "non-contiguous" or (not bad.is_contiguous() and bad.shape == good[arg].shape)
            with pytest.raises(L.AmpnetError, match=f"^{name}: {arg} must be "):         # (the C ABI's refusals start with "ampnet_")
                U.call(L, name, dict(good, **{arg: bad}))


def _block(path):
    M = sub("pointNet.model.pointnet2_utils")
    train = path.endswith("train")
    if path.startswith("fp"):
        mod = M.PointNetFeaturePropagation(U.D1 + U.D2, U.COUTS, grad=True, batch_stats=train)
    else:
        mod = M.PointNetSetAbstraction(None if path == "sa_all" else U.S, 0.5, U.NSAMPLE, 3 + U.D, U.COUTS, path == "sa_all", grad=True,
                                       batch_stats=train)
    return mod.train(train)


@pytest.mark.parametrize("target", ["feats", "mlp_bns.1.weight", "mlp_convs.0.weight"])
@pytest.mark.parametrize("path", ["sa", "sa_all", "sa_train", "fp", "fp_train"])
def test_gradient_reaches_exactly_what_asked_for_it(path, target):
    g = torch.Generator().manual_seed(3)
    mod = _block(path)
    params = dict(mod.named_parameters())
    for p in params.values():
        p.requires_grad_(False)
    xyz = torch.rand((U.B, 3, U.N), generator=g).cuda()
    feats = torch.rand((U.B, U.D, U.N), generator=g).cuda()
    coarse_xyz = torch.rand((U.B, 3, U.S_COARSE), generator=g).cuda()
    coarse = torch.rand((U.B, U.D2, U.S_COARSE), generator=g).cuda()
    wanted = feats if target == "feats" else params[target]
    wanted.requires_grad_(True)
    out = mod(xyz, coarse_xyz, feats, coarse) if path.startswith("fp") else mod(xyz, feats)[1]
    out.sum().backward()
    torch.cuda.synchronize()
    assert wanted.grad is not None and wanted.grad.shape == wanted.shape       # (the conv weight keeps its trailing singleton dimensions)
    for n, t in [("feats", feats), ("xyz", xyz), ("coarse_xyz", coarse_xyz), ("coarse", coarse)] + list(params.items()):
        assert t is wanted or t.grad is None, (path, target, n)
