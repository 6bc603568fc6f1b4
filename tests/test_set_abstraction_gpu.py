"""The fused set-abstraction forward (include/ampnet_hip.h: ampnet_sa_forward_f32) against the float64 restatement tests/sa_ref.py.  The
kernel is fed the restatement's own group indices, so only the gather, the shared MLP and the max are judged.  The bar is the float32
bound of tests/pw_probe.py::bar pushed through the chain (sa_ref.sa_forward's docstring derives it); the worst error / bar ratio of every
case is printed."""
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

BN_EPS = 1e-5
#        name               n    s  nsample  D   widths           radius  negative gammas
CASES = [("sa1_form",       512, 64, 32,     9,  [32, 32, 64],    0.25,   False),
         ("sa2_form",       256, 32, 32,     64, [64, 64, 128],   0.35,   False),
         ("sa3_form",       128, 16, 32,     128, [128, 128, 256], 0.5,   False),
         ("pad_16_rows",    256, 32, 16,     9,  [32, 32, 64],    0.3,    False),
         ("tile_64_rows",   256, 32, 64,     9,  [32, 32, 64],    0.5,    False),
         ("no_feats",       256, 32, 32,     0,  [32, 32, 64],    0.35,   False),
         ("two_layers",     256, 32, 32,     9,  [64, 96],        0.35,   False),
         ("one_layer",      200, 20, 24,     5,  [160],           0.35,   False),
         ("wide_input",     96,  8,  40,     317, [256, 32],      0.6,    False),
         # cin_0 = 313 in 320 padded columns, one wave per workgroup, no layer staged: weight columns 313 .. 319 are masked, not read
         ("wide_odd_input", 96,  8,  40,     310, [256, 32],      0.6,    False),
         ("negative_gamma", 256, 32, 32,     9,  [32, 64, 32],    0.35,   True),
         ("lonely_groups",  256, 32, 32,     9,  [32, 32, 64],    0.02,   False)]


def _inputs(synth, seed, n, s, nsample, D, radius):
    """Two seeded clouds, evenly strided centres, the restatement's ball query."""
    xyz = synth.clouds(seed, 2, n)
    feats = synth.uniform(seed * 16 + 7, (2, n, D), -1.0, 1.0).astype(np.float32) if D else None
    cent = np.stack([(np.arange(s) * (n // s) + c) % n for c in range(2)]).astype(np.int32)
    grp, cnt = zip(*(sa_ref.ball_query(xyz[c], cent[c], radius, nsample) for c in range(2)))
    return xyz, feats, cent, np.stack(grp), np.stack(cnt)


def _run(L, xyz, feats, cent, grp, layers, prefill=float("nan"), eps=None, ws_bytes=None):
    dev = "cuda"
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = torch.full((xyz.shape[0], cent.shape[1], layers[-1][0].shape[0]), prefill, dtype=torch.float32, device=dev)
    ws = torch.empty(L.SA_WORKSPACE_BYTES if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=dev)
    L.sa_forward_f32(t(xyz), t(cent), t(grp), t(feats), [tuple(t(a) for a in layer) for layer in layers],
                     [BN_EPS] * len(layers) if eps is None else eps, out, ws)
    return out.cpu().numpy()


@pytest.mark.parametrize("name,n,s,nsample,D,widths,radius,neg", CASES, ids=[c[0] for c in CASES])
def test_sa_forward_within_the_derived_bar(synth, name, n, s, nsample, D, widths, radius, neg):
    L = sub("_lib")
    xyz, feats, cent, grp, cnt = _inputs(synth, 11, n, s, nsample, D, radius)
    if name == "lonely_groups":
        assert (cnt == 1).mean() > 0.5, cnt                        # most groups are one point repeated nsample times
    layers = sa_ref.make_layers(17, 3 + D, widths, negative_gamma=neg)
    if neg:
        assert all((layer[2] < 0).any() and (layer[2] > 0).any() for layer in layers)
    got = _run(L, xyz, feats, cent, grp, layers)                   # the output starts as NaN: every element must be written
    assert np.isfinite(got).all(), name
    again = _run(L, xyz, feats, cent, grp, layers, prefill=-7.0)
    assert np.array_equal(got, again), name                        # bitwise the same on a second run
    worst = 0.0
    for c in range(2):
        want, bar = sa_ref.sa_forward(xyz[c], cent[c], grp[c], None if feats is None else feats[c], layers, [BN_EPS] * len(layers))
        assert want.shape == got[c].shape and (want > 0).mean() > 0.2          # the ReLU did not wipe the case out
        worst = max(worst, float(np.max(np.abs(got[c].astype(np.float64) - want) / np.maximum(bar, 1e-300))))
    print(f"sa_forward {name}: worst error / bar = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


def test_sa_forward_ignores_extra_xyz_columns_and_the_precision_scope(synth):
    """xyz rows may be wider than 3 (ld = 6); the result is exact fp32 whatever matrix precision is in force."""
    L = sub("_lib")
    xyz, feats, cent, grp, _ = _inputs(synth, 12, 256, 32, 32, 9, 0.3)
    layers = sa_ref.make_layers(18, 12, [32, 64])
    base = _run(L, xyz, feats, cent, grp, layers)
    wide = np.concatenate([xyz, 50.0 + xyz], -1)
    assert np.array_equal(_run(L, wide, feats, cent, grp, layers), base)
    with L.precision_scope("bf16"):
        assert np.array_equal(_run(L, xyz, feats, cent, grp, layers), base)


def test_sa_forward_refusals(synth):
    """Shapes outside the kernel's limits are errors that name the limit: there is no other path."""
    L = sub("_lib")
    xyz, feats, cent, grp, _ = _inputs(synth, 13, 64, 8, 8, 9, 0.5)
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, xyz, feats, cent, grp, sa_ref.make_layers(1, 12, [32, 48]))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, xyz, feats, cent, grp, sa_ref.make_layers(1, 12, [288]))
    big = np.zeros((2, 64, 318), np.float32)
    with pytest.raises(L.AmpnetError, match="320"):
        _run(L, xyz, big, cent, grp, sa_ref.make_layers(1, 321, [32]))
    with pytest.raises(L.AmpnetError, match="layers"):
        _run(L, xyz, feats, cent, grp, sa_ref.make_layers(1, 12, [32, 32, 32, 32]))
    with pytest.raises(L.AmpnetError):
        _run(L, xyz, feats, cent, grp, sa_ref.make_layers(1, 13, [32]))           # weight [32, 13] against cin_0 = 12
    with pytest.raises(L.AmpnetError):
        _run(L, xyz, feats, cent, grp, sa_ref.make_layers(1, 12, [32]), eps=[BN_EPS] * 2)          # one eps per layer
    with pytest.raises(L.AmpnetError):
        _run(L, xyz, feats, cent, grp, sa_ref.make_layers(1, 12, [32]), ws_bytes=L.SA_WORKSPACE_BYTES - 1)
