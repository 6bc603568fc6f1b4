"""The fused feature-propagation forward (include/ampnet_hip.h: ampnet_fp_forward_f32) against the float64 restatement tests/fp_ref.py.
The kernel is fed the restatement's own neighbours and squared distances, so only the interpolation, the concatenation and the shared MLP
are judged.  The bar is derived in fp_ref.fp_forward's docstring; the worst error / bar ratio of every case is printed."""
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

pytestmark = pytest.mark.gpu

BN_EPS = 1e-5
GUARD = -1234.5
#        name               N    S   D1   D2   widths            negative gammas
CASES = [("one_layer",      70,  5,  0,   32,  [32],             False),
         ("odd_cin",        70,  9,  7,   32,  [64, 32],         False),
         ("fp2_form",       100, 16, 64,  256, [256, 128],       False),      # the 320-wide input, weights read through L2
         ("fp3_form",       64,  8,  128, 256, [256, 256],       False),      # the 384-wide input, one wave per workgroup
         ("fp1_form",       33,  4,  0,   128, [128, 128, 128],  False),
         ("one_coarse",     70,  1,  7,   32,  [64, 32],         False),      # k = 1: the "repeat" branch
         ("two_coarse",     70,  2,  0,   32,  [32],             False),      # k = 2
         ("negative_gamma", 70,  9,  7,   32,  [64, 32],         True),
         # no layer's weights fit beside two waves' 265 + 257 wide tiles: layer 0 (cin = 263) is read dword by dword with column
         # 263 of its last block of 8 masked (not read), layer 1 (cin = 256) by dwordx4
         ("odd_wide",       40,  6,  7,   256, [256, 32],        False)]


def _inputs(synth, seed, n, s, D1, D2):
    """Two seeded clouds; the coarse points are a subset of the fine ones (the real case); the restatement's neighbour search."""
    fine = synth.clouds(seed, 2, n)
    pick = np.arange(s) * (n // s) + 1
    coarse = np.ascontiguousarray(fine[:, pick])
    p1 = synth.uniform(seed * 16 + 5, (2, n, D1), -1.0, 1.0) if D1 else None
    p2 = synth.uniform(seed * 16 + 6, (2, s, D2), -1.0, 1.0)
    idx, d2 = zip(*(fp_ref.three_nn(fine[c], coarse[c]) for c in range(2)))
    return p1, p2, np.stack(idx), np.stack(d2), pick


def _run(L, p1, p2, idx, d2, layers, prefill=float("nan"), eps=None):
    """-> out [B, N, cout] as numpy.  The output lives in front of 8 guard rows, which the kernel must leave alone."""
    dev = "cuda"
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, N = idx.shape[:2]
    cout = layers[-1][0].shape[0]
    buf = torch.full((B * N + 8, cout), prefill, dtype=torch.float32, device=dev)
    buf[B * N:] = GUARD
    out = buf[:B * N].view(B, N, cout)
    ws = torch.empty(L.FP_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
    L.fp_forward_f32(t(p1), t(p2), t(idx), t(d2), [tuple(t(a) for a in layer) for layer in layers],
                     [BN_EPS] * len(layers) if eps is None else eps, out, ws)
    assert (buf[B * N:] == GUARD).all(), "rows past the last cloud were written"
    return out.cpu().numpy()


@pytest.mark.parametrize("name,n,s,D1,D2,widths,neg", CASES, ids=[c[0] for c in CASES])
def test_fp_forward_within_the_derived_bar(synth, name, n, s, D1, D2, widths, neg):
    L = sub("_lib")
    p1, p2, idx, d2, pick = _inputs(synth, 41, n, s, D1, D2)
    k = min(3, s)
    assert idx.shape == d2.shape == (2, n, k)
    assert n % 32 != 0 or name == "fp3_form"                       # a partial last tile in every case but the one that fills its tiles
    layers = fp_ref.make_layers(43, D1 + D2, widths, negative_gamma=neg)
    if neg:
        assert all((layer[2] < 0).any() and (layer[2] > 0).any() for layer in layers)
    got = _run(L, p1, p2, idx, d2, layers)                         # the output starts as NaN: every element must be written
    assert np.isfinite(got).all(), name
    again = _run(L, p1, p2, idx, d2, layers, prefill=-7.0)
    assert np.array_equal(got, again), name                        # bitwise the same on a second run
    assert not np.array_equal(got[0], got[1])                      # the second cloud has its own result
    worst = worst_zero = 0.0
    for c in range(2):
        want, bar = fp_ref.fp_forward(None if p1 is None else p1[c], p2[c], idx[c], d2[c], layers, [BN_EPS] * len(layers))
        assert want.shape == got[c].shape and (want > 0).mean() > 0.2          # the ReLU did not wipe the case out
        ratio = np.abs(got[c].astype(np.float64) - want) / np.maximum(bar, 1e-300)
        worst = max(worst, float(ratio.max()))
        # the fine points that ARE coarse points: distance 0, that neighbour's weight is 1 up to 1e-8 / d of the next one
        zero = np.nonzero(d2[c][:, 0] == 0)[0]
        assert np.array_equal(zero, pick), (zero, pick)
        if k > 1:
            assert (d2[c][zero, 1] > 1e-4).all()
            r = 1.0 / (d2[c][zero].astype(np.float64) + np.float64(np.float32(1e-8)))
            assert ((r[:, 0] / r.sum(1)) > 1.0 - 1e-4).all()
        worst_zero = max(worst_zero, float(ratio[zero].max()))
    print(f"fp_forward {name}: worst error / bar = {worst:.3f} (rows at distance 0: {worst_zero:.3f})")
    assert worst <= 1.0, (name, worst)


def test_fp_forward_is_exact_fp32_whatever_the_precision_scope(synth):
    L = sub("_lib")
    p1, p2, idx, d2, _ = _inputs(synth, 44, 70, 9, 7, 32)
    layers = fp_ref.make_layers(45, 39, [64, 32])
    base = _run(L, p1, p2, idx, d2, layers)
    with L.precision_scope("bf16"):
        assert np.array_equal(_run(L, p1, p2, idx, d2, layers), base)


def test_fp_forward_clamps_neighbour_indices(synth):
    """An index outside the coarse cloud is clamped into it, as sa_forward_kernel clamps its group indices: no read out of range."""
    L = sub("_lib")
    p1, p2, idx, d2, _ = _inputs(synth, 46, 70, 9, 0, 32)
    layers = fp_ref.make_layers(47, 32, [32])
    wild = idx.copy()
    wild[:, ::3, 1] = 1 << 30
    wild[:, 1::3, 2] = -5
    want = _run(L, p1, p2, np.clip(wild, 0, 8), d2, layers)
    assert np.array_equal(_run(L, p1, p2, wild, d2, layers), want)


def test_fp_forward_refusals(synth):
    """Shapes outside the kernel's limits are errors of the library that name the limit, not faults: there is no other path."""
    L = sub("_lib")
    p1, p2, idx, d2, _ = _inputs(synth, 48, 70, 9, 7, 32)
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, p1, p2, idx, d2, fp_ref.make_layers(1, 39, [48]))
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        _run(L, p1, p2, idx, d2, fp_ref.make_layers(1, 39, [32, 288]))
    wide1, wide2 = np.zeros((2, 70, 257), np.float32), np.zeros((2, 9, 256), np.float32)
    with pytest.raises(L.AmpnetError, match="512"):
        _run(L, wide1, wide2, idx, d2, fp_ref.make_layers(1, 513, [32]))
    assert _run(L, wide1[..., :256], wide2, idx, d2, fp_ref.make_layers(1, 512, [32])).shape == (2, 70, 32)      # 512 itself is accepted
    with pytest.raises(L.AmpnetError, match="layers"):
        _run(L, p1, p2, idx, d2, fp_ref.make_layers(1, 39, [32, 32, 32, 32]))
    short = fp_ref.make_layers(1, 39, [64, 32])
    short[1] = (short[1][0][:-1],) + short[1][1:]                  # weight [31, 64]: one row short
    with pytest.raises(L.AmpnetError, match="fp_forward: layer 1 needs"):
        _run(L, p1, p2, idx, d2, short)                            # the binding refuses it: the kernel would read past its end
    with pytest.raises(L.AmpnetError, match="fp_forward: layer 0 needs"):
        _run(L, p1, p2, idx, d2, fp_ref.make_layers(1, 40, [32]))  # weight [32, 40] against cin_0 = 39
    with pytest.raises(L.AmpnetError):
        _run(L, p1[:, :69], p2, idx, d2, fp_ref.make_layers(1, 39, [32]))         # points1 of another N
    with pytest.raises(L.AmpnetError):
        _run(L, p1, p2, idx, d2, fp_ref.make_layers(1, 39, [32]), eps=[BN_EPS] * 2)
