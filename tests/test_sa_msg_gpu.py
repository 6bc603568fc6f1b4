"""The multi-branch fused set-abstraction forward (include/ampnet_hip.h: ampnet_sa_msg_forward_f32) through _lib: every branch's column
slice bit for bit the single-branch entry point (sa_forward_f32) on the same groups, on a NaN-prefilled `out` in front of 64 guard
words, twice for the same bits; one case also against the float64 restatement tests/sa_ref.py with its derived bar."""
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
GUARD = -1234.5
DEV = "cuda"
#        name            B  n     s     D    nsamples       widths per branch                       radii
CASES = [("three",       2, 70,   9,    6,   (20, 32, 48),  ([32, 64], [32], [32, 32, 64]),         (0.3, 0.45, 0.6)),     # R = 64 beside R = 32
         ("no_feats",    2, 70,   9,    0,   (8, 40),       ([32, 32], [64]),                       (0.3, 0.6)),
         ("one_branch",  2, 70,   9,    6,   (24,),         ([32, 96],),                            (0.4,)),
         # branch 0: cin_0 = 320, three layers of 256, one wave per workgroup, weights read through L2; branch 1 staged
         ("wide",        1, 64,   3,    317, (32, 16),      ([256, 256, 256], [32]),                (0.6, 0.4)),
         # 4400 groups per branch, more than a branch's 1024 workgroups of 4 waves hold: waves walk several groups, the branch-to-workgroup
         # map goes past one round
         ("many_groups", 4, 2200, 1100, 8,  (2, 2),        ([32], [32, 32]),                       (0.05, 0.1))]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(synth, seed, B, n, s, D, nsamples, radii):
    """Seeded clouds, evenly strided centres, per branch the restatement's ball query."""
    xyz = synth.clouds(seed, B, n)
    feats = synth.uniform(seed * 16 + 7, (B, n, D), -1.0, 1.0).astype(np.float32) if D else None
    cent = np.stack([(np.arange(s) * (n // s) + c) % n for c in range(B)]).astype(np.int32)
    grps = [np.stack([sa_ref.ball_query(xyz[c], cent[c], r, ns)[0] for c in range(B)]) for r, ns in zip(radii, nsamples)]
    return xyz, feats, cent, grps


def _branches(D, widths, seed=17):
    return [sa_ref.make_layers(seed + k, 3 + D, w) for k, w in enumerate(widths)]


def _run_msg(L, xyz, feats, cent, grps, branches, prefill=float("nan"), ws_short=0, out_cols=None, eps=None):
    """-> out [B, s, C] numpy; asserts the 64 guard words behind `out` and the 256 guard bytes behind the workspace"""
    K = len(branches)
    C = sum(b[-1][0].shape[0] for b in branches) if out_cols is None else out_cols
    numel = xyz.shape[0] * cent.shape[1] * C
    buf = torch.full((numel + 64,), prefill, dtype=torch.float32, device=DEV)
    buf[numel:] = GUARD
    out = buf[:numel].view(xyz.shape[0], cent.shape[1], C)
    need = K * L.SA_WORKSPACE_BYTES - ws_short
    ws = torch.full((max(need, 0) + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    try:
        L.sa_msg_forward_f32(_t(xyz), _t(cent), [_t(g) for g in grps], _t(feats), [[tuple(_t(a) for a in layer) for layer in b] for b in branches],
                             [[BN_EPS] * len(b) for b in branches] if eps is None else eps, out, ws[:max(need, 0)])
    finally:
        torch.cuda.synchronize()
        assert (buf[numel:] == GUARD).all(), "written past the end of out"
        assert (ws[max(need, 0):] == 0xAB).all(), "written past the end of the workspace"
    return out.cpu().numpy()


def _run_single(L, xyz, feats, cent, grp, layers):
    out = torch.full((xyz.shape[0], cent.shape[1], layers[-1][0].shape[0]), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(L.SA_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    L.sa_forward_f32(_t(xyz), _t(cent), _t(grp), _t(feats), [tuple(_t(a) for a in layer) for layer in layers], [BN_EPS] * len(layers), out, ws)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def three(synth):
    """The first case's inputs, branches and fused output, shared by the bitwise and the float64 test."""
    L = sub("_lib")
    _, B, n, s, D, nsamples, widths, radii = CASES[0]
    xyz, feats, cent, grps = _inputs(synth, 11, B, n, s, D, nsamples, radii)
    branches = _branches(D, widths)
    return xyz, feats, cent, grps, branches, _run_msg(L, xyz, feats, cent, grps, branches)


@pytest.mark.parametrize("name,B,n,s,D,nsamples,widths,radii", CASES, ids=[c[0] for c in CASES])
def test_every_slice_is_the_single_branch_forward(synth, name, B, n, s, D, nsamples, widths, radii):
    L = sub("_lib")
    xyz, feats, cent, grps = _inputs(synth, 11, B, n, s, D, nsamples, radii)
    branches = _branches(D, widths)
    got = _run_msg(L, xyz, feats, cent, grps, branches)                # the output starts as NaN: every element must be written
    assert got.shape == (B, s, sum(w[-1] for w in widths))
    assert np.isfinite(got).all() and (got > 0).any(), name
    again = _run_msg(L, xyz, feats, cent, grps, branches, prefill=-7.0)
    assert np.array_equal(got, again), name                            # bitwise the same on a second run
    off = 0
    for k, layers in enumerate(branches):
        want = _run_single(L, xyz, feats, cent, grps[k], layers)
        assert np.array_equal(got[..., off:off + want.shape[2]], want), (name, k)
        assert (want > 0).any(), (name, k)
        off += want.shape[2]
    assert off == got.shape[2]


def test_three_branches_within_the_derived_bar(three):
    xyz, feats, cent, grps, branches, got = three
    off = 0
    for k, layers in enumerate(branches):
        worst = 0.0
        for c in range(xyz.shape[0]):
            want, bar = sa_ref.sa_forward(xyz[c], cent[c], grps[k][c], feats[c], layers, [BN_EPS] * len(layers))
            assert (want > 0).mean() > 0.2
            err = np.abs(got[c][:, off:off + want.shape[1]].astype(np.float64) - want)
            worst = max(worst, float(np.max(err / np.maximum(bar, 1e-300))))
        print(f"sa_msg_forward branch {k}: worst error / bar = {worst:.3f}")
        assert worst <= 1.0, (k, worst)
        off += layers[-1][0].shape[0]


def test_refusals(synth):
    """Shapes outside the kernel's limits are errors that name the limit and the branch; nothing is written past out or the workspace."""
    L = sub("_lib")
    xyz, feats, cent, grps = _inputs(synth, 13, 2, 64, 8, 9, (8, 8, 8, 8, 8), (0.5,) * 5)
    ok = sa_ref.make_layers(1, 12, [32])
    with pytest.raises(L.AmpnetError, match="K=0"):
        _run_msg(L, xyz, feats, cent, [], [], out_cols=32)
    with pytest.raises(L.AmpnetError, match="K=5"):
        _run_msg(L, xyz, feats, cent, grps, [ok] * 5)
    with pytest.raises(L.AmpnetError, match="workspace"):
        _run_msg(L, xyz, feats, cent, grps[:2], [ok] * 2, ws_short=1)
    with pytest.raises(L.AmpnetError, match="branch 1.*multiple of 32"):
        _run_msg(L, xyz, feats, cent, grps[:2], [ok, sa_ref.make_layers(1, 12, [32, 48])])
    with pytest.raises(L.AmpnetError, match="branch 2.*layers"):
        _run_msg(L, xyz, feats, cent, grps[:3], [ok, ok, sa_ref.make_layers(1, 12, [32, 32, 32, 32])])
    grp65 = np.zeros((2, 8, 65), np.int32)
    with pytest.raises(L.AmpnetError, match="branch 1.*nsample=65"):
        _run_msg(L, xyz, feats, cent, [grps[0], grp65], [ok, ok])
    big = np.zeros((2, 64, 318), np.float32)
    with pytest.raises(L.AmpnetError, match="320"):
        _run_msg(L, xyz, big, cent, grps[:2], [sa_ref.make_layers(1, 321, [32])] * 2)
    with pytest.raises(L.AmpnetError, match="out"):
        _run_msg(L, xyz, feats, cent, grps[:2], [ok, ok], out_cols=32)
    with pytest.raises(L.AmpnetError, match="branch 1"):
        _run_msg(L, xyz, feats, cent, grps[:2], [ok, sa_ref.make_layers(1, 13, [32])])            # weight [32, 13] against cin_0 = 12
    with pytest.raises(L.AmpnetError):
        _run_msg(L, xyz, feats, cent, grps[:2], [ok, ok], eps=[[BN_EPS], [BN_EPS] * 2])          # one eps per layer
    assert L.sa_msg_forward_workspace_bytes(3) == 3 * L.SA_WORKSPACE_BYTES
