"""Ball-query grouping kernel (BUILD-DEFINED spec, include/ampnet_hip.h: ampnet_ball_query_f32) against the build's own CPU restatement
(tests/sa_ref.py: ball_query): indices and counts bit for bit.  The reference has no ball query."""
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


def _check(U, pc, cent, radius, nsample):
    """pc [B, n, ld] numpy, cent [B, s] numpy int32: GPU == restatement; returns the restatement's counts [B, s]."""
    got, cnt = U.ball_query(torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda(), radius, nsample, return_counts=True)
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy()
    assert got.dtype == np.int32 and cnt.dtype == np.int32 and got.shape == cent.shape + (nsample,)
    want_cnt = []
    for c in range(pc.shape[0]):
        want, wc = sa_ref.ball_query(pc[c], cent[c], radius, nsample)
        assert np.array_equal(cnt[c], wc), (radius, nsample, c)
        assert np.array_equal(got[c], want), (radius, nsample, c)
        want_cnt.append(wc)
    only = U.ball_query(torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda(), radius, nsample)      # count = NULL
    assert np.array_equal(only.cpu().numpy(), got)
    return np.stack(want_cnt)


@pytest.mark.parametrize("n,s,nsample", [(100, 10, 1), (1000, 64, 16), (2048, 256, 32), (777, 33, 64)])
def test_ball_query_matches_restatement(synth, n, s, nsample):
    """Three radii per shape, chosen from the seeded cloud by the distance d_k of every centre to its k-th nearest point (k counts the
    centre): (a) below most centres' d_nsample -- most balls hold fewer than nsample points and are padded; (b) the median d_nsample -- a
    mix; (c) above every centre's d_(nsample+1) -- every ball is truncated.  The regimes are asserted on the restatement's counts first.
    With nsample = 1 the centre alone fills its ball at every radius, so (a) and (b) cannot be had: all three radii give count 1."""
    U = sub("utils.utils")
    pc = synth.clouds(5, 2, n)
    cent = U.fps_indices(torch.from_numpy(pc).cuda(), s).cpu().numpy()
    dk = np.array([[np.sort(sa_ref.sq_dists(pc[c], i))[[nsample - 1, nsample]] for i in cent[c]] for c in range(2)], dtype=np.float64)
    radii = {"a": np.sqrt(np.quantile(dk[..., 0], 0.1)) * 0.999 if nsample > 1 else 1e-3,
             "b": np.sqrt(np.median(dk[..., 0])) if nsample > 1 else 0.05,
             "c": np.sqrt(dk[..., 1].max()) * 1.001}
    for regime, radius in radii.items():
        want = np.stack([sa_ref.ball_query(pc[c], cent[c], radius, nsample)[1] for c in range(2)])
        members = np.stack([sa_ref.ball_query(pc[c], cent[c], radius, n)[1] for c in range(2)])               # uncapped
        if nsample == 1:
            assert (want == 1).all()
        elif regime == "a":
            assert (want < nsample).mean() > 0.5, (regime, want)
        elif regime == "b":
            assert 0.2 < (want < nsample).mean() < 0.8, (regime, want)
        if regime == "c":
            assert (want == nsample).all() and (members > nsample).all(), (regime, members)
        assert np.array_equal(_check(U, pc, cent, float(radius), nsample), want)


def _grid_cloud():
    """The cloud of test_knn_gpu.py::test_knn_ties_and_duplicates: an integer grid, 64 duplicated points, 128 copies of the origin."""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return np.concatenate([g, g[:64], np.zeros((128, 3), np.float32)], 0)[None]


def test_radius_zero_takes_the_duplicates_only():
    U = sub("utils.utils")
    pc = _grid_cloud()
    cent = np.array([[0, 5, 100, 1023, 1024 + 5, pc.shape[1] - 1]], dtype=np.int32)
    got, cnt = U.ball_query(torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda(), 0.0, 8, return_counts=True)
    got, cnt = got.cpu().numpy()[0], cnt.cpu().numpy()[0]
    assert got[1].tolist() == [5, 1029, 5, 5, 5, 5, 5, 5] and cnt[1] == 2          # the point and its copy, in index order
    assert got[4].tolist() == got[1].tolist() and cnt[4] == 2                      # asked from the copy: the same ball
    assert got[2].tolist() == [100] * 8 and cnt[2] == 1                            # no copy of point 100
    assert got[0].tolist() == [0, 1024, 1088, 1089, 1090, 1091, 1092, 1093] and cnt[0] == 8      # the origin: 130 copies, truncated
    _check(U, pc, cent, 0.0, 8)
    _check(U, pc, cent, 0.0, 64)


@pytest.mark.parametrize("radius", [1.0, 2.0])
def test_exact_boundary_ties_on_the_integer_grid(radius):
    """Every squared distance is a small integer: d == r2 exactly for the axis neighbours, and they are members."""
    U = sub("utils.utils")
    pc = _grid_cloud()
    cent = np.array([[0, 5, 100, 341, 1023, 1024, pc.shape[1] - 1]], dtype=np.int32)
    for nsample in (4, 7, 40, 64):
        cnt = _check(U, pc, cent, radius, nsample)
    assert cnt[0, 3] == (7 if radius == 1.0 else 32)       # point 341 = (5, 5, 1): 6 neighbours at d = 1; 33 lattice points within d <= 4, (5, 5, -1) is off the grid


def test_members_past_the_first_step_are_found():
    """Points 0 .. 299 lie 10 apart on a line, points 300 .. 310 are a tight cluster: a centre inside the cluster has no member among
    the first 64 candidates (nor the next 192), so a wave that stopped after an empty step would return nothing.  A second centre's
    members straddle empty steps: point 2 and its copies at 130 and 299."""
    U = sub("utils.utils")
    line = np.stack([10.0 * np.arange(300), np.zeros(300), np.zeros(300)], 1)
    line[130] = line[2]
    line[299] = line[2]
    cluster = np.array([5000.0, 7.0, -3.0]) + 0.01 * np.arange(11)[:, None]
    pc = np.concatenate([line, cluster]).astype(np.float32)[None]
    cent = np.array([[305, 2, 300, 310, 64]], dtype=np.int32)
    for nsample in (1, 3, 16):
        cnt = _check(U, pc, cent, 0.5, nsample)
    assert cnt[0].tolist() == [11, 3, 11, 11, 1]
    got = U.ball_query(torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda(), 0.5, 16).cpu().numpy()[0]
    assert got[0, :11].tolist() == list(range(300, 311)) and got[1, :4].tolist() == [2, 130, 299, 2]


def test_rows_wider_than_three_columns(synth):
    U = sub("utils.utils")
    pc = synth.clouds(6, 2, 500, dims=9)                                           # ld = 9: columns 3 .. 8 must not matter
    cent = U.fps_indices(torch.from_numpy(pc).cuda(), 20).cpu().numpy()
    _check(U, pc, cent, 0.15, 16)
    cnt = _check(U, pc, cent, 0.15, 4)                                             # padded and truncated balls side by side
    assert (cnt < 4).any() and (cnt == 4).any()
    narrow = U.ball_query(torch.from_numpy(np.ascontiguousarray(pc[..., :3])).cuda(), torch.from_numpy(cent).cuda(), 0.15, 4)
    wide = U.ball_query(torch.from_numpy(pc).cuda(), torch.from_numpy(cent).cuda(), 0.15, 4)
    assert torch.equal(narrow, wide)


def test_ball_query_argument_errors(synth):
    U = sub("utils.utils")
    x = torch.from_numpy(synth.clouds(4, 1, 64)).cuda()
    c = torch.zeros((1, 4), dtype=torch.int32).cuda()
    with pytest.raises(IndexError):
        U.ball_query(x, c, 0.1, 0)
    with pytest.raises(IndexError):
        U.ball_query(x, c, 0.1, 65)
    with pytest.raises(Exception):
        U.ball_query(x.cpu(), c, 0.1, 4)           # no CPU fallback
    with pytest.raises(IndexError):
        U.ball_query(x, c + 64, 0.1, 4)
    with pytest.raises(IndexError):
        U.ball_query(x, c - 1, 0.1, 4)
    with pytest.raises(Exception):
        U.ball_query(x, c.long(), 0.1, 4)          # centres must be int32
    with pytest.raises(Exception):
        U.ball_query(x, c, -1.0, 4)
    big = torch.zeros((1, 12289, 3), device="cuda")
    with pytest.raises(Exception, match="12289"):
        U.ball_query(big, c, 0.1, 4)               # coordinates must fit LDS
    assert U.ball_query(torch.zeros((1, 12288, 3), device="cuda"), c, 0.0, 2).shape == (1, 4, 2)
