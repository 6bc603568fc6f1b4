"""Ragged 3-NN (include/ampnet_hip.h: ampnet_three_nn_ragged_f32): fine clouds of unequal size, each against its own S coarse points, in one
launch -- cloud by cloud bit for bit the uniform kernel on that cloud alone; global indices; refusals."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conftest import sub                           # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 600]                    # below, at and above one workgroup of 256 fine points; three workgroups


@pytest.fixture(scope="module")
def fine(synth):
    """SIZES from synth.clouds plus a 100-point cloud repeated cyclically to 250 points (equal fine points must get equal answers)."""
    clouds = [synth.clouds(30 + b, 1, n)[0] for b, n in enumerate(SIZES)]
    clouds.append(synth.clouds(50, 1, 100)[0][np.arange(250) % 100])
    return clouds, [c.shape[0] for c in clouds]


@pytest.mark.parametrize("s", [1, 2, 3, 37])
def test_ragged_equals_the_uniform_kernel_cloud_by_cloud(synth, fine, s):
    U = sub("utils.utils")
    clouds, sizes = fine
    Q = len(sizes)
    coarse = synth.clouds(60 + s, Q, s)
    if s >= 3:
        coarse[:, 2] = coarse[:, 0]                # an exact duplicate among the coarse points: equal distances, the lower index first
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    cx = torch.from_numpy(coarse).cuda()
    idx, d2 = U.three_nn_ragged(rows, sizes, cx)
    gidx, gd2 = U.three_nn_ragged(rows, sizes, cx, global_index=True)
    k = min(3, s)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and tuple(idx.shape) == tuple(d2.shape) == (sum(sizes), k)
    assert torch.equal(gd2, d2)
    off = 0
    for b, (pc, n) in enumerate(zip(clouds, sizes)):
        want_idx, want_d2 = U.three_nn(torch.from_numpy(pc).cuda()[None], cx[b:b + 1])
        assert torch.equal(idx[off:off + n], want_idx[0]) and torch.equal(d2[off:off + n], want_d2[0]), (b, n)
        assert torch.equal(gidx[off:off + n], want_idx[0] + b * s), (b, n)
        off += n
    if s >= 3:                                      # the duplicate pair comes out as (0, 2), never (2, 0)
        both = (idx == 0).any(1) & (idx == 2).any(1)
        assert both.any() and ((idx == 0).int().argmax(1) < (idx == 2).int().argmax(1))[both].all()
    dup = idx[off - 250:off]                        # the cyclic cloud: row j and row j + 100 are the same point
    assert torch.equal(dup[:100], dup[100:200]) and torch.equal(dup[:50], dup[200:250])


def test_more_coarse_points_than_staging_threads(synth):
    """s = 300 coarse points per cloud: more than the 256 threads that stage them, so 44 threads stage a second row; fine clouds of 1 and
    257 points (a workgroup with one live lane, twice).  Coarse point 2 is a copy of point 0."""
    U = sub("utils.utils")
    sizes, s = [1, 257], 300
    clouds = [synth.clouds(40 + b, 1, n)[0] for b, n in enumerate(sizes)]
    coarse = synth.clouds(45, len(sizes), s)
    coarse[:, 2] = coarse[:, 0]
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    cx = torch.from_numpy(coarse).cuda()
    idx, d2 = U.three_nn_ragged(rows, sizes, cx)
    gidx, gd2 = U.three_nn_ragged(rows, sizes, cx, global_index=True)
    assert tuple(idx.shape) == tuple(d2.shape) == (sum(sizes), 3)
    off = 0
    for b, (pc, n) in enumerate(zip(clouds, sizes)):
        want_idx, want_d2 = U.three_nn(torch.from_numpy(pc).cuda()[None], cx[b:b + 1])
        assert torch.equal(idx[off:off + n], want_idx[0]) and torch.equal(d2[off:off + n], want_d2[0]), (b, n)
        assert torch.equal(gidx[off:off + n], want_idx[0] + b * s) and torch.equal(gd2[off:off + n], want_d2[0]), (b, n)
        off += n


def test_wider_rows_and_a_layout_object_give_the_same_answers(synth, fine):
    U = sub("utils.utils")
    clouds, sizes = fine
    xyz = np.concatenate(clouds)
    coarse = synth.clouds(77, len(sizes), 37)
    want = U.three_nn_ragged(torch.from_numpy(xyz).cuda(), sizes, torch.from_numpy(coarse).cuda(), global_index=True)
    rows9 = torch.from_numpy(np.concatenate([xyz, np.ones((xyz.shape[0], 6), np.float32)], 1)).cuda()
    coarse5 = torch.from_numpy(np.concatenate([coarse, np.ones(coarse.shape[:2] + (2,), np.float32)], 2)).cuda()
    got = U.three_nn_ragged(rows9, U.ragged_layout("test", rows9, sizes), coarse5, global_index=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_refusals(fine):
    U, L = sub("utils.utils"), sub("_lib")
    clouds, sizes = fine
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    coarse = torch.zeros((len(sizes), 4, 3), device="cuda")
    with pytest.raises(L.AmpnetError, match="do not tile"):
        U.three_nn_ragged(rows, sizes[:-1], coarse[:-1])
    with pytest.raises(L.AmpnetError, match="fine clouds"):
        U.three_nn_ragged(rows, sizes, coarse[:-1])
    with pytest.raises(IndexError, match="coarse points out of range"):
        U.three_nn_ragged(rows, sizes, coarse[:, :0])
    with pytest.raises(L.AmpnetError, match="expected fine_rows"):
        U.three_nn_ragged(rows[None], sizes, coarse)
