"""Ragged ball query (include/ampnet_hip.h: ampnet_ball_query_ragged_f32): clouds of unequal size in one launch, cloud by cloud bit for bit
the uniform kernel on that cloud alone and the build's CPU restatement (tests/sa_ref.py: ball_query); global indices; refusals."""
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

SIZES = [1, 63, 64, 65, 130, 300]                  # below, at and above a wave's 64 candidates; more than one step of the walk
S = 8


@pytest.fixture(scope="module")
def packed(synth):
    """(clouds as numpy [n_b, 3], sizes, centres [Q, S] numpy int32): SIZES from synth.clouds plus a 100-point cloud repeated cyclically to
    250 points, so that exact duplicates -- equal distances, members at a ball's boundary several times over -- occur."""
    clouds = [synth.clouds(70 + b, 1, n)[0] for b, n in enumerate(SIZES)]
    clouds.append(synth.clouds(90, 1, 100)[0][np.arange(250) % 100])
    sizes = [c.shape[0] for c in clouds]
    centres = np.stack([(np.arange(S) * 7) % n for n in sizes]).astype(np.int32)
    return clouds, sizes, centres


@pytest.mark.parametrize("nsample", [1, 16, 64])
@pytest.mark.parametrize("radius", [0.0, 0.15, 10.0])
def test_ragged_equals_the_uniform_kernel_and_the_restatement_cloud_by_cloud(packed, nsample, radius):
    U = sub("utils.utils")
    clouds, sizes, centres = packed
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    cent = torch.from_numpy(centres).cuda()
    out, count = U.ball_query_ragged(rows, sizes, cent, radius, nsample, return_counts=True)
    glob, gcount = U.ball_query_ragged(rows, sizes, cent, radius, nsample, return_counts=True, global_index=True)
    only = U.ball_query_ragged(rows, sizes, cent, radius, nsample)                                 # count = NULL
    assert out.dtype == torch.int32 and count.dtype == torch.int32
    assert tuple(out.shape) == (len(sizes), S, nsample) and tuple(count.shape) == (len(sizes), S)
    assert torch.equal(only, out) and torch.equal(gcount, count)
    off = 0
    for b, (pc, n) in enumerate(zip(clouds, sizes)):
        alone, acount = U.ball_query(torch.from_numpy(pc).cuda()[None], cent[b:b + 1], radius, nsample, return_counts=True)
        assert torch.equal(out[b], alone[0]) and torch.equal(count[b], acount[0]), (b, n)
        assert torch.equal(glob[b], alone[0] + off), (b, n)
        want, wcount = sa_ref.ball_query(pc, centres[b], radius, nsample)
        assert np.array_equal(out[b].cpu().numpy(), want) and np.array_equal(count[b].cpu().numpy(), wcount), (b, n)
        off += n
    if radius == 10.0:                              # every point is a member: truncated at nsample, or the whole cloud and padding
        assert count.cpu().tolist() == [[min(n, nsample)] * S for n in sizes]


def test_one_launch_over_a_late_member_cloud_a_cloud_above_the_staging_threads_and_a_single_point():
    """Three clouds in one launch.  (1) The 311-point line-plus-cluster cloud of test_ball_query_gpu.py::
    test_members_past_the_first_step_are_found: members past empty steps of the walk.  (2) The 1216-point integer grid with duplicates of
    that file's _grid_cloud(): more points than the 1024 threads that stage a cloud, so every thread stages a second row, and at radius 1.0
    d == r2 exactly for the axis neighbours.  (3) One point.  The ragged kernel and the uniform one share their walk: cloud by cloud the
    lists and counts are the uniform call's and the restatement's, and global_index adds the cloud's first row to EVERY entry, padding
    included."""
    U = sub("utils.utils")
    line = np.stack([10.0 * np.arange(300), np.zeros(300), np.zeros(300)], 1)
    line[130] = line[2]
    line[299] = line[2]
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    clouds = [np.concatenate([line, np.array([5000.0, 7.0, -3.0]) + 0.01 * np.arange(11)[:, None]]).astype(np.float32),
              np.concatenate([g, g[:64], np.zeros((128, 3), np.float32)], 0),
              np.array([[0.25, -1.5, 3.0]], np.float32)]
    sizes = [c.shape[0] for c in clouds]
    assert sizes == [311, 1216, 1]
    centres = np.array([[305, 2, 300, 310, 64], [0, 5, 341, 1023, 1215], [0, 0, 0, 0, 0]], dtype=np.int32)
    assert sa_ref.ball_query(clouds[0], centres[0], 0.5, 16)[1].tolist() == [11, 3, 11, 11, 1]
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    cent = torch.from_numpy(centres).cuda()
    for radius, nsample in ((0.5, 1), (0.5, 3), (0.5, 16), (1.0, 7)):
        out, count = U.ball_query_ragged(rows, sizes, cent, radius, nsample, return_counts=True)
        glob, gcount = U.ball_query_ragged(rows, sizes, cent, radius, nsample, return_counts=True, global_index=True)
        assert tuple(out.shape) == (3, 5, nsample) and tuple(count.shape) == (3, 5)
        off, alone = 0, []
        for b, (pc, n) in enumerate(zip(clouds, sizes)):
            lists, acount = U.ball_query(torch.from_numpy(pc).cuda()[None], cent[b:b + 1], radius, nsample, return_counts=True)
            want, wcount = sa_ref.ball_query(pc, centres[b], radius, nsample)
            assert torch.equal(out[b], lists[0]) and torch.equal(count[b], acount[0]), (radius, nsample, b)
            assert np.array_equal(out[b].cpu().numpy(), want) and np.array_equal(count[b].cpu().numpy(), wcount), (radius, nsample, b)
            alone.append(lists[0] + off)
            off += n
        assert torch.equal(gcount, count)
        for b in range(3):
            assert torch.equal(glob[b], alone[b]), (radius, nsample, b)
        assert count[2].tolist() == [1] * 5 and glob[2].unique().tolist() == [311 + 1216]      # the single point: one member, then padding


def test_a_wider_row_and_a_layout_object_give_the_same_lists(packed):
    """ld = 9 (the model's packed rows) and a RaggedLayout built once, as the model hands them over."""
    U = sub("utils.utils")
    clouds, sizes, centres = packed
    xyz = np.concatenate(clouds)
    rows9 = torch.from_numpy(np.concatenate([xyz, np.ones((xyz.shape[0], 6), np.float32)], 1)).cuda()
    cent = torch.from_numpy(centres).cuda()
    want = U.ball_query_ragged(torch.from_numpy(xyz).cuda(), sizes, cent, 0.15, 16, global_index=True)
    lay = U.ragged_layout("test", rows9, sizes)
    assert lay.off.dtype == torch.int32 and lay.off.cpu().tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist() and lay.max_n == 300
    assert torch.equal(U.ball_query_ragged(rows9, lay, cent, 0.15, 16, global_index=True, _trusted_centres=True), want)


def test_refusals(packed):
    U, L = sub("utils.utils"), sub("_lib")
    clouds, sizes, centres = packed
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    cent = torch.from_numpy(centres).cuda()
    with pytest.raises(L.AmpnetError, match="do not tile"):
        U.ball_query_ragged(rows, sizes[:-1] + [sizes[-1] - 1], cent, 0.1, 4)
    with pytest.raises(L.AmpnetError, match="do not tile"):
        U.ball_query_ragged(rows, [0] + sizes, torch.zeros((len(sizes) + 1, S), dtype=torch.int32, device="cuda"), 0.1, 4)
    big = torch.zeros((12289 + 5, 3), device="cuda")
    with pytest.raises(L.AmpnetError, match="cloud 1 has 12289 points"):
        U.ball_query_ragged(big, [5, 12289], torch.zeros((2, 1), dtype=torch.int32, device="cuda"), 0.1, 4)
    bad = cent.clone()
    bad[3, 2] = sizes[3]                            # one past its cloud's end, though a valid row of the packed array
    with pytest.raises(L.AmpnetError, match="out of its cloud's range") as e:
        U.ball_query_ragged(rows, sizes, bad, 0.1, 4)
    assert isinstance(e.value, IndexError)          # ball_query's error type for it, too
    bad[3, 2] = -1
    with pytest.raises(L.AmpnetError, match="out of its cloud's range"):
        U.ball_query_ragged(rows, sizes, bad, 0.1, 4)
    with pytest.raises(IndexError, match="nsample"):
        U.ball_query_ragged(rows, sizes, cent, 0.1, 65)
    with pytest.raises(L.AmpnetError, match="radius"):
        U.ball_query_ragged(rows, sizes, cent, -1.0, 4)
    with pytest.raises(L.AmpnetError, match="int32"):
        U.ball_query_ragged(rows, sizes, cent.long(), 0.1, 4)
    with pytest.raises(L.AmpnetError, match=r"centres \[Q, S\]"):
        U.ball_query_ragged(rows, sizes, cent[:-1], 0.1, 4)
