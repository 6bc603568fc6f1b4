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
