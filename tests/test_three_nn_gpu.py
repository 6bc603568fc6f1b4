"""3-nearest-neighbour kernel (BUILD-DEFINED spec, include/ampnet_hip.h: ampnet_three_nn_f32) against the build's own CPU restatement
(tests/fp_ref.py: three_nn): indices and squared distances bit for bit."""
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


def _check(U, fine, coarse):
    """fine [B, n, ld1], coarse [B, s, ld2] numpy -> the kernel's (idx, dist2), asserted bit-equal to the restatement per cloud."""
    idx, d = U.three_nn(torch.from_numpy(fine).cuda(), torch.from_numpy(coarse).cuda())
    k = min(3, coarse.shape[1])
    assert idx.dtype == torch.int32 and d.dtype == torch.float32
    assert idx.shape == d.shape == (fine.shape[0], fine.shape[1], k)
    idx, d = idx.cpu().numpy(), d.cpu().numpy()
    for c in range(fine.shape[0]):
        want_i, want_d = fp_ref.three_nn(fine[c], coarse[c])
        assert np.array_equal(idx[c], want_i), (c, np.argwhere(idx[c] != want_i)[:4])
        assert idx[c].tobytes() == want_i.tobytes() and d[c].tobytes() == want_d.tobytes(), c
    return idx, d


@pytest.mark.parametrize("n,s", [(70, 5), (256, 64), (1000, 333)])
def test_three_nn_matches_restatement(synth, n, s):
    """A tail that is no multiple of 64, s smaller than a wave, more than one workgroup per cloud."""
    idx, d = _check(sub("utils.utils"), synth.clouds(31, 2, n), synth.clouds(32, 2, s))
    assert (np.diff(d, axis=2) >= 0).all() and (d > 0).all()
    assert all(len(set(row)) == 3 for row in idx[0])               # three different neighbours


@pytest.mark.parametrize("s", [1, 2, 3])
def test_three_nn_with_at_most_three_coarse_points(synth, s):
    idx, d = _check(sub("utils.utils"), synth.clouds(33, 2, 70), synth.clouds(34, 2, s))
    assert idx.shape[2] == s and (np.sort(idx, axis=2) == np.arange(s)).all()        # every coarse point, each once


def test_three_nn_exact_ties_on_an_integer_grid():
    """Fine points at the centres of grid cells and of cell faces: 8 or 4 coarse grid points at exactly the same distance; the lower
    indices win, in index order."""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)    # 75 points
    inner = g[(g[:, 0] < 4) & (g[:, 1] < 4) & (g[:, 2] < 2)]                                                                   # 32 cells
    fine = np.concatenate([inner + np.float32(0.5), inner + np.array([0.5, 0.5, 0.0], np.float32), g], 0)[None]
    idx, d = _check(sub("utils.utils"), fine, g[None])
    tied = d[0, :, 0] == d[0, :, 2]
    assert tied[:64].all() and not tied[64:].any()                 # the cell and face centres see a tie of all three, the grid points do not
    assert (d[0, :32] == 0.75).all() and (d[0, 32:64] == 0.5).all()
    assert (idx[0, :64, 0] < idx[0, :64, 1]).all() and (idx[0, :64, 1] < idx[0, :64, 2]).all()
    assert (d[0, 64:, 0] == 0).all() and (idx[0, 64:, 0] == np.arange(75)).all()
    assert (d[0, 64:, 1] == 1).all() and (idx[0, 64:, 1] < idx[0, 64:, 2]).all()     # two of the grid neighbours at distance 1


def test_three_nn_coarse_subset_of_fine(synth):
    """The real case: the coarse points are sampled FROM the fine ones, so distance 0 appears."""
    fine = synth.clouds(35, 2, 300)
    pick = (np.arange(37) * 8 + 1) % 300
    idx, d = _check(sub("utils.utils"), fine, np.ascontiguousarray(fine[:, pick]))
    assert (d[:, pick, 0] == 0).all() and (idx[:, pick, 0] == np.arange(37)).all()
    assert ((d[..., 0] == 0).sum(1) == 37).all() and (d[..., 1] > 0).all()


def test_three_nn_wide_rows_and_different_clouds(synth):
    """ld1 != ld2 > 3 (the extra columns are ignored), B = 3 with different clouds."""
    fine, coarse = synth.clouds(36, 3, 130, dims=9), synth.clouds(37, 3, 21, dims=5)
    idx, d = _check(sub("utils.utils"), fine, coarse)
    narrow = _check(sub("utils.utils"), np.ascontiguousarray(fine[..., :3]), np.ascontiguousarray(coarse[..., :3]))
    assert np.array_equal(idx, narrow[0]) and np.array_equal(d, narrow[1])
    assert not np.array_equal(idx[0], idx[1]) and not np.array_equal(idx[1], idx[2])


def test_three_nn_argument_errors(synth):
    U, L = sub("utils.utils"), sub("_lib")
    fine = torch.from_numpy(synth.clouds(38, 2, 64)).cuda()
    coarse = torch.from_numpy(synth.clouds(39, 2, 8)).cuda()
    with pytest.raises(L.AmpnetError):
        U.three_nn(fine.cpu(), coarse)                             # no CPU fallback
    with pytest.raises(L.AmpnetError):
        U.three_nn(fine, coarse.cpu())
    with pytest.raises(IndexError):
        U.three_nn(fine, coarse[:, :0])                            # s = 0
    with pytest.raises(IndexError):
        U.three_nn(fine, torch.zeros((2, L.THREE_NN_MAX_S + 1, 3), device="cuda"))        # the coarse coordinates must fit LDS
    with pytest.raises(L.AmpnetError):
        U.three_nn(fine, coarse[:1])                               # batch mismatch
    with pytest.raises(L.AmpnetError):
        U.three_nn(fine[..., :2], coarse)                          # fewer than 3 columns
    # the library itself refuses what the wrapper refuses
    idx = torch.empty((2, 64, 3), dtype=torch.int32, device="cuda")
    d = torch.empty((2, 64, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(L.AmpnetError, match="s="):
        L.three_nn_f32(fine, torch.zeros((2, L.THREE_NN_MAX_S + 1, 3), device="cuda"), idx, d)
    with pytest.raises(L.AmpnetError):
        L.three_nn_f32(fine, coarse, idx[:, :32], d)               # output of the wrong shape
    i, dd = U.three_nn(fine[:1], torch.zeros((1, L.THREE_NN_MAX_S, 3), device="cuda"))   # the limit itself is accepted
    assert i.shape == (1, 64, 3) and (i[0, :, 0] == 0).all() and (i[0, :, 2] == 2).all()
