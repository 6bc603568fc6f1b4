"""The CPU restatement of the ball query (tests/sa_ref.py, spec: include/ampnet_hip.h ampnet_ball_query_f32) against answers worked out by
hand on a 4 x 4 x 1 integer grid: point (x, y, 0) has index 4 x + y."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sa_ref                                      # noqa: E402

GRID = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(1), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def test_boundary_is_included():
    """radius 1.0: the four axis neighbours sit at d == r2 == 1 exactly and are members; the diagonals (d = 2) are not."""
    idx, cnt = sa_ref.ball_query(GRID, [5, 0, 15, 7], 1.0, 5)
    assert idx.dtype == np.int32 and cnt.dtype == np.int32
    assert idx[0].tolist() == [1, 4, 5, 6, 9] and cnt[0] == 5              # interior point (1, 1)
    assert idx[1].tolist() == [0, 1, 4, 0, 0] and cnt[1] == 3              # corner (0, 0)
    assert idx[2].tolist() == [11, 14, 15, 11, 11] and cnt[2] == 3         # corner (3, 3)
    assert idx[3].tolist() == [3, 6, 7, 11, 3] and cnt[3] == 4             # edge (1, 3)


def test_just_below_the_boundary_excludes_it():
    idx, cnt = sa_ref.ball_query(GRID, [5], np.nextafter(np.float32(1.0), np.float32(0.0)), 4)
    assert idx[0].tolist() == [5, 5, 5, 5] and cnt[0] == 1


def test_truncation_at_nsample():
    """radius 1.5 (r2 = 2.25) takes the 3 x 3 block round (1, 1): nine members, the first nsample in index order are kept."""
    idx, cnt = sa_ref.ball_query(GRID, [5], 1.5, 16)
    assert idx[0, :9].tolist() == [0, 1, 2, 4, 5, 6, 8, 9, 10] and cnt[0] == 9
    idx, cnt = sa_ref.ball_query(GRID, [5, 10], 1.5, 4)
    assert idx[0].tolist() == [0, 1, 2, 4] and cnt[0] == 4                 # the centre itself (5) is cut off
    assert idx[1].tolist() == [5, 6, 7, 9] and cnt[1] == 4
    idx, cnt = sa_ref.ball_query(GRID, [5], 1.0, 1)
    assert idx[0].tolist() == [1] and cnt[0] == 1


def test_padding_repeats_the_first_member():
    idx, cnt = sa_ref.ball_query(GRID, [10, 12], 1.0, 8)
    assert idx[0].tolist() == [6, 9, 10, 11, 14, 6, 6, 6] and cnt[0] == 5  # first member 6, not the centre 10
    assert idx[1].tolist() == [8, 12, 13, 8, 8, 8, 8, 8] and cnt[1] == 3
    idx, cnt = sa_ref.ball_query(GRID, [3], 0.0, 3)                        # radius 0: the point alone
    assert idx[0].tolist() == [3, 3, 3] and cnt[0] == 1


def test_extra_columns_are_ignored():
    wide = np.concatenate([GRID, 100.0 * np.arange(16 * 6, dtype=np.float32).reshape(16, 6)], 1)
    a = sa_ref.ball_query(wide, [5, 0], 1.0, 6)
    b = sa_ref.ball_query(GRID, [5, 0], 1.0, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
