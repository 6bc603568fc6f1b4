"""The CPU restatement of the 3-nearest-neighbour search (tests/fp_ref.py, spec: include/ampnet_hip.h ampnet_three_nn_f32) against answers
worked out by hand.  No GPU, no library."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fp_ref                                      # noqa: E402

# coarse points on the x axis at 0, 1, 2, 3, 4
LINE = np.array([[float(i), 0.0, 0.0] for i in range(5)], np.float32)


def test_nearest_three_ascending():
    fine = np.array([[0.25, 0, 0], [3.75, 0, 0], [2.0, 0.5, 0]], np.float32)
    idx, d = fp_ref.three_nn(fine, LINE)
    assert idx.dtype == np.int32 and d.dtype == np.float32 and idx.shape == d.shape == (3, 3)
    assert idx.tolist() == [[0, 1, 2], [4, 3, 2], [2, 1, 3]]       # third row: 1 and 3 tie at 1.25, the lower index first
    assert d.tolist() == [[0.0625, 0.5625, 3.0625], [0.0625, 0.5625, 3.0625],
                          [0.25, 1.25, 1.25]]
    assert (np.diff(d, axis=1) >= 0).all()


def test_exact_tie_goes_to_the_lower_index():
    fine = np.array([[0.5, 0, 0], [1.5, 0, 0], [2.0, 0, 0]], np.float32)
    idx, d = fp_ref.three_nn(fine, LINE)
    assert idx.tolist() == [[0, 1, 2], [1, 2, 0], [2, 1, 3]]       # 0.5: 0|1 tie; 1.5: 1|2 tie then 0|3 tie; 2.0: 1|3 tie
    assert d.tolist() == [[0.25, 0.25, 2.25], [0.25, 0.25, 2.25], [0.0, 1.0, 1.0]]
    # the rule does not depend on where the tied points sit in the array: reversed coarse order, reversed winners
    ridx, rd = fp_ref.three_nn(fine, LINE[::-1])
    assert ridx.tolist() == [[3, 4, 2], [2, 3, 1], [2, 1, 3]] and np.array_equal(rd, d)


def test_duplicated_coarse_points():
    coarse = np.array([[1, 1, 1], [0, 0, 0], [1, 1, 1], [1, 1, 1], [0, 0, 0]], np.float32)
    idx, d = fp_ref.three_nn(np.array([[1, 1, 1], [0, 0, 0.25]], np.float32), coarse)
    assert idx.tolist() == [[0, 2, 3], [1, 4, 0]]
    assert d.tolist() == [[0.0, 0.0, 0.0], [0.0625, 0.0625, 2.5625]]


def test_fewer_than_three_coarse_points():
    fine = np.array([[0.75, 0, 0], [0.25, 0, 0]], np.float32)
    idx, d = fp_ref.three_nn(fine, LINE[:1])
    assert idx.shape == d.shape == (2, 1) and idx.tolist() == [[0], [0]] and d.tolist() == [[0.5625], [0.0625]]
    idx, d = fp_ref.three_nn(fine, LINE[:2])
    assert idx.shape == d.shape == (2, 2) and idx.tolist() == [[1, 0], [0, 1]] and d.tolist() == [[0.0625, 0.5625], [0.0625, 0.5625]]
    idx, d = fp_ref.three_nn(fine, LINE[:3])
    assert idx.shape == (2, 3) and idx.tolist() == [[1, 0, 2], [0, 1, 2]]


def test_extra_columns_are_ignored():
    rng = np.random.default_rng(3)
    fine, coarse = rng.random((20, 3), np.float32), rng.random((9, 3), np.float32)
    a = fp_ref.three_nn(fine, coarse)
    wide_f = np.concatenate([fine, 50.0 + fine, fine], 1)          # 9 columns
    wide_c = np.concatenate([coarse, -7.0 * coarse[:, :2]], 1)     # 5 columns
    b = fp_ref.three_nn(wide_f, wide_c)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_distance_is_the_difference_form_rounded_per_operation():
    fine = np.array([[0.1, 0.2, 0.3]], np.float32)
    coarse = np.array([[0.7, -0.4, 0.9]], np.float32)
    dx, dy, dz = (fine[0] - coarse[0]).astype(np.float32)
    want = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
    idx, d = fp_ref.three_nn(fine, coarse)
    assert d[0, 0] == want and d[0, 0].tobytes() == want.tobytes()
