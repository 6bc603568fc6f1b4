"""CPU restatements of the PointNet++ feature-propagation kernels, written from the spec in include/ampnet_hip.h (ampnet_three_nn_f32,
ampnet_fp_forward_f32): float32 for the neighbour search, float64 for the interpolation and the MLP.  Test infrastructure: no GPU, no
library."""
import numpy as np

from sa_ref import EPS32, make_layers, mlp_chain     # noqa: F401  (make_layers: re-exported for the tests)

# roundings between the float32 inputs and one interpolated feature, see fp_forward
C_INTERP = 11.0


def sq_dists(fine, coarse):
    """float32 ((dx*dx + dy*dy) + dz*dz) from every fine point to every coarse point, one rounding per operation -> [n, s]."""
    f = np.ascontiguousarray(np.asarray(fine)[:, :3], dtype=np.float32)
    c = np.ascontiguousarray(np.asarray(coarse)[:, :3], dtype=np.float32)
    d = f[:, None, :] - c[None, :, :]
    sq = d * d
    out = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    assert out.dtype == np.float32
    return out


def three_nn(fine, coarse):
    """fine [n, >=3], coarse [s, >=3] float32 -> (idx int32 [n, k], dist2 float32 [n, k]), k = min(3, s): per fine point the k coarse
    points with the smallest (d, index), ascending, d = float32 ((dx*dx + dy*dy) + dz*dz) with one rounding per operation."""
    dist = sq_dists(fine, coarse)
    k = min(3, dist.shape[1])
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]          # stable: equal distances keep the index order
    return order.astype(np.int32), np.take_along_axis(dist, order, 1)


def fp_forward(points1, points2, idx, dist2, layers, eps):
    """One cloud.  points1 [n, D1] float32 or None, points2 [s, D2] float32, idx [n, k] and dist2 [n, k] float32 (three_nn's output, taken
    as exact), layers as sa_ref.make_layers with cin_0 = D1 + D2, eps per layer -> (out float64 [n, cout_last], bar float64 likewise).

    out: float64 evaluation of the layers relu(bn_eval(W row + b)) on row_i = [points1[i], sum_k w_k points2[idx_k]],
    w_k = r_k / sum_k r_k, r_k = 1 / (dist2_k + float32(1e-8)), bn_eval(v) = (v - mean) / sqrt(var + eps) * gamma + beta.

    bar: the float32 error bound per output element, derived as in sa_ref.sa_forward.  With e = 2^-24:
      * input: the points1 columns are exact.  An interpolated column is the float32 value of sum_k w_k f_k, every operation rounding once
        (relative error <= e; no operation here can underflow for features and distances of ordinary size).  The kernel forms
        r_k = 1 / (dist2_k + 1e-8f): 2 roundings;  sum_k r_k: <= 2 additions on top of the 2 of every r_k, so <= 4;  w_k = r_k / sum: 1 more,
        in all 2 + 4 + 1 = 7 on w_k;  then the product w_k f_k and <= 2 additions of the 3-term sum: 3 (a fused multiply-add only
        removes one).  Every term w_k f_k therefore carries <= 10 roundings, a relative error (1 + e)^10 - 1 < 11 e:
            |err| <= C_INTERP e sum_k |w_k f_k|,  C_INTERP = 11;
      * the layers: sa_ref.mlp_chain."""
    d = np.asarray(dist2, dtype=np.float64)
    r = 1.0 / (d + np.float64(np.float32(1e-8)))
    w = r / r.sum(1, keepdims=True)
    terms = w[..., None] * np.asarray(points2, dtype=np.float64)[np.asarray(idx)]          # [n, k, D2]
    rows = terms.sum(1)
    b_in = C_INTERP * EPS32 * np.abs(terms).sum(1)
    if points1 is not None:
        p1 = np.asarray(points1, dtype=np.float64)
        rows = np.concatenate([p1, rows], -1)
        b_in = np.concatenate([np.zeros_like(p1), b_in], -1)
    return mlp_chain(rows, b_in, layers, eps)
