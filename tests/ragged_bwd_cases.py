"""The seeded inputs of tests/test_ragged_bwd_gpu.py: clouds of unequal size packed back to back, with GLOBAL indices, as the ragged
searches of the package write them -- here from the CPU restatements (fp_ref.three_nn, sa_ref.ball_query) cloud by cloud plus the offsets,
so that the float64 references (fp_bwd_ref, sa_bwd_ref, fp_train_ref, sa_train_ref) can be run on the packed array as ONE cloud (B = 1).
Test infrastructure: no GPU, no library."""
import numpy as np

import fp_bwd_ref
import fp_ref
import fp_train_ref
import sa_bwd_ref
import sa_ref
import sa_train_ref
from sa_ref import make_layers

SIZES = [128, 129, 200, 200, 511]                  # npoint of the reduced model itself, one more, two equal clouds, no multiple of a 32-row tile
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
TOTAL = int(OFF[-1])
Q = len(SIZES)
BN_EPS = fp_bwd_ref.BN_EPS

# feature propagation: s coarse points per cloud, a subset of its fine points; the last two of cloud 1 are moved away (nobody's neighbour)
FP_S, FP_D1, FP_D2, FP_WIDTHS = 16, 16, 32, [32, 64]
# Train mode: the reference's bars of a batch-normalised layer grow with sqrt(rows) and pile up from layer to layer, and at the ~1200 rows of
# these clouds no beta of a SECOND layer keeps every ReLU input 8 bars from zero (twelve seeds were tried; the references' own train cases
# hold 140 rows).  So the reference is asked about one layer, and depth is checked by bits: the ragged entry point against the uniform one
# on the packed array as one cloud (DEEP_WIDTHS), which the existing layer tests hold to the reference and to composition.
FP_TRAIN_WIDTHS = SA_TRAIN_WIDTHS = [64]
DEEP_WIDTHS = [32, 64, 32]
# set abstraction: s centres per cloud; at this radius most points of the larger clouds are in no group
SA_S, SA_NSAMPLE, SA_D, SA_WIDTHS, SA_RADIUS = 12, 20, 6, [32, 64], 0.35


def _clouds(synth, seed):
    return [synth.clouds(seed + b, 1, n)[0] for b, n in enumerate(SIZES)]


def fp_inputs(synth, train, widths=None):
    """widths=None: the layers the float64 reference takes (below).  Given: those widths, seeded and NOT settled -- for comparisons of bits
    between entry points, which need no ReLU margin.  -> dict: points1 [1, total, D1], points2 [1, Q s, D2], idx int32 / dist2 [1, total, 3] with global coarse indices, local_idx (the
    same relative to the cloud), layers (seeded, then the reference's settle_betas on the packed rows), eps, dout [1, total, cout_last],
    unpicked (global coarse points that are nobody's neighbour)."""
    R = fp_train_ref if train else fp_bwd_ref
    seed = 7100 if train else 7000
    fine = _clouds(synth, seed)
    local, d2 = [], []
    for b, (x, n) in enumerate(zip(fine, SIZES)):
        coarse = np.ascontiguousarray(x[np.arange(FP_S) * (n // FP_S) + 1])
        if b == 1:
            coarse[-2:] += np.float32(50.0)
        i, d = fp_ref.three_nn(x, coarse)
        local.append(i)
        d2.append(d)
    local = np.concatenate(local)
    idx = (local + np.repeat(np.arange(Q, dtype=np.int32) * FP_S, SIZES)[:, None]).astype(np.int32)[None]
    d2 = np.concatenate(d2)[None]
    p1 = synth.uniform(seed * 16 + 5, (1, TOTAL, FP_D1), -1.0, 1.0)
    p2 = synth.uniform(seed * 16 + 6, (1, Q * FP_S, FP_D2), -1.0, 1.0)
    settle = widths is None
    widths = (FP_TRAIN_WIDTHS if train else FP_WIDTHS) if settle else widths
    dout = synth.uniform(seed * 16 + 7, (1, TOTAL, widths[-1]), -1.0, 1.0)
    layers = make_layers(seed + 1, FP_D1 + FP_D2, widths)
    eps = [BN_EPS] * len(widths)
    if settle:
        R.settle_betas(p1, p2, idx, d2, layers, eps)
    unpicked = np.setdiff1d(np.arange(Q * FP_S), idx)
    assert {FP_S + FP_S - 2, FP_S + FP_S - 1} <= set(unpicked.tolist())
    return dict(points1=p1, points2=p2, idx=idx, dist2=d2, local_idx=local.astype(np.int32), layers=layers, eps=eps, dout=dout,
                unpicked=unpicked)


def sa_inputs(synth, train, widths=None):
    """widths: as in fp_inputs.  -> dict: xyz [1, total, 3], centres int32 [1, Q s] and group_idx int32 [1, Q s, nsample] with global point indices, local_centres
    [Q, s] and local_group_idx [Q, s, nsample] (the same relative to the cloud), feats [1, total, D], layers (seeded, then the reference's
    settle_betas on the packed rows), eps, dout [1, Q s, cout_last], unpicked (global points that are in no group)."""
    R = sa_train_ref if train else sa_bwd_ref
    seed = 7300 if train else 7200
    clouds = _clouds(synth, seed)
    cen, grp = [], []
    for x, n in zip(clouds, SIZES):
        c = (np.arange(SA_S) * (n // SA_S) + 1).astype(np.int32)
        g, _ = sa_ref.ball_query(x, c, SA_RADIUS, SA_NSAMPLE)
        cen.append(c)
        grp.append(g.astype(np.int32))
    local_c, local_g = np.stack(cen), np.stack(grp)
    centres = (local_c + OFF[:-1, None]).reshape(1, Q * SA_S).astype(np.int32)
    group_idx = (local_g + OFF[:-1, None, None]).reshape(1, Q * SA_S, SA_NSAMPLE).astype(np.int32)
    xyz = np.concatenate(clouds)[None]
    feats = synth.uniform(seed * 16 + 5, (1, TOTAL, SA_D), -1.0, 1.0)
    settle = widths is None
    widths = (SA_TRAIN_WIDTHS if train else SA_WIDTHS) if settle else widths
    dout = synth.uniform(seed * 16 + 7, (1, Q * SA_S, widths[-1]), -1.0, 1.0)
    layers = make_layers(seed + 1, 3 + SA_D, widths)
    eps = [BN_EPS] * len(widths)
    if settle:
        x, bx = R.input_rows(xyz, centres, group_idx, feats)
        R.settle_betas(x, bx, layers, eps)
    unpicked = np.setdiff1d(np.arange(TOTAL), group_idx)
    assert all(((unpicked >= OFF[b]) & (unpicked < OFF[b + 1])).sum() >= 2 for b in range(Q))      # in every cloud
    return dict(xyz=xyz, centres=centres, group_idx=group_idx, local_centres=local_c, local_group_idx=local_g, feats=feats, layers=layers,
                eps=eps, dout=dout, unpicked=unpicked)
