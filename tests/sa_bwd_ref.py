"""CPU restatement of the set-abstraction backward, written from the spec in include/ampnet_hip.h (ampnet_sa_backward_f32), in float64,
with a derived float32 error bar per output element; and the seeded cases of tests/test_sa_backward_gpu.py, so that the CPU test
(tests/test_sa_bwd_ref_cpu.py) can check the yardstick and the seeds without a GPU.  Test infrastructure: no GPU, no library."""
import numpy as np

import sa_ref
from fp_bwd_ref import BN_EPS, RELU_MARGIN, forward_layer
from sa_ref import EPS32, make_layers

# full64: the seeded cloud is scaled by 0.625 (x, y in [-0.625, 0.625]) so that every ball of radius 0.9 holds at least 64 of the 150 points --
# at the other cases' density no seed of sixty gives five centres with 64 distinct members each, which is what the case is there for.
#         name               n    s   nsample  D    widths            radius  seed
CASES = [("tail_group",      70,  9,  20,      6,   [32, 64],         0.35,   0),
         ("no_feats",        70,  9,  32,      0,   [32],             0.35,   0),
         ("two_tiles",       150, 5,  48,      13,  [32, 32, 64],     0.6,    0),
         ("full64",          150, 5,  64,      16,  [64],             0.9,    0),
         ("sa2_form",        96,  6,  32,      64,  [64, 64, 128],    0.5,    0),
         ("sa3_form",        64,  4,  32,      128, [128, 128, 256],  0.6,    0),
         ("negative_gamma",  70,  9,  20,      16,  [32, 64, 32],     0.35,   0),
         ("sparse_ball",     70,  9,  16,      8,   [32, 32],         0.12,   0),
         ("unpicked",        70,  9,  16,      8,   [32, 32],         0.12,   0),
         ("widest",          64,  3,  32,      317, [256, 256, 256],  0.6,    0)]
N_CLOUDS = 2


def case_inputs(synth, name):
    """The seeded inputs of case `name` as a dict of numpy arrays: xyz [2, n, 3], centres [2, s] int32 (arange(s) * (n // s) + 1),
    group_idx [2, s, nsample] int32 and count [2, s] (sa_ref.ball_query), feats [2, n, D] or None, layers (seeded, then settle_betas), eps,
    dout [2, s, cout_last], unpicked (per cloud the points that are in no group).  full64's cloud is scaled by 0.625 (see the table)."""
    _, n, s, nsample, D, widths, radius, seed = next(c for c in CASES if c[0] == name)
    base = 3000 + 97 * seed + 7 * [c[0] for c in CASES].index(name)
    xyz = synth.clouds(base, N_CLOUDS, n)
    if name == "full64":
        xyz = xyz * np.float32(0.625)                       # denser: at the clouds' own density no ball of radius 0.9 holds 64 of 150 points everywhere
    centres = np.tile((np.arange(s) * (n // s) + 1).astype(np.int32), (N_CLOUDS, 1))
    group_idx, count = (np.stack(a) for a in zip(*(sa_ref.ball_query(xyz[c], centres[c], radius, nsample) for c in range(N_CLOUDS))))
    feats = synth.uniform(base * 16 + 5, (N_CLOUDS, n, D), -1.0, 1.0) if D else None
    dout = synth.uniform(base * 16 + 7, (N_CLOUDS, s, widths[-1]), -1.0, 1.0)
    layers = make_layers(base + 1, 3 + D, widths, negative_gamma=name == "negative_gamma")
    if name == "negative_gamma":
        assert all((layer[2] < 0).any() and (layer[2] > 0).any() for layer in layers)
        layers[0][2][1] = 0.0                               # one gamma exactly 0
    eps = [BN_EPS] * len(widths)
    x, bx = input_rows(xyz, centres, group_idx, feats)
    settle_betas(x, bx, layers, eps)
    unpicked = [np.setdiff1d(np.arange(n), group_idx[c]) for c in range(N_CLOUDS)]
    if name == "unpicked":
        assert all(len(u) >= 2 for u in unpicked)
    if name == "sparse_ball":
        assert (count == 1).any() and count.max() <= 3      # some ball holds its centre alone
    if name == "full64":
        assert (count == nsample).all()                     # every slot a distinct member
    if name in ("tail_group", "two_tiles"):
        assert (count < nsample).any()                      # repeated slots
    return dict(xyz=xyz, centres=centres, group_idx=group_idx, count=count, feats=feats, layers=layers, eps=eps, dout=dout,
                unpicked=unpicked, nsample=nsample)


def input_rows(xyz, centres, group_idx, feats):
    """-> (x_0 [B s nsample, 3 + D] float64, its float32 bar): rows [xyz[idx_t] - xyz[centre], feats[idx_t]] formed exactly from the float32
    inputs; the kernel rounds the three coordinate differences once (e |dx|, sa_ref.sa_forward's rule), the features are exact."""
    p = np.asarray(xyz, dtype=np.float64)[..., :3]
    B, n = p.shape[:2]
    idx = np.clip(np.asarray(group_idx), 0, n - 1)
    cen = np.clip(np.asarray(centres), 0, n - 1)
    rows = np.stack([p[c][idx[c]] - p[c][cen[c]][:, None, :] for c in range(B)])                      # [B, s, nsample, 3]
    bx = EPS32 * np.abs(rows)
    if feats is not None:
        f = np.stack([np.asarray(feats[c], dtype=np.float64)[idx[c]] for c in range(B)])
        rows = np.concatenate([rows, f], -1)
        bx = np.concatenate([bx, np.zeros_like(f)], -1)
    return rows.reshape(-1, rows.shape[-1]), bx.reshape(-1, rows.shape[-1])


def settle_betas(x, bx, layers, eps, margin=2.0 * RELU_MARGIN, step=2.0 ** -10):
    """fp_bwd_ref.settle_betas on the rows (x, bx): moves the BatchNorm biases of `layers`, in place, channel by channel in steps of
    +-2^-10 to the nearest float32 value at which no ReLU input of the channel lies within `margin` x its bar of zero (twice the margin
    sa_backward asserts).  Everything else about the case stays as seeded."""
    for layer, e in zip(layers, eps):
        beta = layer[3]
        a, ba, _, _, _, scale, _, bm = forward_layer(x, bx, layer, e)         # (none of these depends on beta)
        pre, fixed = (a + bm) * scale, np.abs(scale) * ba + 6.0 * EPS32 * (np.abs(a * scale) + np.abs(bm * scale))
        for c in range(len(beta)):
            b0 = np.float32(beta[c])
            for j in range(4096):
                beta[c] = b0 + np.float32(((j + 1) // 2) * (step if j % 2 else -step))
                if (np.abs(pre[:, c] + np.float64(beta[c])) > margin * (fixed[:, c] + 6.0 * EPS32 * abs(np.float64(beta[c])))).all():
                    break
            else:
                raise AssertionError(f"no beta near {b0} clears channel {c}")
        _, _, y, by, *_ = forward_layer(x, bx, layer, e)
        assert (np.abs(y) > margin * by).all()
        x, bx = np.maximum(y, 0.0), by


def output_names(L, has_feats):
    return (["dfeats"] if has_feats else []) + [f"{k}{l}" for l in range(L) for k in ("dW", "dbias", "dgamma", "dbeta")]


def forward_tape(xyz, centres, group_idx, feats, layers, eps, margin=RELU_MARGIN):
    """-> (tape, worst): per layer (x, bx, W, a, ba, y, by, scale, inv, b - mean) in float64 on the M = B s nsample rows; asserts the
    ReLU margin of fp_bwd_ref.fp_backward on every ReLU input of every layer."""
    x, bx = input_rows(xyz, centres, group_idx, feats)
    tape, worst = [], np.inf
    for layer, e in zip(layers, eps):
        a, ba, y, by, W, scale, inv, bm = forward_layer(x, bx, layer, e)
        worst = min(worst, float((np.abs(y) / np.maximum(by, 1e-300)).min()))
        tape.append((x, bx, W, a, ba, y, by, scale, inv, bm))
        x, bx = np.maximum(y, 0.0), by
    assert worst > margin, f"a ReLU input lies within {margin} x its bar of zero (|y| / bar = {worst:.3g}): choose other inputs"
    return tape, worst


def float64_argmax(tape, group_idx):
    """The lowest row of every (group, column) that attains the float64 maximum of relu(y): [B, s, cout_last] int32 (for the CPU tests;
    the GPU test takes the kernel's own choice)."""
    B, s, nsample = np.asarray(group_idx).shape
    v = np.maximum(tape[-1][5], 0.0).reshape(B, s, nsample, -1)
    return v.argmax(2).astype(np.int32)


def check_argmax(arg, tape, group_idx):
    """Asserts for every (group, column) that the row `arg` [B, s, cout_last] is one the max may select: 0 <= arg < nsample; the float64
    relu(y) at `arg` is within bar(arg row) + bar(top row) of the float64 maximum (either float32 value may be off by its bar); and `arg`
    is the first occurrence of its source point in the group (repeated slots are bit-identical, the lowest row wins)."""
    idx = np.asarray(group_idx)
    B, s, nsample = idx.shape
    arg = np.asarray(arg).astype(np.int64)
    y, by = (t.reshape(B, s, nsample, -1) for t in (tape[-1][5], tape[-1][6]))
    assert arg.shape == (B, s, y.shape[-1]), arg.shape
    assert (arg >= 0).all() and (arg < nsample).all(), "arg outside [0, nsample)"
    v = np.maximum(y, 0.0)
    top = v.argmax(2)[:, :, None, :]
    pick = arg[:, :, None, :]
    gap = np.take_along_axis(v, top, 2) - np.take_along_axis(v, pick, 2)
    slack = np.take_along_axis(by, top, 2) + np.take_along_axis(by, pick, 2)
    assert (gap <= slack).all(), f"arg is not a maximum: worst gap / slack = {float((gap / np.maximum(slack, 1e-300)).max()):.3g}"
    first = np.ones((B, s, nsample), bool)
    for t in range(1, nsample):
        first[:, :, t] = (idx[:, :, :t] != idx[:, :, t:t + 1]).all(-1)
    assert np.take_along_axis(first, arg.reshape(B, s, -1), 2).all(), "arg is a repeated slot, not the first occurrence of its point"


def sa_backward(xyz, centres, group_idx, feats, layers, eps, dout, arg, tape=None):
    """xyz [B, n, >= 3] float32, centres [B, s], group_idx [B, s, nsample] (taken as exact), feats [B, n, D] float32 or None, layers as
    sa_ref.make_layers, eps per layer, dout [B, s, cout_last], arg [B, s, cout_last] the row the max selected (an INPUT, like idx / dist2 of
    fp_bwd_ref.fp_backward: with float32 bars the runner-up often lies within the winner's bar, so the restatement must not decide it;
    check_argmax says whether a given choice is admissible) -> {name: (value, bar)} with the names of output_names().

    Values.  Rows x_0 = [xyz[idx_t] - xyz[centre], feats[idx_t]], M = B s nsample of them.  Per layer a = x W^T, y = (a + b - mean) scale +
    beta, x_{l+1} = relu(y).  dx_L[(g, t), c] = dout[g, c] where t = arg[g, c], 0 elsewhere; then fp_bwd_ref.fp_backward's walk:
    dy = dx [y > 0], dbeta = sum dy, G = sum dy a, dgamma = (G + (b - mean) dbeta) / sqrt(var + eps), dz = dy scale, dbias = scale dbeta,
    dW = dz^T x_l, dx_l = dz W.  dfeats[j] = sum over the entries with group_idx = j (clamped) of dx_0[entry, 3:].

    Bars, e = 2^-24: fp_bwd_ref.fp_backward's rules with M = B s nsample, and
      * x_0: e |dx| on the three coordinate differences, the features exact (sa_ref.sa_forward);
      * the last layer's dx is an exact selection of dout: bar 0;
      * dfeats[j], a plain sum of its c_j terms:  sum b_dx0 + 8 e sqrt(c_j) sum |dx_0| + 2 e |dfeats|.  A point in no group has value 0 and
        bar 0: it must come back as exact zeros."""
    if tape is None:
        tape, _ = forward_tape(xyz, centres, group_idx, feats, layers, eps)
    idx = np.asarray(group_idx)
    B, s, nsample = idx.shape
    n = np.asarray(xyz).shape[1]
    idx = np.clip(idx, 0, n - 1)
    M = B * s * nsample
    cl = tape[-1][5].shape[1]
    dx4 = np.zeros((B, s, nsample, cl))
    np.put_along_axis(dx4, np.asarray(arg).astype(np.int64)[:, :, None, :], np.asarray(dout, dtype=np.float64)[:, :, None, :], 2)
    dx, bdx = dx4.reshape(M, cl), np.zeros((M, cl))
    out, sq = {}, np.sqrt(M)
    for l in range(len(layers) - 1, -1, -1):
        x, bx, W, a, ba, y, _, scale, inv, bm = tape[l]
        mask = y > 0.0
        dy, bdy = dx * mask, bdx * mask
        dbeta = dy.sum(0)
        b_dbeta = bdy.sum(0) + 8.0 * EPS32 * sq * np.abs(dy).sum(0) + 2.0 * EPS32 * np.abs(dbeta)
        G = (dy * a).sum(0)
        b_G = (bdy * np.abs(a) + np.abs(dy) * ba + bdy * ba).sum(0) + 8.0 * EPS32 * sq * np.abs(dy * a).sum(0) + 2.0 * EPS32 * np.abs(G)
        out[f"dbeta{l}"] = (dbeta, b_dbeta)
        out[f"dgamma{l}"] = ((G + bm * dbeta) * inv,
                             inv * (b_G + np.abs(bm) * b_dbeta) + 6.0 * EPS32 * inv * (np.abs(G) + np.abs(bm * dbeta)))
        out[f"dbias{l}"] = (scale * dbeta, np.abs(scale) * b_dbeta + 4.0 * EPS32 * np.abs(scale * dbeta))
        dz = dy * scale
        bdz = bdy * np.abs(scale) + 4.0 * EPS32 * np.abs(dz)
        dW = dz.T @ x
        out[f"dW{l}"] = (dW, bdz.T @ np.abs(x) + np.abs(dz).T @ bx + bdz.T @ bx + 8.0 * EPS32 * sq * (np.abs(dz).T @ np.abs(x))
                         + 2.0 * EPS32 * np.abs(dW))
        dx = dz @ W
        bdx = bdz @ np.abs(W) + 8.0 * EPS32 * np.sqrt(W.shape[0]) * (np.abs(dz) @ np.abs(W)) + 2.0 * EPS32 * np.abs(dx)
    if feats is not None:
        D = feats.shape[2]
        g, bg = dx[:, 3:].reshape(B, s * nsample, D), bdx[:, 3:].reshape(B, s * nsample, D)
        df, carry, mag = (np.zeros((B, n, D)) for _ in range(3))
        cnt = np.zeros((B, n, 1))
        for c in range(B):
            flat = idx[c].reshape(-1)
            np.add.at(df[c], flat, g[c])
            np.add.at(carry[c], flat, bg[c])
            np.add.at(mag[c], flat, np.abs(g[c]))
            np.add.at(cnt[c], flat, 1.0)
        out["dfeats"] = (df, carry + 8.0 * EPS32 * np.sqrt(cnt) * mag + 2.0 * EPS32 * np.abs(df))
    return out
